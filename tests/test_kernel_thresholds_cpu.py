"""The size and grid thresholds that tests/test_gpu_full_size_oracle.py built its SIZES table from, read from the HIP
sources.  A tuning change that moves one fails here, naming the table entry to move, instead of leaving a full-size GPU
case quietly on another kernel variant."""
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "mat_mul_amd" / "csrc"
MiB = 1 << 20


def source(name):
    return (CSRC / name).read_text()


# (file, regex whose first group is the value, the value SIZES assumes, the SIZES entries that rest on it)
PINS = [
    ("tg_device.h", r"constexpr int64_t kStreamOutBytes = (\d+)ll << 20;", 128,
     "expand_s4_nt, expand_s16_nt, expand_s25_keyed, step_emit_s4_two_launches, step_emit_s16_two_launches"),
    ("tg_kernels.hip", r"const int64_t out_bytes16 = B \* T \* (\d+) \* \(out_dtype \? 2 : 4\);", 4096, "step_emit_s16_two_launches"),
    # the fused generator declines an S=9 target whose game stride is not a multiple of 16 (or R beyond 256): only then does
    # tg_gen_demos_i8 reach the capped basis-token grid
    ("tg_kernels.hip", r"if \(!aligned\(target, 16\) \|\| stride % (\d+) != 0\) return 0;", 16, "gen_s9_basis_grid_cap"),
    ("tg_kernels.hip", r"if \(!\(S == 9 \|\| S == 16 \|\| S == 25\) \|\| R > (\d+) \|\| B == 0\) return 0;", 256,
     "gen_s9_basis_grid_cap"),
    ("tg_kernels.hip", r"constexpr int64_t kS4TokenWaitBytes = (\d+)ll << 20;", 384, "step_s4_nt_loads, step_s4_token_wait"),
    ("tg_kernels.hip", r"constexpr int64_t kNtLoadsFromBytes = (\d+)ll << 20", 320,
     "step_s16_lines, step_s16_nt_loads, step_s25_lines, step_s25_nt_loads"),
    ("tg_kernels.hip", r"kNtLoadsToBytes = (\d+)ll << 20;", 1280,
     "step_s16_nt_loads, step_s16_lds_pad, step_s25_nt_loads, step_s25_lds_pad"),
    ("tg_kernels.hip", r"constexpr int64_t kLanesFrom = (\d+);", 57344, "stream_s4_rounds (the lane kernel's layout)"),
    ("tg_kernels.hip", r"constexpr int64_t kTrackedSparse25 = (\d+);", 2048, "tracked_s25_sparse"),
    # the S=4 step: non-temporal loads from 96 MiB, the alternating sweep above 16 MiB
    ("tg_kernels.hip", r"constexpr int64_t kS4NtLoadsFromBytes = (\d+)ll << 20;", 96, "step_s4_plain_reversed, step_s4_nt_loads"),
    ("tg_kernels.hip", r"constexpr int64_t kS4SweepAboveBytes = (\d+)ll << 20;", 16, "step_s4_plain_one_way, step_s4_plain_reversed"),
    # S=16 / S=25 whole-line stores from 96 MiB
    ("tg_kernels.hip", r"constexpr int64_t kLinesFromBytes = (\d+)ll << 20;", 96, "step_s16_lines"),
    ("tg_kernels.hip", r"constexpr int64_t kLinesFromBytes = (\d+)ll << 20;", 96, "step_s25_lines"),
    # copy: by the bytes of both buffers, and the byte path's grid
    ("tg_kernels.hip", r"kCopyNtStoresAboveBytes = (\d+)ll << 20;", 640, "copy_s16_nt1, copy_s16_nt2"),
    ("tg_kernels.hip", r"constexpr int64_t kCopyNtLoadsAboveBytes = (\d+)ll << 20,", 256, "copy_s16_nt1"),
    ("tg_kernels.hip", r"copy_bytes_kernel, grid_for\(B, (\d+)\)", 65536, "copy_bytes_grid_cap"),
    # grid caps
    ("tg_kernels.hip", r"done_kernel, grid_for\(blocks, (\d+)\)", 8192, "done_s4_grid_cap, done_s16_grid_cap"),
    ("tg_kernels.hip", r"tg_reset_broadcast_i8[\s\S]*?broadcast_kernel, grid_for\(blocks, (\d+)\)", 8192,
     "reset_broadcast_s4_grid_cap"),
    ("tg_aux.hip", r"hash_kernel, dim3\(grid_for\(blocks, (\d+)\)\)", 8192, "hash_s4_grid_cap"),
    ("tg_aux.hip", r"const dim3 grid\(grid_for\(\(n \+ tg::kBlock - 1\) / tg::kBlock, (\d+)\)\)", 8192, "seen_grid_cap"),
    ("tg_aux.hip", r"grid_for\(S == 4 \? \(B \+ 3\) / 4 : B, 1 << (\d+)\)", 20, "rank_s4_grid_cap, rank_s5_grid_cap"),
    ("tg_gen.hip", r"gen_tokens_kernel<ST, M>\), dim3\(grid_for\(wgs > (\d+) \?", 16384, "gen_s4_tokens_grid_cap"),
    ("tg_gen.hip", r"if \(nvec >= \(int64_t\)tg::kBlock \* 16 \* (\d+)\) rc = tokens\(launch_tokens<4, 16>\)", 2048,
     "gen_s4_tokens_grid_cap"),
    ("tg_gen.hip", r"const dim3 bgrid\(grid_for\(B > (\d+) \?", 16384, "gen_s4_basis_grid_cap"),
    ("tg_gen.hip", r"const dim3 mgrid\(grid_for\(B > (\d+) \?", 65536, "gen_s9_basis_grid_cap"),
    ("tg_gen.hip", r"const dim3 mgrid\(grid_for\(B > (\d+)LL \* cus \?", 4, "change_basis_s16_rounds"),
    ("tg_device.h", r"constexpr int kBlock = (\d+);", 256, "every grid-cap entry (games per workgroup)"),
]


@pytest.mark.parametrize("fname, pattern, want, entries", PINS, ids=[f"{p[0]}:{p[3].split(',')[0]}" for p in PINS])
def test_threshold_still_has_the_value_the_size_table_assumes(fname, pattern, want, entries):
    m = re.search(pattern, source(fname))
    assert m, f"{fname}: the threshold behind SIZES[{entries}] is no longer written as /{pattern}/ -- find it and update " \
              f"the table in tests/test_gpu_full_size_oracle.py and this pin"
    got = int(m.group(1))
    assert got == want, f"{fname}: the threshold is now {got}, SIZES assumes {want} -- move SIZES[{entries}] in " \
                        f"tests/test_gpu_full_size_oracle.py (and this pin)"


def test_env_crossover_is_the_table_entry():
    from mat_mul_amd.env import TensorGameEnv

    assert TensorGameEnv.TRACKED_FROM == {16: 12000, 25: 2048}, "move SIZES['tracked_s16_crossover'] / ['tracked_s25_sparse']"
