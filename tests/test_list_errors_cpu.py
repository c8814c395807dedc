"""Every refusal of the entries that take action lists (tokens int8 (M,K,3S) + lengths int64 (M) + shift), characterised
without a device: the wrappers of mat_mul_amd/ops.py and the C entries behind them.

``PY_CASES`` is a table in the manner of tests/test_ops_errors_cpu.py (whose ``Cuda`` stand-ins it uses): named calls of
``solution_canon``, ``orbit_canon``, ``flip_begin``, ``solution_rebase`` and ``replay_add_lists`` (and of ``flip_advance``
and ``flip_advance_plus``, which read the sizes off ``cur`` the same way), each with one bad argument per check and a
few with two, to pin the order of the checks.  ``C_CASES`` calls ``tg_solution_canon``,
``tg_orbit_canon``, ``tg_orbit_workspace_size``, ``tg_solution_rebase``, ``tg_flip_begin``, ``tg_flip_advance``,
``tg_flip_advance_plus`` and the ``*_check`` entries through ctypes with pointers that are never dereferenced: every case
is refused (or returns at once because there is no work) before anything is launched.

``tests/golden/list_errors.json`` holds what the PARENT of the commit that gave these entries one copy of their shared
checks answered: for a wrapper the exception type, ``code`` and the full message, for a C entry the return code and the
text of ``tg_last_error()``.  It is recorded by

    git show <parent>:mat_mul_amd/ops.py > parent_ops.py            (and the parent's library built into PARENT_LIB)
    python tests/test_list_errors_cpu.py --record --ops parent_ops.py --lib PARENT_LIB

and never from the refactored code.  The tests compare today's ops.py and library with it.
"""
import ctypes as C
import importlib.util
import json
import sys
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = Path(__file__).resolve().parent / "golden" / "list_errors.json"
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from mat_mul_amd import _lib, ops  # noqa: E402

from test_ops_errors_cpu import DEV, OTHER, games, observe, same, t, view  # noqa: E402

i8, u8, i32, u32, i64, f32 = torch.int8, torch.uint8, torch.int32, torch.uint32, torch.int64, torch.float32

PY_CASES = {}


def cases(fn, base, **named):
    for name, bad in named.items():
        assert f"{fn}.{name}" not in PY_CASES, name
        PY_CASES[f"{fn}.{name}"] = (fn, base, bad)


def cpu(shape, dtype=i8):
    return torch.zeros(shape, dtype=dtype)


# ---- the wrappers: M = 3 lists of K = 5 terms at S = 4 -------------------------------------------------------------------
TOK, LEN = t((3, 5, 12)), t((3,), i64)
TOKENS_BAD = dict(
    tokens_cpu=dict(tokens=cpu((3, 5, 12))),
    tokens_dtype=dict(tokens=t((3, 5, 12), u8)),
    tokens_dim=dict(tokens=t((15, 12))),
    tokens_width=dict(tokens=t((3, 5, 13))))
LENGTHS_BAD = dict(
    lengths_cpu=dict(lengths=cpu((3,), i64)),
    lengths_dtype=dict(lengths=t((3,), i32)),
    lengths_shape=dict(lengths=t((4,), i64)),
    lengths_device=dict(lengths=t((3,), i64, OTHER)),
    lengths_strided=dict(lengths=view(lambda z: z[::2], (6,), i64)))
CANON_OUT = dict(canon=t((3, 5, 12)), rank=t((3,), i32), key=t((3,), i64), residual_nnz=t((3,), i32), status=t((1,), u32))
CANON_BAD = dict(
    TOKENS_BAD, **LENGTHS_BAD,
    size_S=dict(tokens=t((3, 5, 99))),
    size_K=dict(tokens=t((3, 257, 12))),
    size_shift=dict(shift=65),
    targets_cpu=dict(targets=cpu((3, 4, 4, 4))),
    targets_dtype=dict(targets=t((3, 4, 4, 4), u8)),
    targets_shape=dict(targets=games(2)),
    targets_size=dict(targets=games(3, 5)),
    targets_device=dict(targets=games(3, device=OTHER)),
    residual_without_targets=dict(targets=None),
    lengths_none=dict(lengths=None),
    canon_dtype=dict(canon=t((3, 5, 12), u8)),
    canon_shape=dict(canon=t((3, 4, 12))),
    canon_strided=dict(canon=view(lambda z: z[:, :5], (3, 6, 12))),
    rank_dtype=dict(rank=t((3,), i64)),
    rank_shape=dict(rank=t((2,), i32)),
    key_dtype=dict(key=t((3,), i32)),
    key_device=dict(key=t((3,), i64, OTHER)),
    residual_dtype=dict(residual_nnz=t((3,), i64)),
    residual_shape=dict(residual_nnz=t((3, 1), i32)),
    status_dtype=dict(status=t((1,), i32)),
    status_shape=dict(status=t((2,), u32)),
    tokens_then_size=dict(tokens=t((3, 5, 12), u8), shift=65),
    size_then_targets=dict(shift=65, targets=games(2)),
    targets_then_lengths=dict(targets=games(2), lengths=t((4,), i64)),
    no_targets_then_lengths=dict(targets=None, lengths=t((4,), i64)),
    lengths_then_canon=dict(lengths=t((4,), i64), canon=t((3, 4, 12))),
    canon_then_rank=dict(canon=t((3, 4, 12)), rank=t((2,), i32)),
    rank_then_key=dict(rank=t((2,), i32), key=t((3,), i32)),
    key_then_residual=dict(key=t((3,), i32), residual_nnz=t((3, 1), i32)),
    residual_then_status=dict(residual_nnz=t((3, 1), i32), status=t((2,), u32)))
cases("solution_canon", dict(CANON_OUT, targets=games(3), tokens=TOK, lengths=LEN), **CANON_BAD)
cases("orbit_canon", dict(CANON_OUT, targets=games(3), tokens=TOK, lengths=LEN, sym=t((6, 13), u8), which=t((3,), i32),
                          stab=t((3,), i32), workspace=False), **CANON_BAD,
      sym_cpu=dict(sym=cpu((6, 13), u8)),
      sym_dtype=dict(sym=t((6, 13), i8)),
      sym_dim=dict(sym=t((78,), u8)),
      sym_width=dict(sym=t((6, 12), u8)),
      sym_empty=dict(sym=t((0, 13), u8)),
      sym_device=dict(sym=t((6, 13), u8, OTHER)),
      sym_strided=dict(sym=view(lambda z: z[::2], (12, 13), u8)),
      size_G=dict(sym=t((_lib.TG_ORBIT_MAX_G + 1, 13), u8)),
      size_S_of_both=dict(tokens=t((3, 5, 99)), sym=t((6, 100), u8)),
      which_dtype=dict(which=t((3,), i64)),
      which_shape=dict(which=t((2,), i32)),
      stab_dtype=dict(stab=t((3,), u32)),
      stab_device=dict(stab=t((3,), i32, OTHER)),
      tokens_then_sym=dict(tokens=t((15, 12)), sym=t((6, 12), u8)),
      sym_then_size=dict(sym=t((6, 12), u8), shift=65),
      residual_then_which=dict(residual_nnz=t((3, 1), i32), which=t((2,), i32)),
      which_then_stab=dict(which=t((2,), i32), stab=t((3,), u32)),
      stab_then_status=dict(stab=t((3,), u32), status=t((2,), u32)))
WALK = dict(cur=t((4, 5, 12)), cur_rank=t((4,), i32), best=t((4, 5, 12)), best_rank=t((4,), i32), best_step=t((4,), i64),
            flips=t((4,), i64), state=t((4,), i32))
cases("flip_begin", dict(WALK, tokens=TOK, lengths=LEN, src=t((4,), i64), status=t((1,), u32)), **TOKENS_BAD, **LENGTHS_BAD,
      lengths_none=dict(lengths=None),
      src_cpu=dict(src=cpu((4,), i64)),
      src_dim=dict(src=t((4, 1), i64)),
      src_dtype=dict(src=t((4,), i32)),
      src_device=dict(src=t((4,), i64, OTHER)),
      size_S=dict(tokens=t((3, 5, 99))),
      size_K=dict(tokens=t((3, _lib.TG_FLIP_MAX_K + 1, 12))),
      size_shift=dict(shift=65),
      size_bound=dict(bound=64),
      no_src_other_count=dict(src=None),
      cur_cpu=dict(cur=cpu((4, 5, 12))),
      cur_shape=dict(cur=t((3, 5, 12))),
      cur_rank_dtype=dict(cur_rank=t((4,), i64)),
      best_dtype=dict(best=t((4, 5, 12), u8)),
      best_rank_shape=dict(best_rank=t((4, 1), i32)),
      best_step_dtype=dict(best_step=t((4,), i32)),
      flips_device=dict(flips=t((4,), i64, OTHER)),
      state_dtype=dict(state=t((4,), u8)),
      status_dtype=dict(status=t((1,), i32)),
      tokens_then_lengths=dict(tokens=t((15, 12)), lengths=t((4,), i64)),
      lengths_then_src=dict(lengths=t((4,), i64), src=t((4, 1), i64)),
      src_then_size=dict(src=t((4,), i32), bound=64),
      size_then_cur=dict(bound=64, cur=t((3, 5, 12))),
      cur_then_best=dict(cur=t((3, 5, 12)), best=t((4, 5, 12), u8)),
      state_then_status=dict(state=t((4,), u8), status=t((1,), i32)))
WALK_PLUS = dict(WALK, since=t((4,), i32), pluses=t((4,), i64))
for entry, walk, more in (("flip_advance", WALK, {}), ("flip_advance_plus", WALK_PLUS, dict(plus_after=3))):
    cases(entry, dict(st=walk, n_steps=2, **more),
          cur_cpu=dict(st=dict(walk, cur=cpu((4, 5, 12)))),
          cur_dtype=dict(st=dict(walk, cur=t((4, 5, 12), u8))),
          cur_dim=dict(st=dict(walk, cur=t((20, 12)))),
          cur_width=dict(st=dict(walk, cur=t((4, 5, 13)))),
          size_K=dict(st=dict(walk, cur=t((4, _lib.TG_FLIP_MAX_K + 1, 12)))),
          size_steps=dict(n_steps=0),
          best_shape=dict(st=dict(walk, best=t((4, 4, 12)))),
          state_dtype=dict(st=dict(walk, state=t((4,), i64))),
          cur_then_size=dict(st=dict(walk, cur=t((20, 12))), n_steps=0),
          size_then_best=dict(n_steps=0, st=dict(walk, best=t((4, 4, 12)))))
cases("flip_advance_plus", dict(st=WALK_PLUS, n_steps=2, plus_after=3),
      size_plus_after=dict(plus_after=0),
      no_since=dict(st=WALK),
      no_pluses=dict(st=dict(WALK, since=t((4,), i32))),
      pluses_dtype=dict(st=dict(WALK_PLUS, pluses=t((4,), i32))),
      size_then_no_since=dict(plus_after=0, st=WALK))
cases("solution_rebase", dict(tokens=TOK, lengths=LEN, mats=t((2, 3, 4, 4), i32), index=t((3,), i64), tokens_out=t((3, 5, 12)),
                              lengths_out=t((3,), i64), bad=t((3,), u8), status=t((1,), u32)),
      tokens_dtype=dict(tokens=t((3, 5, 12), u8)),
      tokens_dim=dict(tokens=t((15, 12))),
      tokens_width=dict(tokens=t((3, 5, 13))),
      mats_dtype=dict(mats=t((2, 3, 4, 4), i64)),
      mats_dim=dict(mats=t((6, 4, 4), i32)),
      mats_size=dict(mats=t((2, 3, 5, 5), i32)),
      lengths_dtype=dict(lengths=t((3,), i32)),
      lengths_shape=dict(lengths=t((4,), i64)),
      no_index_other_count=dict(index=None),
      index_dtype=dict(index=t((3,), i32)),
      index_shape=dict(index=t((2,), i64)),
      tokens_cpu=dict(tokens=cpu((3, 5, 12))),
      lengths_device=dict(lengths=t((3,), i64, OTHER)),
      mats_device=dict(mats=t((2, 3, 4, 4), i32, OTHER)),
      index_device=dict(index=t((3,), i64, OTHER)),
      size_S=dict(tokens=t((3, 5, 99)), mats=t((2, 3, 33, 33), i32)),
      size_K=dict(tokens=t((3, 257, 12))),
      size_shift=dict(shift=65),
      tokens_out_shape=dict(tokens_out=t((3, 5, 13))),
      tokens_out_dtype=dict(tokens_out=t((3, 5, 12), u8)),
      in_place=dict(tokens_out=TOK),
      lengths_out_dtype=dict(lengths_out=t((3,), i32)),
      lengths_out_device=dict(lengths_out=t((3,), i64, OTHER)),
      bad_shape=dict(bad=t((2,), u8)),
      status_shape=dict(status=t((2,), u32)),
      tokens_then_mats=dict(tokens=t((15, 12)), mats=t((6, 4, 4), i32)),
      mats_then_lengths=dict(mats=t((6, 4, 4), i32), lengths=t((4,), i64)),
      lengths_then_index=dict(lengths=t((4,), i64), index=t((2,), i64)),
      index_then_tokens_cpu=dict(index=t((2,), i64), tokens=cpu((3, 5, 12))),
      device_then_size=dict(mats=t((2, 3, 4, 4), i32, OTHER), shift=65),
      size_then_tokens_out=dict(shift=65, tokens_out=t((3, 5, 13))),
      in_place_then_lengths_out=dict(tokens_out=TOK, lengths_out=t((3,), i32)),
      lengths_out_then_bad=dict(lengths_out=t((3,), i32), bad=t((2,), u8)),
      bad_then_status=dict(bad=t((2,), u8), status=t((2,), u32)))
BUF = types.SimpleNamespace(L=4, T=2, S=4, device=DEV, desc=None)
cases("replay_add_lists", dict(buf=BUF, starts=t((3, 2, 4, 4, 4)), tokens=TOK, lengths=LEN, groups=t((3,), i64),
                               stored=t((3,), u8), status=t((1,), u32)),
      starts_cpu=dict(starts=cpu((3, 2, 4, 4, 4))),
      tokens_cpu=dict(tokens=cpu((3, 5, 12))),
      lengths_cpu=dict(lengths=cpu((3,), i64)),
      starts_dim=dict(starts=t((3, 4, 4, 4))),
      starts_dtype=dict(starts=t((3, 2, 4, 4, 4), f32)),
      starts_frames=dict(starts=t((3, 1, 4, 4, 4))),
      starts_device=dict(starts=t((3, 2, 4, 4, 4), device=OTHER)),
      tokens_dim=dict(tokens=t((15, 12))),
      tokens_dtype=dict(tokens=t((3, 5, 12), u8)),
      tokens_width=dict(tokens=t((3, 5, 15))),
      tokens_device=dict(tokens=t((3, 5, 12), device=OTHER)),
      lengths_dtype=dict(lengths=t((3,), i32)),
      lengths_shape=dict(lengths=t((4,), i64)),
      lengths_device=dict(lengths=t((3,), i64, OTHER)),
      no_groups_more_lists=dict(groups=None, starts=t((2, 2, 4, 4, 4))),
      groups_cpu=dict(groups=cpu((3,), i64)),
      groups_dtype=dict(groups=t((3,), i32)),
      groups_shape=dict(groups=t((2,), i64)),
      stored_dtype=dict(stored=t((3,), i8)),
      stored_shape=dict(stored=t((4,), u8)),
      status_dtype=dict(status=t((1,), i32)),
      starts_then_tokens=dict(starts=t((3, 1, 4, 4, 4)), tokens=t((15, 12))),
      tokens_then_lengths=dict(tokens=t((3, 5, 15)), lengths=t((4,), i64)),
      lengths_then_groups=dict(lengths=t((4,), i64), groups=t((2,), i64)),
      groups_then_stored=dict(groups=t((2,), i64), stored=t((4,), u8)),
      stored_then_status=dict(stored=t((4,), u8), status=t((1,), i32)))

# ---- the C entries: M = 4 lists of K = 8 terms at S = 4; the pointers are never dereferenced -------------------------
C_CASES = {}
BIG = 2 ** 62


def c_cases(entry, order, base, **named):
    for name, bad in named.items():
        assert f"{entry}.{name}" not in C_CASES, name
        C_CASES[f"{entry}.{name}"] = (entry, order, {**base, **bad})


SIZES_BAD = dict(S_zero=dict(S=0), S_large=dict(S=33), K_zero=dict(K=0), shift_negative=dict(shift=-1), shift_large=dict(shift=65),
                 S_then_K=dict(S=33, K=0), K_then_shift=dict(K=0, shift=65))
LIST_SIZES_BAD = dict(SIZES_BAD, K_large=dict(K=257), M_negative=dict(M=-1), M_large=dict(M=BIG), shift_then_M=dict(shift=65, M=-1))
c_cases("tg_solution_check", ("M", "K", "S", "shift"), dict(M=4, K=8, S=4, shift=1), **LIST_SIZES_BAD)
c_cases("tg_orbit_check", ("M", "K", "S", "shift", "G"), dict(M=4, K=8, S=4, shift=1, G=64), **LIST_SIZES_BAD,
        G_zero=dict(G=0), G_large=dict(G=2049), shift_then_G=dict(shift=65, G=0), G_then_M=dict(G=0, M=-1))
c_cases("tg_solution_rebase_check", ("M", "K", "S", "G", "shift"), dict(M=4, K=8, S=4, G=2, shift=1), **LIST_SIZES_BAD,
        G_negative=dict(G=-1), G_large=dict(G=BIG), G_zero_with_lists=dict(G=0), M_then_G=dict(M=-1, G=-1))
FLIP_SIZES_BAD = dict(SIZES_BAD, K_large=dict(K=129), bound_zero=dict(bound=0), bound_large=dict(bound=64), W_negative=dict(W=-1),
                      W_large=dict(W=BIG), shift_then_bound=dict(shift=65, bound=0), bound_then_W=dict(bound=0, W=-1))
STEPS_BAD = dict(n_steps_zero=dict(n_steps=0), n_steps_large=dict(n_steps=65537), step0_negative=dict(step0=-1),
                 steps_beyond=dict(step0=2 ** 32 - 1, n_steps=2), W_then_n_steps=dict(W=-1, n_steps=0),
                 n_steps_then_step0=dict(n_steps=0, step0=-1))
PLUS_BAD = dict(plus_after_zero=dict(plus_after=0), plus_after_large=dict(plus_after=2 ** 31), plus_slack_negative=dict(plus_slack=-1),
                plus_slack_large=dict(plus_slack=129), step0_then_plus_after=dict(step0=-1, plus_after=0),
                plus_after_then_slack=dict(plus_after=0, plus_slack=-1))
c_cases("tg_flip_check", ("M", "W", "K", "S", "shift", "bound", "step0", "n_steps"),
        dict(M=4, W=6, K=8, S=4, shift=1, bound=1, step0=0, n_steps=1), **FLIP_SIZES_BAD, **STEPS_BAD,
        M_negative=dict(M=-1), M_large=dict(M=BIG), bound_then_M=dict(bound=0, M=-1), M_then_W=dict(M=-1, W=-1))
c_cases("tg_flip_plus_check", ("W", "K", "S", "shift", "bound", "step0", "n_steps", "plus_after", "plus_slack"),
        dict(W=6, K=8, S=4, shift=1, bound=1, step0=0, n_steps=1, plus_after=1, plus_slack=1), **FLIP_SIZES_BAD, **STEPS_BAD,
        **PLUS_BAD)
c_cases("tg_orbit_workspace_size", ("M", "K", "S", "G", "bytes"), dict(M=4, K=8, S=4, G=64, bytes=4096),
        sliced=dict(), one_launch=dict(M=1 << 20),  # (the plan for 4 lists cuts 64 elements into 8 slices on any device)
        S_large=dict(S=33), K_large=dict(K=257), G_zero=dict(G=0), M_negative=dict(M=-1), null_bytes=dict(bytes=None),
        M_then_bytes=dict(M=-1, bytes=None))

CANON_PTRS = dict(targets=1, tokens=4099, lengths=8192, canon=16387, rank=32768, key=65536, res=131072, status=262144)
CANON_PTRS_BAD = dict(
    no_lists=dict(M=0, tokens=None, lengths=None, canon=None),
    null_tokens=dict(tokens=None), null_lengths=dict(lengths=None), null_canon=dict(canon=None), null_rank=dict(rank=None),
    null_key=dict(key=None), residual_without_targets=dict(targets=None), in_place=dict(canon=4099),
    lengths_unaligned=dict(lengths=8196), key_unaligned=dict(key=65540), rank_unaligned=dict(rank=32770),
    residual_unaligned=dict(res=131073), status_unaligned=dict(status=262146),
    sizes_then_tokens=dict(shift=65, tokens=None), tokens_then_lengths=dict(tokens=None, lengths=None),
    lengths_then_canon=dict(lengths=None, canon=None), canon_then_rank=dict(canon=None, rank=None),
    rank_then_key=dict(rank=None, key=None), key_then_targets=dict(key=None, targets=None),
    targets_then_in_place=dict(targets=None, canon=4099), in_place_then_lengths=dict(canon=4099, lengths=8196),
    lengths_then_key_unaligned=dict(lengths=8196, key=65540), key_then_rank_unaligned=dict(key=65540, rank=32770),
    rank_then_residual_unaligned=dict(rank=32770, res=131073), residual_then_status_unaligned=dict(res=131073, status=262146))
c_cases("tg_solution_canon", ("targets", "tokens", "lengths", "M", "K", "S", "shift", "canon", "rank", "key", "res", "status"),
        dict(CANON_PTRS, M=4, K=8, S=4, shift=1), **LIST_SIZES_BAD, **CANON_PTRS_BAD)
c_cases("tg_orbit_canon", ("targets", "tokens", "lengths", "M", "K", "S", "shift", "sym", "G", "canon", "rank", "key", "res", "which",
                           "stab", "status", "workspace", "workspace_bytes"),
        dict(CANON_PTRS, M=4, K=8, S=4, shift=1, sym=524288, G=64, which=1048576, stab=2097152, workspace=4194304,
             workspace_bytes=4096), **LIST_SIZES_BAD, **CANON_PTRS_BAD,
        G_zero=dict(G=0), G_large=dict(G=2049), shift_then_G=dict(shift=65, G=0), G_then_M=dict(G=0, M=-1),
        null_sym=dict(sym=None), null_which=dict(which=None), null_stab=dict(stab=None),
        which_unaligned=dict(which=1048578), stab_unaligned=dict(stab=2097153),
        workspace_unaligned=dict(workspace=4194312), workspace_small=dict(workspace_bytes=4095),
        lengths_then_sym=dict(lengths=None, sym=None), sym_then_canon=dict(sym=None, canon=None),
        key_then_which=dict(key=None, which=None), which_then_stab=dict(which=None, stab=None),
        stab_then_targets=dict(stab=None, targets=None), residual_then_which_unaligned=dict(res=131073, which=1048578),
        which_then_stab_unaligned=dict(which=1048578, stab=2097153), stab_then_status_unaligned=dict(stab=2097153, status=262146),
        status_then_workspace=dict(status=262146, workspace=4194312),
        workspace_unaligned_then_small=dict(workspace=4194312, workspace_bytes=4095))
c_cases("tg_solution_rebase", ("tokens", "lengths", "mats", "index", "M", "K", "S", "G", "shift", "tokens_out", "lengths_out", "bad",
                               "status"),
        dict(tokens=4099, lengths=8192, mats=16384, index=32768, M=4, K=8, S=4, G=2, shift=1, tokens_out=65539, lengths_out=131072,
             bad=262145, status=524288), **LIST_SIZES_BAD,
        G_negative=dict(G=-1), G_zero_with_lists=dict(G=0), M_then_G=dict(M=-1, G=-1),
        no_lists=dict(M=0, G=0, tokens=None), null_tokens=dict(tokens=None), null_lengths=dict(lengths=None),
        null_mats=dict(mats=None), no_index_other_count=dict(index=None), null_tokens_out=dict(tokens_out=None),
        null_lengths_out=dict(lengths_out=None), in_place=dict(tokens_out=4099), lengths_unaligned=dict(lengths=8196),
        index_unaligned=dict(index=32772), lengths_out_unaligned=dict(lengths_out=131076), mats_unaligned=dict(mats=16386),
        status_unaligned=dict(status=524290), sizes_then_tokens=dict(shift=65, tokens=None),
        tokens_then_lengths=dict(tokens=None, lengths=None), lengths_then_mats=dict(lengths=None, mats=None),
        mats_then_index=dict(mats=None, index=None), index_then_tokens_out=dict(index=None, tokens_out=None),
        tokens_out_then_lengths_out=dict(tokens_out=None, lengths_out=None),
        lengths_out_then_in_place=dict(lengths_out=None, tokens_out=4099), in_place_then_lengths=dict(tokens_out=4099, lengths=8196),
        lengths_then_index_unaligned=dict(lengths=8196, index=32772),
        index_then_lengths_out_unaligned=dict(index=32772, lengths_out=131076),
        lengths_out_then_mats_unaligned=dict(lengths_out=131076, mats=16386),
        mats_then_status_unaligned=dict(mats=16386, status=524290))
WALK_PTRS = dict(cur=16387, cur_rank=32768, best=65539, best_rank=131072, best_step=262144, flips=524288, state=1048576)
WALK_ORDER = ("cur", "cur_rank", "best", "best_rank", "best_step", "flips", "state")
WALK_PTRS_BAD = dict(
    no_walks=dict(W=0, cur=None, best=None), null_cur=dict(cur=None), null_cur_rank=dict(cur_rank=None), null_best=dict(best=None),
    null_best_rank=dict(best_rank=None), null_best_step=dict(best_step=None), null_flips=dict(flips=None),
    null_state=dict(state=None), cur_is_best=dict(best=16387), cur_rank_unaligned=dict(cur_rank=32770),
    best_rank_unaligned=dict(best_rank=131073), state_unaligned=dict(state=1048578), best_step_unaligned=dict(best_step=262148),
    flips_unaligned=dict(flips=524292), cur_then_cur_rank=dict(cur=None, cur_rank=None), best_rank_then_best_step=dict(best_rank=None,
                                                                                                                  best_step=None),
    state_then_cur_is_best=dict(state=None, best=16387), cur_is_best_then_unaligned=dict(best=16387, cur_rank=32770),
    state_then_best_step_unaligned=dict(state=1048578, best_step=262148))
c_cases("tg_flip_begin", ("tokens", "lengths", "M", "src", "W", "K", "S", "shift", "bound", *WALK_ORDER, "status"),
        dict(WALK_PTRS, tokens=4099, lengths=8192, M=4, src=2097152, W=6, K=8, S=4, shift=1, bound=1, status=4194304),
        **FLIP_SIZES_BAD, **WALK_PTRS_BAD,
        M_negative=dict(M=-1), M_then_W=dict(M=-1, W=-1), no_src_other_count=dict(src=None), W_then_no_src=dict(W=-1, src=None),
        no_src_no_walks=dict(src=None, W=0, M=0, tokens=None), null_tokens=dict(tokens=None), null_lengths=dict(lengths=None),
        cur_is_tokens=dict(cur=4099), best_is_tokens=dict(best=4099), lengths_unaligned=dict(lengths=8196),
        src_unaligned=dict(src=2097156), status_unaligned=dict(status=4194306), no_src_then_tokens=dict(src=None, tokens=None),
        tokens_then_lengths=dict(tokens=None, lengths=None), lengths_then_cur=dict(lengths=None, cur=None),
        flips_unaligned_then_in_place=dict(flips=524292, cur=4099), in_place_then_lengths=dict(best=4099, lengths=8196),
        lengths_then_src_unaligned=dict(lengths=8196, src=2097156), src_then_status_unaligned=dict(src=2097156, status=4194306))
ADVANCE = dict(WALK_PTRS, W=6, K=8, S=4, shift=1, bound=1, seed=7, walk0=0, step0=0, n_steps=4)
c_cases("tg_flip_advance", (*WALK_ORDER, "W", "K", "S", "shift", "bound", "seed", "walk0", "step0", "n_steps"), ADVANCE,
        **FLIP_SIZES_BAD, **STEPS_BAD, **WALK_PTRS_BAD, step0_then_cur=dict(step0=-1, cur=None),
        no_walks_bad_steps=dict(W=0, n_steps=0))
c_cases("tg_flip_advance_plus", (*WALK_ORDER, "since", "pluses", "W", "K", "S", "shift", "bound", "seed", "walk0", "step0", "n_steps",
                                 "plus_after", "plus_slack"),
        dict(ADVANCE, since=2097152, pluses=4194304, plus_after=3, plus_slack=1), **FLIP_SIZES_BAD, **STEPS_BAD, **PLUS_BAD,
        **WALK_PTRS_BAD,
        null_since=dict(since=None), null_pluses=dict(pluses=None), since_unaligned=dict(since=2097154),
        pluses_unaligned=dict(pluses=4194308), plus_slack_then_cur=dict(plus_slack=-1, cur=None),
        flips_unaligned_then_since=dict(flips=524292, since=None), since_then_pluses=dict(since=None, pluses=None),
        pluses_then_since_unaligned=dict(pluses=None, since=2097154),
        since_then_pluses_unaligned=dict(since=2097154, pluses=4194308))


def observe_c(lib, entry, order, args):
    """The return code of the C entry and, when it is not TG_OK, the text of tg_last_error()."""
    fn = getattr(lib, entry)
    vals = [args[k] for k in order]
    if len(fn.argtypes) == len(vals) + 1:  # the stream
        vals.append(None)
    if entry == "tg_orbit_workspace_size" and vals[-1] is not None:
        got = C.c_int64(-1)
        rc = fn(*vals[:-1], C.byref(got))
        return dict(code=rc, message=lib.tg_last_error().decode() if rc else "", bytes=got.value)
    rc = fn(*vals)
    return dict(code=rc, message=lib.tg_last_error().decode() if rc else "")


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def test_the_tables_and_the_fixture_hold_the_same_cases(recorded):
    assert sorted(recorded["python"]) == sorted(PY_CASES)
    assert sorted(recorded["c"]) == sorted(C_CASES)


@pytest.mark.parametrize("name", list(PY_CASES))
def test_wrapper_refusal_is_the_parents(name, recorded):
    want = recorded["python"][name]
    assert want["type"] is not None, "every case of the table is a refusal"
    got = observe(ops, *PY_CASES[name])
    assert same(got, want), (got, want)


@pytest.mark.parametrize("name", list(C_CASES))
def test_c_answer_is_the_parents(name, recorded):
    want = recorded["c"][name]
    assert want["code"] in (0, -1), "refused, or nothing to do: never a launch"
    assert observe_c(_lib.lib, *C_CASES[name]) == want


def record(ops_path, lib_path):
    """Write the fixture from the parent's ops.py and the parent's library."""
    parent = C.CDLL(str(lib_path))
    for name in dir(_lib):
        if name.endswith("SIGNATURES"):
            for entry, argtypes in getattr(_lib, name).items():
                fn = getattr(parent, entry)
                fn.argtypes, fn.restype = argtypes, (C.c_char_p if entry == "tg_last_error" else C.c_int)
    _lib.lib = parent  # what _lib.call, and so the parent's ops.py, goes through
    spec = importlib.util.spec_from_file_location("mat_mul_amd._ops_recorded", ops_path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module  # (its dataclasses look their module up)
    spec.loader.exec_module(module)
    out = dict(python={n: {k: v for k, v in observe(module, *c).items() if k != "line"} for n, c in PY_CASES.items()},
               c={n: observe_c(parent, *c) for n, c in C_CASES.items()})
    FIXTURE.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    odd = {n: r for n, r in out["python"].items() if r["type"] != "TensorGameError"}
    odd.update({n: r for n, r in out["c"].items() if r["code"] != -1})
    print(f"{len(out['python'])} wrapper cases, {len(out['c'])} C cases; not a refusal by the library's own rule:")
    for n, r in odd.items():
        print("  ", n, r)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--record" and sys.argv[2] == "--ops" and sys.argv[4] == "--lib":
        sys.exit(record(sys.argv[3], sys.argv[5]))
    sys.exit("usage: test_list_errors_cpu.py --record --ops PARENT_OPS_PY --lib PARENT_LIBTENSORGAME_SO")
