"""CPU checks of training at the 4x4 matmul tensor (S = 16, include/tensor_game_train_sliced.h): the three entries and
the family they accept, the refusal of every other size, the LDS plans the library prints against their restatement
(net_s16_train_family) over a sweep, the workspace formula, argument validation before any launch, and that the one
plan-derived loop (the cross-attention's chunks of decoder positions) is reached with a partial last chunk.  No GPU
needed."""
import ctypes as C
import re

import pytest

from mat_mul_amd import SlicedTrainer, _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import CONFIGS as CONFIGS_S4
from net_ref import make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from net_s16_train_family import LDS, ROWS, chunks, dims, sliced_bytes, workspace_bytes
from test_net_s16_cpu import sweep

_NEEDS = re.compile(r"the sliced training LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes > 160 KiB")
ENTRIES = ("tg_net_train_sliced_check", "tg_net_train_sliced_workspace_size", "tg_net_loss_grad_sliced")


def test_the_three_symbols_exist_with_the_whole_game_signatures():
    assert sorted(_lib.TRAIN_SLICED_SIGNATURES) == sorted(ENTRIES)
    for sliced, whole in zip(ENTRIES, ("tg_net_train_check", "tg_net_train_workspace_size", "tg_net_loss_grad")):
        assert getattr(_lib.lib, sliced).argtypes == _lib.TRAIN_SIGNATURES[whole]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_the_rows_are_inside_the_sliced_family(name):
    m = dims(ROWS[name])
    ops.net_train_sliced_check(net.check_config(m))
    assert max(sliced_bytes(m)) <= LDS
    assert {"a16", "b16", "ones16", "odd16", "c13", "t8"} <= set(ROWS)


@pytest.mark.parametrize("cfg", [CONFIGS_S4["a"], CONFIGS_S9["a9"]], ids=["S4", "S9"])
def test_other_sizes_are_refused_with_a_pointer_to_the_whole_game_entry(cfg):
    c = net.check_config(dims(cfg))
    ops.net_train_check(c)  # the whole-game entries take them
    for call in (lambda: ops.net_train_sliced_check(c), lambda: ops.net_train_sliced_workspace_size(c, 4)):
        with pytest.raises(TensorGameError, match="tg_net_loss_grad") as e:
            call()
        assert e.value.code == -2


def test_plan_restatement_matches_the_library_over_a_sweep():
    accepted = refused = 0
    for m in sweep(400, 1616):
        c = _lib.NetConfig(**m)
        try:
            ops.net_check(c)
        except TensorGameError as e:  # outside inference's family: the same refusal, not counted
            with pytest.raises(TensorGameError) as e2:
                ops.net_train_sliced_check(c)
            assert str(e2.value).split(": ", 1)[1] == str(e).split(": ", 1)[1] and not _NEEDS.search(str(e2.value))
            continue
        want = sliced_bytes(m)
        try:
            ops.net_train_sliced_check(c)
        except TensorGameError as e:
            got = _NEEDS.search(str(e))
            assert got and e.code == -2, str(e)
            assert (int(got.group(1)), int(got.group(2))) == want, (m, str(e), want)
            assert max(want) > LDS
            refused += 1
            continue
        assert max(want) <= LDS, (m, want)
        accepted += 1
    assert accepted >= 50 and refused >= 50, (accepted, refused)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_workspace_size_is_the_headers_formula(name):
    m = dims(ROWS[name])
    c = net.check_config(m)
    for B in (1, 16, 257):
        assert ops.net_train_sliced_workspace_size(c, B) == workspace_bytes(m, B)
    for B in (0, (1 << 24) + 1):
        with pytest.raises(TensorGameError) as e:
            ops.net_train_sliced_workspace_size(c, B)
        assert e.value.code == -1


def test_the_slabs_at_the_apps_configuration_are_172_mb():
    m = dims(ROWS["a16"])
    c = net.check_config(m)
    assert ops.net_weights_size(c) == 167739
    assert 256 * 167739 * 4 < ops.net_train_sliced_workspace_size(c, 16) < 256 * 167739 * 4 + (8 << 20)


def test_abi_argument_validation_without_gpu():
    lib = _lib.lib
    cfg = net.check_config(dims(ROWS["a16"]))
    small = net.check_config(dims(CONFIGS_S9["a9"]))
    need = ops.net_train_sliced_workspace_size(cfg, 4)
    p, ws = C.c_void_p(64), C.c_void_p(256)  # never dereferenced: every call below is refused before any launch

    def call(cfg=cfg, theta=p, pos_fix=p, frames=p, i8=1, scalars=p, g_action=p, g_value=p, B=4, wp=1.0, wv=1000.0, dp=0.5,
             ws=ws, ws_bytes=need, grad=p, losses=p, status=p):
        return lib.tg_net_loss_grad_sliced(C.byref(cfg) if cfg is not None else None, theta, pos_fix, frames, i8, scalars,
                                           g_action, g_value, B, wp, wv, dp, 0, 0, None, None, ws, ws_bytes, grad, losses,
                                           status, None)

    assert lib.tg_net_train_sliced_check(C.byref(cfg)) == 0
    assert lib.tg_net_train_sliced_check(None) == -1
    assert lib.tg_net_train_sliced_check(C.byref(small)) == -2 and b"tg_net_loss_grad" in lib.tg_last_error()
    assert lib.tg_net_train_sliced_workspace_size(C.byref(cfg), 4, None) == -1
    assert call(cfg=None) == -1
    assert call(cfg=small) == -2
    for name in ("theta", "pos_fix", "frames", "scalars", "g_action", "g_value", "ws", "losses", "status"):
        assert call(**{name: None}) == -1, name
        assert b"null" in lib.tg_last_error()
    assert call(i8=2) == -1 and b"frames_is_i8=2" in lib.tg_last_error()
    assert call(dp=1.0) == -1 and b"dropout_p=1" in lib.tg_last_error()
    assert call(dp=-0.1) == -1
    assert call(wp=float("nan")) == -1 and b"not finite" in lib.tg_last_error()
    assert call(wv=float("inf")) == -1
    assert call(B=0) == -1 and call(B=(1 << 24) + 1) == -1
    assert call(ws=C.c_void_p(384)) == -1 and b"aligned" in lib.tg_last_error()  # 128-byte aligned only
    assert call(theta=C.c_void_p(66)) == -1 and call(grad=C.c_void_p(66)) == -1
    assert call(i8=0, frames=C.c_void_p(65)) == -1  # float32 frames on an odd address
    assert call(ws_bytes=need - 1) == -1 and b"needed" in lib.tg_last_error()


def test_the_chunk_loop_is_reached_with_full_and_partial_last_chunks():
    table = {name: chunks(dims(cfg)) for name, cfg in ROWS.items()}
    assert table["a16"] == (8, 6, 8) and table["b16"] == (8, 6, 8)   # six full chunks
    assert table["odd16"] == (7, 1, 7) and table["c13"] == (5, 1, 5) and table["ones16"] == (1, 1, 1)  # one chunk
    nq, count, last = table["tail16"]
    assert count > 1 and 0 < last < nq, table["tail16"]              # a partial last chunk
    for name, (nq, count, last) in table.items():
        assert (count - 1) * nq + last == dims(ROWS[name])["n_steps"] and 1 <= last <= nq


def test_the_python_entries_share_one_body():
    assert ops.net_loss_grad.__code__.co_names.count("_loss_grad") == 1
    assert ops.net_loss_grad_sliced.__code__.co_names.count("_loss_grad") == 1


def test_sliced_trainer_needs_a_rocm_device_and_is_exported():
    import mat_mul_amd
    from mat_mul_amd.train import FusedTrainer

    assert issubclass(SlicedTrainer, FusedTrainer) and "SlicedTrainer" in mat_mul_amd.__all__
    with pytest.raises(TensorGameError, match="a ROCm device is required"):
        SlicedTrainer.from_state_dict(make_weights(ROWS["b16"], 1), device="cpu")
