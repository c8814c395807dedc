"""CPU checks of training at the 5x5 matmul tensor (S = 25, include/tensor_game_train_s25.h): the three entries and the
family they accept, the refusal of every other size and of S = 25 by the two other training headers, the LDS plans the
library prints against their restatement (net_s25_train_family) over a sweep, the workspace formula, argument
validation before any launch, that each row reaches the case of the two chunk loops it is there for, and the float64
restatement against the reference's own recorded losses and gradients (tests/golden/train_s25_cases.npz).  No GPU
needed."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from mat_mul_amd import SlicedTrainer25, _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import CONFIGS as CONFIGS_S4
from net_ref import make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from net_s16_ref import CONFIGS as CONFIGS_S16
from net_s25_ref import CONFIGS, RECORDED
from net_s25_train_family import (LDS, REFUSED, ROWS, chunks, decoder_bytes, decoder_runs, dims, plan_bytes, torso_runs,
                                   workspace_bytes)
from test_net_s25_cpu import sweep
from train_ref import TrainRef, make_batch

_NEEDS = re.compile(r"the S = 25 training LDS plan needs (\d+) \(torso\) / (\d+) \(decoder, self-attention\) / (\d+) "
                    r"\(decoder, cross-attention\) bytes > 160 KiB")
ENTRIES = ("tg_net_train_s25_check", "tg_net_train_s25_workspace_size", "tg_net_loss_grad_s25")


def cfg25(m):
    return net.check_config(dims(m), ops.net_s25_check)


def test_the_three_symbols_exist_with_the_whole_game_signatures():
    assert sorted(_lib.TRAIN_S25_SIGNATURES) == sorted(ENTRIES)
    for s25, whole in zip(ENTRIES, ("tg_net_train_check", "tg_net_train_workspace_size", "tg_net_loss_grad")):
        assert getattr(_lib.lib, s25).argtypes == _lib.TRAIN_SIGNATURES[whole]
    assert not set(ENTRIES) & (set(_lib.TRAIN_SLICED_SIGNATURES) | set(_lib.NET_S25_SIGNATURES))


@pytest.mark.parametrize("name", sorted(ROWS))
def test_the_rows_are_inside_the_s25_training_family(name):
    m = dims(ROWS[name])
    ops.net_train_s25_check(cfg25(m))
    assert max(plan_bytes(m)) <= LDS and decoder_bytes(m) <= LDS
    assert {"a25", "b25", "c25"} <= set(ROWS)


def test_the_plans_the_header_states():
    kib = lambda b: round(b / 1024, 1)  # noqa: E731
    for name, torso, launch2 in (("a25", 103.1, 150.6), ("b25", 95.8, 154.1)):
        m = dims(ROWS[name])
        assert kib(plan_bytes(m)[0]) == torso and kib(decoder_bytes(m)) == launch2
        assert chunks(m) == ((19, 4, 18), (2, 38, 1))


def test_a_dim_c_whose_resident_keys_cannot_fit_is_refused():
    m = dims(REFUSED["wide25"])
    with pytest.raises(TensorGameError) as e:
        ops.net_train_s25_check(cfg25(m))
    got = _NEEDS.search(str(e.value))
    assert got and e.value.code == -2, str(e.value)
    assert tuple(int(x) for x in got.groups()) == plan_bytes(m)
    assert plan_bytes(m)[2] > LDS >= max(plan_bytes(m)[:2])
    ops.net_train_s25_check(cfg25(dict(m, c=8)))  # dim_c alone decides: the resident ln2(ee) is 3 * 625 * c floats


@pytest.mark.parametrize("cfg", [CONFIGS_S4["a"], CONFIGS_S9["a9"], CONFIGS_S16["a16"]], ids=["S4", "S9", "S16"])
def test_other_sizes_are_refused_with_a_pointer_to_the_other_entries(cfg):
    c = net.check_config(dims(cfg))
    for call in (lambda: ops.net_train_s25_check(c), lambda: ops.net_train_s25_workspace_size(c, 4)):
        with pytest.raises(TensorGameError, match="tg_net_loss_grad .*tg_net_loss_grad_sliced") as e:
            call()
        assert e.value.code == -2


def test_the_other_training_headers_still_refuse_s25():
    for name in ("a25", "b25", "c25"):
        c = cfg25(CONFIGS[name])
        for call in (ops.net_train_check, ops.net_train_sliced_check):
            with pytest.raises(TensorGameError, match="TG_NET_MAX_S") as e:
                call(c)
            assert e.value.code == -2


def test_plan_restatement_matches_the_library_over_a_sweep():
    accepted = refused = 0
    for m in sweep(600, 7525):
        c = _lib.NetConfig(**m)
        try:
            ops.net_s25_check(c)
        except TensorGameError as e:  # outside inference's family: the same refusal, not counted
            with pytest.raises(TensorGameError) as e2:
                ops.net_train_s25_check(c)
            assert str(e2.value).split(": ", 1)[1] == str(e).split(": ", 1)[1] and not _NEEDS.search(str(e2.value))
            continue
        want = plan_bytes(m)
        try:
            ops.net_train_s25_check(c)
        except TensorGameError as e:
            got = _NEEDS.search(str(e))
            assert got and e.code == -2, str(e)
            assert tuple(int(x) for x in got.groups()) == want, (m, str(e), want)
            assert max(want) > LDS
            refused += 1
            continue
        assert max(want) <= LDS and decoder_bytes(m) <= LDS, (m, want)
        accepted += 1
    print(f"accepted {accepted}, refused {refused}")
    assert accepted >= 20 and refused >= 20, (accepted, refused)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_workspace_size_is_the_headers_formula(name):
    m = dims(ROWS[name])
    c = cfg25(m)
    for B in (1, 16, 257):
        assert ops.net_train_s25_workspace_size(c, B) == workspace_bytes(m, B)
    for B in (0, (1 << 24) + 1):
        with pytest.raises(TensorGameError) as e:
            ops.net_train_s25_workspace_size(c, B)
        assert e.value.code == -1


def test_the_slabs_at_the_apps_configuration_are_175_mb():
    c = cfg25(ROWS["a25"])
    assert ops.net_s25_weights_size(c) == 171249
    assert 256 * 171249 * 4 < ops.net_train_s25_workspace_size(c, 16) < 256 * 171249 * 4 + (20 << 20)
    assert round(ops.net_train_s25_workspace_size(c, 16) / 1e6) == 194
    assert round(ops.net_train_s25_workspace_size(c, 256) / 1e6) == 477


def test_abi_argument_validation_without_gpu():
    lib = _lib.lib
    cfg = cfg25(ROWS["a25"])
    small = net.check_config(dims(CONFIGS_S9["a9"]))
    need = ops.net_train_s25_workspace_size(cfg, 4)
    p, ws = C.c_void_p(64), C.c_void_p(256)  # never dereferenced: every call below is refused before any launch

    def call(cfg=cfg, theta=p, pos_fix=p, frames=p, i8=1, scalars=p, g_action=p, g_value=p, B=4, wp=1.0, wv=1000.0, dp=0.5,
             ws=ws, ws_bytes=need, grad=p, losses=p, status=p):
        return lib.tg_net_loss_grad_s25(C.byref(cfg) if cfg is not None else None, theta, pos_fix, frames, i8, scalars,
                                        g_action, g_value, B, wp, wv, dp, 0, 0, None, None, ws, ws_bytes, grad, losses,
                                        status, None)

    assert lib.tg_net_train_s25_check(C.byref(cfg)) == 0
    assert lib.tg_net_train_s25_check(None) == -1
    assert lib.tg_net_train_s25_check(C.byref(small)) == -2 and b"tg_net_loss_grad" in lib.tg_last_error()
    assert lib.tg_net_train_s25_workspace_size(C.byref(cfg), 4, None) == -1
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


def test_both_chunk_loops_are_reached_with_one_chunk_full_chunks_and_partial_last_chunks():
    table = {name: chunks(dims(cfg)) for name, cfg in ROWS.items()}
    assert table["a25"] == table["b25"] == ((19, 4, 18), (2, 38, 1))
    assert table["c25"] == ((38, 2, 37), (6, 13, 3))
    assert table["one25"] == ((1, 1, 1), (1, 1, 1)) and table["odd25"] == ((5, 1, 5), (5, 1, 5))  # one chunk in both
    (s_nq, s_count, s_last), (x_nq, x_count, x_last) = table["xtail25"]
    assert s_count == 1 and x_count > 1 and 0 < x_last < x_nq, table["xtail25"]  # a partial last chunk, cross-attention
    (s_nq, s_count, s_last), _ = table["stail25"]
    assert s_count > 1 and 0 < s_last < s_nq, table["stail25"]                   # a partial last chunk, self-attention
    for name, blocks in table.items():
        for nq, count, last in blocks:
            assert (count - 1) * nq + last == dims(ROWS[name])["n_steps"] and 1 <= last <= nq


def test_the_gpu_shapes_reach_the_runs_they_are_there_for():
    assert len(torso_runs(1)) == 25 and len(decoder_runs(1)) == 1
    straddles = lambda B: [r for r in torso_runs(B) if r[1] > r[0] and r[0] // 25 != (r[1] - 1) // 25]  # noqa: E731
    assert sorted({u1 - u0 for u0, u1 in torso_runs(11)}) == [1, 2] and len(torso_runs(11)) == 256
    assert len(straddles(15)) == 4 and not straddles(11)
    assert sorted(g1 - g0 for g0, g1 in decoder_runs(257)) == [1] * 255 + [2]
    assert (263 * 25) % 256 != 0 and sorted(g1 - g0 for g0, g1 in decoder_runs(263)) == [1] * 249 + [2] * 7


def test_the_python_entries_share_one_body():
    for fn in (ops.net_loss_grad, ops.net_loss_grad_sliced, ops.net_loss_grad_s25):
        assert fn.__code__.co_names.count("_loss_grad") == 1
    for fn in (ops.net_train_workspace_size, ops.net_train_sliced_workspace_size, ops.net_train_s25_workspace_size):
        assert fn.__code__.co_names.count("_workspace_size") == 1


def test_sliced_trainer_25_needs_a_rocm_device_and_is_exported():
    import mat_mul_amd
    from mat_mul_amd.train import FusedTrainer

    assert issubclass(SlicedTrainer25, FusedTrainer) and "SlicedTrainer25" in mat_mul_amd.__all__
    assert SlicedTrainer25._net is mat_mul_amd.FusedAlphaTensor25 and FusedTrainer._net is mat_mul_amd.FusedAlphaTensor
    with pytest.raises(TensorGameError, match="a ROCm device is required"):
        SlicedTrainer25.from_state_dict(make_weights(ROWS["c25"], 1), device="cpu")


def _signs(seed, index, shape):  # make_golden_train.signs
    rng = np.random.default_rng([seed, index])
    return rng.integers(0, 2, size=(2,) + tuple(shape)).astype(np.float64) * 2.0 - 1.0


@pytest.fixture(scope="module")
def train_cases(golden):
    return golden("train_s25_cases")


@pytest.mark.parametrize("name", RECORDED)
def test_train_restatement_reproduces_the_reference_loss_and_gradient_at_s25(train_cases, name):
    cfg = CONFIGS[name]
    seed = int(train_cases[f"{name}_seed"].item())
    keys = [k.decode() for k in train_cases[f"{name}_keys"]]
    ref = TrainRef(make_weights(cfg, seed), cfg)
    l_pol, l_val, grads = ref.loss_grad(*make_batch(cfg, 2, seed + 300))
    assert abs(l_pol - train_cases[f"{name}_l_pol"].item()) <= 1e-9 * abs(l_pol)
    assert abs(l_val - train_cases[f"{name}_l_val"].item()) <= 1e-9 * abs(l_val)
    norm, dot = train_cases[f"{name}_gnorm"], train_cases[f"{name}_gdot"]
    for i, k in enumerate(keys):
        v = grads.get(k)
        if v is None:
            assert norm[i] == 0.0, k
            continue
        s, scale = _signs(seed, i, v.shape), max(1.0, norm[i])
        assert abs(np.sqrt((v * v).sum()) - norm[i]) <= 1e-9 * scale, k
        assert abs((s[0] * v).sum() - dot[i, 0]) <= 1e-9 * scale * np.sqrt(v.size), k
        assert abs((s[1] * v).sum() - dot[i, 1]) <= 1e-9 * scale * np.sqrt(v.size), k
    full = [k[len(name) + 3:] for k in train_cases.files if k.startswith(f"{name}_g_")]
    assert len(full) >= 6
    for k in full:
        np.testing.assert_allclose(grads[k], train_cases[f"{name}_g_{k}"], rtol=0, atol=1e-9, err_msg=k)
    assert torch.isfinite(torch.tensor(train_cases[f"{name}_adam_loss"])).all()
