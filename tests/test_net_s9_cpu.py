"""CPU checks of the network at the 3x3 matmul tensor (S = TG_NET_WIDE_S = 9, include/tensor_game_net.h and
include/tensor_game_train.h): the family's new member and its bounds, the training workspace, and the float64
restatements against the reference's own recorded S = 9 outputs (tests/golden/net_s9_cases.npz, train_s9_cases.npz).
No GPU needed."""
import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import Ref, dims, make_weights
from net_s9_ref import CONFIGS
from train_ref import TrainRef, make_batch

CASES = sorted(CONFIGS)


@pytest.mark.parametrize("name", CASES)
def test_inference_and_training_families_hold_s9(name):
    c = net.check_config(dims(CONFIGS[name]))
    ops.net_train_check(c)
    assert ops.net_weights_size(c) == sum(v.size for k, v in make_weights(CONFIGS[name], 0).items()
                                          if not k.endswith("pos_enc_fix"))


def test_the_constants_mirror_the_header():
    assert (_lib.TG_NET_WIDE_S, _lib.TG_NET_WIDE_MAX_STEPS) == (9, 27)
    assert _lib.NET_LIMITS["S"] == 5 and _lib.NET_LIMITS["n_steps"] == 16


@pytest.mark.parametrize("S", [6, 7, 8, 10])
def test_other_state_sizes_above_the_bound_are_refused(S):
    cfg = dict(dims(CONFIGS["a9"]), S=S)
    for check in (net.check_config, lambda m: ops.net_train_check(_lib.NetConfig(**m))):
        with pytest.raises(TensorGameError, match="TG_NET_MAX_S") as e:
            check(cfg)
        assert e.value.code == -2


def test_s9_has_its_own_steps_bound():
    cfg = dict(dims(CONFIGS["a9"]), n_steps=28)
    with pytest.raises(TensorGameError, match="TG_NET_WIDE_MAX_STEPS"):
        net.check_config(cfg)
    net.check_config(dict(cfg, n_steps=17))  # above TG_NET_MAX_STEPS, inside the S = 9 bound
    with pytest.raises(TensorGameError, match="TG_NET_MAX_STEPS"):  # the S <= 5 bound is unchanged
        net.check_config(dict(cfg, S=4, n_steps=17))


def test_every_other_bound_still_applies_at_s9():
    with pytest.raises(TensorGameError, match="TG_NET_MAX_W"):
        net.check_config(dict(dims(CONFIGS["a9"]), W=128))
    with pytest.raises(TensorGameError, match="TG_NET_MAX_T"):
        net.check_config(dict(dims(CONFIGS["a9"]), T=9))


def test_an_s9_configuration_whose_plan_cannot_fit_is_refused():
    cfg = dict(dims(CONFIGS["a9"]), c=32, W=64, blocks=4)
    with pytest.raises(TensorGameError, match="LDS plan"):
        net.check_config(cfg)
    # inside the inference family, outside the training one: a wide torso MLP and decoder
    wide = dict(dims(CONFIGS["a9"]), c=16, torso_ff=128, W=64, ff=256, heads=8, d=64)
    c = _lib.NetConfig(**wide)
    try:
        ops.net_check(c)
    except TensorGameError:
        pytest.skip("outside the inference family too")
    with pytest.raises(TensorGameError, match="training LDS plan"):
        ops.net_train_check(c)


@pytest.mark.parametrize("name", CASES)
def test_training_workspace_follows_the_per_game_formula(name):
    m = dims(CONFIGS[name])
    c = net.check_config(m)
    n = ops.net_weights_size(c)
    for B in (1, 256, 4096):
        ws = ops.net_train_workspace_size(c, B)
        assert ws >= 4 * min(B, _lib.TG_NET_TRAIN_PARTIALS) * n and ws % 256 == 0
    per_game = 4 * (2 * 3 * m["S"] ** 2 * m["c"] + m["torso_layers"] * 3 * 2 * m["S"] ** 2 * m["c"] + 3)
    grow = ops.net_train_workspace_size(c, 8192) - ops.net_train_workspace_size(c, 4096)
    assert 4096 * per_game <= grow <= 4096 * per_game + 5 * 256


@pytest.fixture(scope="module")
def net_cases(golden):
    return golden("net_s9_cases")


@pytest.fixture(scope="module")
def train_cases(golden):
    return golden("train_s9_cases")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_float64_reference_at_s9(net_cases, name):
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, int(net_cases[f"{name}_seed"].item())), cfg)
    n_out, n_ee = net_cases[f"{name}_oo64"].shape[0], net_cases[f"{name}_ee64"].shape[0]
    assert net_cases[f"{name}_xx"].shape == (16, cfg["dim_t"], 9, 9, 9)
    ee = ref.torso(net_cases[f"{name}_xx"][:n_out], net_cases[f"{name}_ss"][:n_out])
    np.testing.assert_allclose(ee[:n_ee].numpy(), net_cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, net_cases[f"{name}_g_action"][:n_out])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), net_cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)
    # the reference's own float32 run is inside the GPU tests' bound, with a margin
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64 = net_cases[f"{name}_{key}64"]
        err = np.abs(net_cases[f"{name}_{key}32"].astype(np.float64) - r64).max()
        assert err < 1e-6 * max(1.0, np.abs(r64).max()), (key, err)


def _signs(seed, index, shape):  # make_golden_train.signs
    rng = np.random.default_rng([seed, index])
    return rng.integers(0, 2, size=(2,) + tuple(shape)).astype(np.float64) * 2.0 - 1.0


@pytest.mark.parametrize("name", CASES)
def test_train_restatement_reproduces_the_reference_loss_and_gradient_at_s9(train_cases, name):
    cfg = CONFIGS[name]
    seed = int(train_cases[f"{name}_seed"].item())
    keys = [k.decode() for k in train_cases[f"{name}_keys"]]
    ref = TrainRef(make_weights(cfg, seed), cfg)
    l_pol, l_val, grads = ref.loss_grad(*make_batch(cfg, 4, seed + 300))
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
    assert torch.isfinite(torch.tensor(train_cases[f"{name}_adam_loss"])).all()
