"""CPU checks of the training path (include/tensor_game_train.h, mat_mul_amd.train): train_ref's float64 autograd
against the reference's own recorded losses, gradients and AdamW steps (tests/golden/train_cases.npz), the parameter
vector's packing, and the C ABI's argument validation (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, ops
from mat_mul_amd._lib import NET_LIMITS, TensorGameError
from mat_mul_amd.net import check_config, infer_config, pack_weights
from mat_mul_amd.train import blob_layout, unpack_weights

from net_ref import CONFIGS, P, dims, make_weights
from train_ref import TrainRef, keep_mask, make_batch

CASES = sorted(CONFIGS)
B_CASE = 4
FULL = ["value_head.mlp.6.weight", "value_head.mlp.6.bias", P + "li1.weight", P + "li1.bias", P + "emb1.weight",
        P + "pos_enc"] + [f"torso.li1.{i}.{w}" for i in range(3) for w in ("weight", "bias")]


@pytest.fixture(scope="module")
def cases(golden):
    return golden("train_cases")


def signs(seed, index, shape):  # make_golden_train.signs
    rng = np.random.default_rng([seed, index])
    return rng.integers(0, 2, size=(2,) + tuple(shape)).astype(np.float64) * 2.0 - 1.0


def check_projections(seed, keys, values, norm, dot, rtol):
    for i, k in enumerate(keys):
        v = values.get(k)
        if v is None:
            assert norm[i] == 0.0, k
            continue
        s = signs(seed, i, v.shape)
        scale = max(1.0, norm[i])
        assert abs(np.sqrt((v * v).sum()) - norm[i]) <= rtol * scale, k
        assert abs((s[0] * v).sum() - dot[i, 0]) <= rtol * scale * np.sqrt(v.size), k
        assert abs((s[1] * v).sum() - dot[i, 1]) <= rtol * scale * np.sqrt(v.size), k


def setup(cases, name):
    cfg = CONFIGS[name]
    seed = int(cases[f"{name}_seed"].item())
    keys = [k.decode() for k in cases[f"{name}_keys"]]
    return cfg, seed, keys, make_batch(cfg, B_CASE, seed + 300)


@pytest.mark.parametrize("name", CASES)
def test_train_ref_reproduces_the_reference_loss_and_gradient(cases, name):
    cfg, seed, keys, batch = setup(cases, name)
    ref = TrainRef(make_weights(cfg, seed), cfg)
    l_pol, l_val, grads = ref.loss_grad(*batch)
    assert abs(l_pol - cases[f"{name}_l_pol"].item()) <= 1e-9 * abs(l_pol)
    assert abs(l_val - cases[f"{name}_l_val"].item()) <= 1e-9 * abs(l_val)
    check_projections(seed, keys, grads, cases[f"{name}_gnorm"], cases[f"{name}_gdot"], 1e-9)
    for k in FULL:
        want = cases[f"{name}_g_{k}"]
        np.testing.assert_allclose(grads[k], want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()), err_msg=k)


@pytest.mark.parametrize("name", CASES)
def test_train_ref_reproduces_three_adamw_steps(cases, name):
    cfg, seed, keys, batch = setup(cases, name)
    ref = TrainRef(make_weights(cfg, seed), cfg)
    params = [ref.w[k] for k in keys if ref.w[k].requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        l_pol, l_val = ref.losses(*batch)
        loss = l_pol + 1000.0 * l_val
        loss.backward()
        opt.step()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, cases[f"{name}_adam_loss"], rtol=1e-9)
    values = {k: v.detach().numpy() for k, v in ref.w.items()}
    check_projections(seed, keys, values, cases[f"{name}_pnorm"], cases[f"{name}_pdot"], 1e-9)
    for k in FULL:
        np.testing.assert_allclose(values[k], cases[f"{name}_p_{k}"], rtol=0, atol=1e-9, err_msg=k)


@pytest.mark.parametrize("name", CASES)
def test_unpack_inverts_pack_exactly(name):
    sd = make_weights(CONFIGS[name], 3)
    cfg = infer_config(sd)
    theta = pack_weights(sd, cfg, fold_pos=False)
    back = unpack_weights(theta, cfg, sd[P + "pos_enc_fix"])
    assert sorted(back) == sorted(sd)
    for k, v in sd.items():
        assert back[k].dtype == torch.float32 and np.array_equal(back[k].numpy(), v), k
    # the layout's size is the library's, and the inference blob differs only in the pos slot
    assert theta.size == ops.net_weights_size(check_config(cfg))
    blob = pack_weights(sd, cfg)
    pos = next(e for e in blob_layout(cfg) if e[2] == "pos")
    sl = slice(pos[3], pos[3] + sd[P + "pos_enc"].size)
    assert np.array_equal(np.delete(blob, np.arange(sl.start, sl.stop)), np.delete(theta, np.arange(sl.start, sl.stop)))
    assert np.array_equal(blob[sl], (theta[sl] + sd[P + "pos_enc_fix"].reshape(-1)).astype(np.float32))
    folded = unpack_weights(blob, cfg, sd[P + "pos_enc_fix"], folded=True)
    np.testing.assert_allclose(folded[P + "pos_enc"].numpy(), sd[P + "pos_enc"], rtol=0, atol=1e-6)


def test_keep_rule_restatement_is_a_fair_coin():
    m = dims(CONFIGS["a"])
    k = keep_mask(7, 3, 200, m, 0.5)
    assert k.shape == (200, m["blocks"], 2, m["n_steps"], m["W"]) and abs(k.mean() - 0.5) < 0.01
    assert keep_mask(7, 3, 200, m, 0.0).all()
    assert not np.array_equal(k, keep_mask(7, 4, 200, m, 0.5))


def _cfg(**over):
    c = dims(CONFIGS["a"])
    c.update(over)
    return _lib.NetConfig(**c)


@pytest.mark.parametrize("name", CASES)
def test_training_family_holds_the_three_configurations(name):
    ops.net_train_check(check_config(dims(CONFIGS[name])))
    n = ops.net_weights_size(check_config(dims(CONFIGS[name])))
    for B in (1, 256, 4096):
        ws = ops.net_train_workspace_size(check_config(dims(CONFIGS[name])), B)
        assert ws >= 4 * min(B, _lib.TG_NET_TRAIN_PARTIALS) * n and ws % 256 == 0
    # the slabs are bounded: past TG_NET_TRAIN_PARTIALS games the workspace grows by the activations only
    c = check_config(dims(CONFIGS[name]))
    m = dims(CONFIGS[name])
    per_game = 4 * (2 * 3 * m["S"] ** 2 * m["c"] + m["torso_layers"] * 3 * 2 * m["S"] ** 2 * m["c"] + 3)
    grow = ops.net_train_workspace_size(c, 8192) - ops.net_train_workspace_size(c, 4096)
    assert 4096 * per_game <= grow <= 4096 * per_game + 5 * 256


def test_training_family_refuses_the_inference_family_at_its_bounds():
    big = _lib.NetConfig(**NET_LIMITS)
    ops.net_check(big)  # inside the inference family
    with pytest.raises(TensorGameError, match="training LDS plan"):
        ops.net_train_check(big)
    with pytest.raises(TensorGameError, match="TG_NET_MAX_W"):
        ops.net_train_check(_cfg(W=128))
    with pytest.raises(TensorGameError):
        ops.net_train_workspace_size(big, 4)


def _loss_grad(cfg, B=4, p=0.0, theta=1, pos=1, frames=1, scalars=1, act=1, val=1, ws=1, ws_bytes=1 << 40, grad=1,
               losses=1, status=1, i8=1):
    ptr = lambda v: C.c_void_p(0x10000 if v else 0)  # noqa: E731  (never dereferenced: validation fails first)
    return _lib.lib.tg_net_loss_grad(C.byref(cfg), ptr(theta), ptr(pos), ptr(frames), i8, ptr(scalars), ptr(act),
                                     ptr(val), B, 1.0, 1000.0, p, 0, 0, None, None, ptr(ws), ws_bytes, ptr(grad),
                                     ptr(losses), ptr(status), None)


def test_loss_grad_validates_before_touching_a_device():
    cfg = _cfg()
    for kw in (dict(p=1.0), dict(p=-0.1), dict(p=float("nan")), dict(B=0), dict(theta=0), dict(pos=0), dict(frames=0),
               dict(scalars=0), dict(act=0), dict(val=0), dict(ws=0), dict(losses=0), dict(status=0), dict(i8=2),
               dict(ws_bytes=100)):
        assert _loss_grad(cfg, **kw) == -1, kw
        assert b"tg_net_loss_grad" in _lib.lib.tg_last_error(), kw
    assert _loss_grad(_lib.NetConfig(**NET_LIMITS)) == -2
    assert b"training LDS plan" in _lib.lib.tg_last_error()
    assert _lib.lib.tg_net_train_workspace_size(C.byref(cfg), 4, None) == -1
    assert _lib.lib.tg_net_train_check(None) == -1


def test_python_binding_validates_arguments():
    c = check_config(dims(CONFIGS["a"]))
    theta = torch.zeros(ops.net_weights_size(c))
    with pytest.raises(TensorGameError):
        ops.net_loss_grad(c, theta, torch.zeros(12, 32), torch.zeros(2, 2, 4, 4, 4), torch.zeros(2, 1),
                          torch.zeros(2, 12, dtype=torch.int8), torch.zeros(2, 1), torch.zeros(16, dtype=torch.uint8))
