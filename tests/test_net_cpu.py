"""CPU checks of the fused network (include/tensor_game_net.h, mat_mul_amd.net): the float64 restatement against the
reference's own recorded outputs (tests/golden/net_cases.npz), the precision bound, configuration inference, the
supported family, the weight blob and the C ABI's argument validation (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import CONFIGS, Ref, dims, make_weights, philox_uniforms, pick

CASES = sorted(CONFIGS)


@pytest.fixture(scope="module")
def cases(golden):
    return golden("net_cases")


def bound(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_float64_reference(cases, name):
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, int(cases[f"{name}_seed"].item())), cfg)
    n_out, n_ee = cases[f"{name}_oo64"].shape[0], cases[f"{name}_ee64"].shape[0]
    ee = ref.torso(cases[f"{name}_xx"][:n_out], cases[f"{name}_ss"][:n_out])
    np.testing.assert_allclose(ee[:n_ee].numpy(), cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, cases[f"{name}_g_action"][:n_out])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)


@pytest.mark.parametrize("name", CASES)
def test_reference_float32_is_within_the_precision_bound(cases, name):
    worst = 0.0
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64 = cases[f"{name}_{key}64"]
        err = np.abs(cases[f"{name}_{key}32"].astype(np.float64) - r64).max()
        assert err < bound(r64), (key, err)
        worst = max(worst, err / max(1.0, np.abs(r64).max()))
    assert worst < 1e-6  # the bound has a margin of 10x over the reference's own float32 rounding


@pytest.mark.parametrize("name", CASES)
def test_config_inference_from_the_recorded_keys(cases, name):
    keys, shapes = cases[f"{name}_keys"], cases[f"{name}_shapes"]
    keys = [k.decode() for k in keys]
    sd = {k: np.zeros(tuple(int(x) for x in s if x), np.float32) for k, s in zip(keys, shapes)}
    assert net.infer_config(sd) == dims(CONFIGS[name])
    # make_weights produces exactly the reference's key set and shapes
    w = make_weights(CONFIGS[name], 0)
    assert sorted(w) == sorted(keys)
    for k, s in zip(keys, shapes):
        assert w[k].shape == tuple(int(x) for x in s if x), k


def test_infer_config_refuses_other_state_dicts():
    with pytest.raises(TensorGameError, match="missing"):
        net.infer_config({"torso.li1.0.weight": np.zeros((16, 1))})


@pytest.mark.parametrize("field,value,bound_name", [
    ("S", 6, "TG_NET_MAX_S"), ("T", 9, "TG_NET_MAX_T"), ("dim_s", 5, "TG_NET_MAX_DIM_S"), ("c", 33, "TG_NET_MAX_C"),
    ("W", 128, "TG_NET_MAX_W"), ("heads", 9, "TG_NET_MAX_HEADS"), ("d", 65, "TG_NET_MAX_D"),
    ("torso_layers", 17, "TG_NET_MAX_LAYERS"), ("blocks", 5, "TG_NET_MAX_BLOCKS"), ("n_steps", 17, "TG_NET_MAX_STEPS"),
    ("n_logits", 9, "TG_NET_MAX_LOGITS"), ("n_hidden", 513, "TG_NET_MAX_HIDDEN"),
    ("n_quantile", 17, "TG_NET_MAX_QUANTILE"), ("ff", 257, "TG_NET_MAX_FF"), ("torso_ff", 129, "TG_NET_MAX_TORSO_FF")])
def test_unsupported_configurations_are_refused_by_name(field, value, bound_name):
    cfg = dims(CONFIGS["a"])
    cfg[field] = value
    with pytest.raises(TensorGameError, match=bound_name) as e:
        net.check_config(cfg)
    assert e.value.code == -2  # TG_ERR_UNSUPPORTED


def test_the_reference_constructor_default_is_outside_the_family():
    cfg = dict(dims(CONFIGS["a"]), W=2048, heads=32, ff=8192, d=32)
    with pytest.raises(TensorGameError, match="TG_NET_MAX_W"):
        net.check_config(cfg)


def test_the_bounds_themselves_are_supported():
    L = _lib.NET_LIMITS
    net.check_config(dict(L))  # every dimension at its bound: the LDS plan fits
    with pytest.raises(TensorGameError, match="< 1"):
        net.check_config(dict(L, n_steps=0))


@pytest.mark.parametrize("name", CASES)
def test_blob_size_and_packing(name):
    cfg = CONFIGS[name]
    sd = make_weights(cfg, 3)
    m = dims(cfg)
    blob = net.pack_weights(sd, m)
    assert blob.dtype == np.float32 and blob.shape == (ops.net_weights_size(net.check_config(m)),)
    # every parameter appears once (pos_enc and pos_enc_fix as their float64 sum): the blob has the parameter count
    n_params = sum(v.size for v in sd.values()) - sd["policy_head.predict_action_logits.pos_enc_fix"].size
    assert blob.size == n_params
    # spot checks of the layout: the first entry is torso.li1.0.weight transposed, the last the value head's last bias
    S2 = m["S"] ** 2
    np.testing.assert_array_equal(blob[:m["dim_s"] * S2], sd["torso.li1.0.weight"].T.reshape(-1))
    np.testing.assert_array_equal(blob[-m["n_quantile"]:], sd["value_head.mlp.6.bias"])
    p = "policy_head.predict_action_logits."
    pos = (sd[p + "pos_enc"].astype(np.float64) + sd[p + "pos_enc_fix"]).astype(np.float32).reshape(-1)
    i = np.flatnonzero(blob == pos[0])
    assert any(np.array_equal(blob[j:j + pos.size], pos) for j in i)


def test_training_configuration_parameter_count():
    sd = make_weights(CONFIGS["a"], 0)
    n = sum(v.size for k, v in sd.items() if not k.endswith("pos_enc_fix"))
    assert 150_000 < n < 180_000  # about 165 k parameters


def test_abi_argument_validation_without_gpu():
    lib = _lib.lib
    cfg = net.check_config(dims(CONFIGS["a"]))
    bad = _lib.NetConfig(**dict(dims(CONFIGS["a"]), S=6))
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch
    assert lib.tg_net_check(None) == -1
    assert lib.tg_net_check(C.byref(bad)) == -2
    assert b"TG_NET_MAX_S" in lib.tg_last_error()
    n = C.c_int64(0)
    assert lib.tg_net_weights_size(C.byref(cfg), None) == -1
    assert lib.tg_net_torso(C.byref(cfg), None, p, 0, p, p, 4, None) == -1
    assert b"null weights" in lib.tg_last_error()
    assert lib.tg_net_torso(C.byref(cfg), p, p, 2, p, p, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, None, 0, p, p, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), C.c_void_p(66), p, 0, p, p, 4, None) == -1  # misaligned weights
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, p, p, -1, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, None, 0, None, None, 0, None) == 0  # B = 0 is a no-op
    assert lib.tg_net_sample(C.byref(cfg), p, p, p, 4, 0, 0, 0, None, None, None, None, None) == -2
    assert b"TG_NET_MAX_SAMPLES" in lib.tg_last_error()
    assert lib.tg_net_sample(C.byref(cfg), p, p, p, 4, 65, 0, 0, None, None, None, None, None) == -2
    assert lib.tg_net_sample(C.byref(cfg), p, p, None, 4, 8, 0, 0, None, None, None, None, None) == -1
    assert lib.tg_net_sample(C.byref(bad), p, p, p, 4, 8, 0, 0, None, None, None, None, None) == -2
    assert lib.tg_net_logits(C.byref(cfg), p, p, None, 4, None, None, None, None) == -1
    assert lib.tg_net_logits(C.byref(cfg), p, p, C.c_void_p(68), 4, None, None, None, None) == -1  # misaligned
    assert lib.tg_net_weights_size(C.byref(cfg), C.byref(n)) == 0 and n.value > 0


def test_python_layer_needs_a_device():
    sd = make_weights(CONFIGS["a"], 0)
    with pytest.raises(TensorGameError, match="ROCm"):
        net.FusedAlphaTensor.from_state_dict(sd, 8, device="cpu")


def test_host_sampling_rule():
    u = philox_uniforms(5, np.array([0, 7, 2 ** 33 + 1]), 3, 4, 12)
    assert u.shape == (3, 4, 12) and (u >= 0).all() and (u < 1).all()
    assert np.all(u * 2 ** 24 == np.floor(u * 2 ** 24))  # 24-bit grid
    # the row key uses the low 32 bits of the game index; a different call or sample gives different draws
    np.testing.assert_array_equal(u[2], philox_uniforms(5, np.array([1]), 3, 4, 12)[0])
    assert not np.array_equal(u, philox_uniforms(5, np.array([0, 7, 2 ** 33 + 1]), 4, 4, 12))
    tok, dist = pick(np.array([0.05, 0.5, 0.99, 0.3]), np.array([[0.1, 0.2, 0.7]] * 4))
    assert tok.tolist() == [0, 2, 2, 1] and np.isclose(dist[3], 0.0)  # 0.3 < 0.1 + 0.2 in float64
