"""CPU checks of the network at the 4x4 matmul tensor (S = TG_NET_WIDE2_S = 16, include/tensor_game_net.h): the family's
third state size and its bounds, the LDS plans the library prints there against their restatement (net_s16_ref), that
training stays refused, argument validation before any launch, and the float64 restatement against the reference's own
recorded S = 16 outputs (tests/golden/net_s16_cases.npz).  No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import FIELDS, Ref, dims, make_weights
from net_s16_ref import CONFIGS, LDS, SEEDS_NET, inference_bytes

CASES = sorted(CONFIGS)
_NEEDS = re.compile(r"LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes")


@pytest.mark.parametrize("name", CASES)
def test_the_inference_family_holds_s16(name):
    c = net.check_config(dims(CONFIGS[name]))
    assert c.S == 16 and c.n_steps == 48
    assert ops.net_weights_size(c) == sum(v.size for k, v in make_weights(CONFIGS[name], 0).items()
                                          if not k.endswith("pos_enc_fix"))
    assert all(b <= LDS for b in inference_bytes(dims(CONFIGS[name])))


def test_the_constants_mirror_the_header():
    assert (_lib.TG_NET_WIDE2_S, _lib.TG_NET_WIDE2_MAX_STEPS) == (16, 48)
    text = (Path(__file__).resolve().parent.parent / "include" / "tensor_game_net.h").read_text()
    assert re.search(r"#define TG_NET_WIDE2_S 16\b", text) and re.search(r"#define TG_NET_WIDE2_MAX_STEPS 48\b", text)
    assert (_lib.TG_NET_WIDE_S, _lib.TG_NET_WIDE_MAX_STEPS) == (9, 27)  # the first wide size keeps its own


def test_s16_has_its_own_steps_bound():
    cfg = dims(CONFIGS["a16"])
    with pytest.raises(TensorGameError, match="TG_NET_WIDE2_MAX_STEPS") as e:
        net.check_config(dict(cfg, n_steps=49))
    assert e.value.code == -2
    net.check_config(dict(cfg, n_steps=28))  # above the S = 9 bound, inside this one


@pytest.mark.parametrize("S", [11, 15, 17, 25])
def test_other_state_sizes_are_refused(S):
    cfg = dict(dims(CONFIGS["a16"]), S=S)
    for check in (net.check_config, lambda m: ops.net_train_check(_lib.NetConfig(**m))):
        with pytest.raises(TensorGameError, match="TG_NET_MAX_S") as e:
            check(cfg)
        assert e.value.code == -2


def test_every_other_bound_still_applies_at_s16():
    with pytest.raises(TensorGameError, match="TG_NET_MAX_W"):
        net.check_config(dict(dims(CONFIGS["a16"]), W=128))
    with pytest.raises(TensorGameError, match="TG_NET_MAX_T"):
        net.check_config(dict(dims(CONFIGS["a16"]), T=9))


def test_an_s16_configuration_whose_plan_cannot_fit_is_refused():
    with pytest.raises(TensorGameError, match="LDS plan"):
        net.check_config(dict(dims(CONFIGS["a16"]), c=32, W=64, blocks=4))


def sweep(n, seed):
    """n configurations at S = 16 inside the TG_NET_MAX_* bounds (n_steps inside its S = 16 bound).  Each draws a size
    u: each field is uniform in [1, bound] with probability u, log-uniform otherwise (test_net_family_cpu.sweep), so
    that accepted and refused configurations both occur."""
    rng = np.random.default_rng(seed)
    lim = _lib.NET_LIMITS
    for _ in range(n):
        u = rng.random() ** 0.3
        m = {k: int(rng.integers(1, lim[k] + 1)) if rng.random() < u
             else min(lim[k], int(np.exp(rng.uniform(0.0, np.log(lim[k] + 1.0))))) for k in FIELDS}
        m["S"] = _lib.TG_NET_WIDE2_S
        m["n_steps"] = int(rng.integers(1, _lib.TG_NET_WIDE2_MAX_STEPS + 1))
        yield m


def test_plan_restatement_matches_the_library_over_a_sweep():
    accepted = refused = 0
    for m in sweep(400, 1616):
        want = inference_bytes(m)
        try:
            ops.net_check(_lib.NetConfig(**m))
        except TensorGameError as e:
            got = _NEEDS.search(str(e))
            assert got, str(e)
            assert (int(got.group(1)), int(got.group(2))) == want, (m, str(e), want)
            assert max(want) > LDS
            refused += 1
            continue
        assert max(want) <= LDS, (m, want)
        accepted += 1
    assert accepted >= 50 and refused >= 50, (accepted, refused)


@pytest.mark.parametrize("name", CASES)
def test_training_is_refused_at_s16(name):
    c = net.check_config(dims(CONFIGS[name]))
    with pytest.raises(TensorGameError, match="training at dim_3d=16 .* is not built") as e:
        ops.net_train_check(c)
    assert e.value.code == -2
    with pytest.raises(TensorGameError, match="is not built"):
        ops.net_train_workspace_size(c, 16)


def test_abi_argument_validation_without_gpu_s16():
    lib = _lib.lib
    cfg = net.check_config(dims(CONFIGS["a16"]))
    bad = _lib.NetConfig(**dict(dims(CONFIGS["a16"]), n_steps=49))
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch
    assert lib.tg_net_check(C.byref(cfg)) == 0
    assert lib.tg_net_check(C.byref(bad)) == -2
    assert b"TG_NET_WIDE2_MAX_STEPS" in lib.tg_last_error()
    assert lib.tg_net_train_check(C.byref(cfg)) == -2
    assert lib.tg_net_torso(C.byref(cfg), None, p, 0, p, p, 4, None) == -1
    assert b"null weights" in lib.tg_last_error()
    assert lib.tg_net_torso(C.byref(cfg), p, p, 2, p, p, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, None, 0, p, p, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, None, p, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, p, None, 4, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), C.c_void_p(66), p, 0, p, p, 4, None) == -1  # misaligned weights
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, p, C.c_void_p(66), 4, None) == -1  # misaligned ee
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, p, p, -1, None) == -1
    assert lib.tg_net_torso(C.byref(cfg), p, p, 0, p, p, 1 << 28, None) == -1          # B x S workgroups: too large a grid
    assert b"too large a grid" in lib.tg_last_error()
    assert lib.tg_net_torso(C.byref(bad), p, p, 0, p, p, 4, None) == -2
    assert lib.tg_net_torso(C.byref(cfg), p, None, 0, None, None, 0, None) == 0  # B = 0 is a no-op
    assert lib.tg_net_sample(C.byref(cfg), p, p, p, 4, 0, 0, 0, None, None, None, None, None) == -2
    assert lib.tg_net_sample(C.byref(cfg), p, p, p, 4, 65, 0, 0, None, None, None, None, None) == -2
    assert lib.tg_net_sample(C.byref(cfg), p, p, None, 4, 8, 0, 0, None, None, None, None, None) == -1
    assert lib.tg_net_sample(C.byref(cfg), p, C.c_void_p(66), p, 4, 8, 0, 0, None, None, None, None, None) == -1
    assert lib.tg_net_sample(C.byref(bad), p, p, p, 4, 8, 0, 0, None, None, None, None, None) == -2
    assert lib.tg_net_sample(C.byref(cfg), p, None, None, 0, 8, 0, 0, None, None, None, None, None) == 0
    assert lib.tg_net_logits(C.byref(cfg), p, p, None, 4, None, None, None, None) == -1
    assert lib.tg_net_logits(C.byref(cfg), p, p, C.c_void_p(68), 4, None, None, None, None) == -1  # misaligned
    assert lib.tg_net_logits(C.byref(cfg), p, None, None, 0, None, None, None, None) == 0


@pytest.fixture(scope="module")
def net_cases(golden):
    return golden("net_s16_cases")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_float64_reference_at_s16(net_cases, name):
    cfg = CONFIGS[name]
    assert int(net_cases[f"{name}_seed"].item()) == SEEDS_NET[name]
    ref = Ref(make_weights(cfg, SEEDS_NET[name]), cfg)
    n_out, n_ee = net_cases[f"{name}_oo64"].shape[0], net_cases[f"{name}_ee64"].shape[0]
    assert net_cases[f"{name}_xx"].shape[1:] == (cfg["dim_t"], 16, 16, 16)
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
