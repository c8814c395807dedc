"""CPU checks of the network at the 5x5 matmul tensor (S = TG_NET_WIDE3_S = 25, include/tensor_game_net_s25.h): the
header's constants, what tg_net_s25_check accepts and refuses and that tg_net_check keeps refusing the size, the LDS
plans the library prints against their restatement (net_s25_ref), argument validation of the five entries before any
launch, and the float64 restatement against the reference's own recorded S = 25 outputs
(tests/golden/net_s25_cases.npz).  No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

from net_ref import FIELDS, Ref, dims, make_weights
from net_s25_ref import CONFIGS, EE_SLICES, LDS, RECORDED, SEEDS_NET, decoder_rows, inference_bytes

CASES = sorted(CONFIGS)
_NEEDS = re.compile(r"LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes")


def check(m):
    return net.check_config(m, ops.net_s25_check)


def test_the_constants_mirror_the_header():
    assert (_lib.TG_NET_WIDE3_S, _lib.TG_NET_WIDE3_MAX_STEPS) == (25, 75)
    text = (Path(__file__).resolve().parent.parent / "include" / "tensor_game_net_s25.h").read_text()
    assert re.search(r"#define TG_NET_WIDE3_S 25\b", text) and re.search(r"#define TG_NET_WIDE3_MAX_STEPS 75\b", text)
    for name in _lib.NET_S25_SIGNATURES:
        assert re.search(rf"\bint {name}\(", text), name
    assert len(_lib.NET_S25_SIGNATURES) == 5


@pytest.mark.parametrize("name", CASES)
def test_the_s25_family_holds_the_configurations(name):
    c = check(dims(CONFIGS[name]))
    assert c.S == 25 and c.n_steps == 75
    assert ops.net_s25_weights_size(c) == sum(v.size for k, v in make_weights(CONFIGS[name], 0).items()
                                              if not k.endswith("pos_enc_fix"))
    assert all(b <= LDS for b in inference_bytes(dims(CONFIGS[name])))


def test_the_plans_the_header_states():
    a25, b25, c25 = (dims(CONFIGS[n]) for n in ("a25", "b25", "c25"))
    assert inference_bytes(a25) == (38000, 113592)      # 37.1 KiB, 110.9 KiB
    assert inference_bytes(b25)[1] == 106656            # 104.2 KiB
    # one sample per workgroup at a25 whatever k, two at b25 (149.2 KiB); c25 holds its four samples, five at the most
    assert [decoder_rows(a25, k) for k in (1, 2, 8)] == [1, 1, 1]
    assert [decoder_rows(b25, k) for k in (1, 4, 8)] == [1, 2, 2]
    assert [decoder_rows(c25, k) for k in (1, 4, 5, 6, 8)] == [1, 4, 5, 5, 5]


@pytest.mark.parametrize("S", [4, 9, 16, 24, 26])
def test_every_other_state_size_is_refused(S):
    with pytest.raises(TensorGameError, match="tg_net_check") as e:
        check(dict(dims(CONFIGS["a25"]), S=S))
    assert e.value.code == -2
    with pytest.raises(TensorGameError, match="tg_net_check"):
        ops.net_s25_weights_size(_lib.NetConfig(**dict(dims(CONFIGS["a25"]), S=S)))


def test_s25_has_its_own_steps_bound():
    cfg = dims(CONFIGS["a25"])
    with pytest.raises(TensorGameError, match="TG_NET_WIDE3_MAX_STEPS") as e:
        check(dict(cfg, n_steps=76))
    assert e.value.code == -2
    check(dict(cfg, n_steps=49))  # above the S = 16 bound, inside this one
    check(dict(cfg, n_steps=1))


def test_every_other_bound_still_applies_at_s25():
    with pytest.raises(TensorGameError, match=r"W=128 above TG_NET_MAX_W=64"):
        check(dict(dims(CONFIGS["a25"]), W=128))
    with pytest.raises(TensorGameError, match=r"dim_t=9 above TG_NET_MAX_T=8"):
        check(dict(dims(CONFIGS["a25"]), T=9))
    with pytest.raises(TensorGameError, match="blocks=0 < 1") as e:
        check(dict(dims(CONFIGS["a25"]), blocks=0))
    assert e.value.code == -1


def test_an_s25_configuration_whose_plan_cannot_fit_is_refused():
    with pytest.raises(TensorGameError, match="LDS plan"):
        check(dict(dims(CONFIGS["a25"]), c=32, W=64, blocks=4))


def test_the_other_header_still_refuses_s25():
    for name in CASES:
        with pytest.raises(TensorGameError, match="TG_NET_MAX_S") as e:
            ops.net_check(_lib.NetConfig(**dims(CONFIGS[name])))
        assert e.value.code == -2
        with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):
            net.check_config(dims(CONFIGS[name]))


def sweep(n, seed):
    """n configurations at S = 25 inside the TG_NET_MAX_* bounds (n_steps inside its S = 25 bound), drawn as
    test_net_s16_cpu.sweep draws them: each draws a size u, each field is uniform in [1, bound] with probability u and
    log-uniform otherwise, so that accepted and refused configurations both occur."""
    rng = np.random.default_rng(seed)
    lim = _lib.NET_LIMITS
    for _ in range(n):
        u = rng.random() ** 0.3
        m = {k: int(rng.integers(1, lim[k] + 1)) if rng.random() < u
             else min(lim[k], int(np.exp(rng.uniform(0.0, np.log(lim[k] + 1.0))))) for k in FIELDS}
        m["S"] = _lib.TG_NET_WIDE3_S
        m["n_steps"] = int(rng.integers(1, _lib.TG_NET_WIDE3_MAX_STEPS + 1))
        yield m


def test_plan_restatement_matches_the_library_over_a_sweep():
    accepted = refused = 0
    for m in sweep(400, 2525):
        want = inference_bytes(m)
        try:
            ops.net_s25_check(_lib.NetConfig(**m))
        except TensorGameError as e:
            got = _NEEDS.search(str(e))
            assert got, str(e)
            assert (int(got.group(1)), int(got.group(2))) == want, (m, str(e), want)
            assert max(want) > LDS
            refused += 1
            continue
        assert max(want) <= LDS, (m, want)
        accepted += 1
    print(f"accepted {accepted}, refused {refused}")
    assert accepted >= 50 and refused >= 50, (accepted, refused)


def test_abi_argument_validation_without_gpu_s25():
    lib = _lib.lib
    cfg = check(dims(CONFIGS["a25"]))
    bad = _lib.NetConfig(**dict(dims(CONFIGS["a25"]), n_steps=76))
    s16 = _lib.NetConfig(**dict(dims(CONFIGS["a25"]), S=16, n_steps=48))
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch
    n = C.c_int64(0)
    assert lib.tg_net_s25_check(C.byref(cfg)) == 0
    assert lib.tg_net_s25_check(None) == -1
    assert lib.tg_net_s25_check(C.byref(bad)) == -2
    assert b"TG_NET_WIDE3_MAX_STEPS" in lib.tg_last_error()
    assert lib.tg_net_s25_check(C.byref(s16)) == -2
    assert b"tg_net_check" in lib.tg_last_error()
    assert lib.tg_net_check(C.byref(cfg)) == -2 and lib.tg_net_train_check(C.byref(cfg)) == -2
    assert lib.tg_net_s25_weights_size(C.byref(cfg), C.byref(n)) == 0 and n.value > 0
    assert lib.tg_net_s25_weights_size(C.byref(cfg), None) == -1
    assert b"null output" in lib.tg_last_error()
    assert lib.tg_net_s25_weights_size(C.byref(bad), C.byref(n)) == -2
    torso = lib.tg_net_s25_torso
    assert torso(C.byref(cfg), None, p, 0, p, p, 4, None, 0, None) == -1
    assert b"null weights" in lib.tg_last_error()
    assert torso(C.byref(cfg), p, p, 2, p, p, 4, None, 0, None) == -1
    assert torso(C.byref(cfg), p, None, 0, p, p, 4, None, 0, None) == -1
    assert torso(C.byref(cfg), p, p, 0, None, p, 4, None, 0, None) == -1
    assert torso(C.byref(cfg), p, p, 0, p, None, 4, None, 0, None) == -1
    assert torso(C.byref(cfg), C.c_void_p(66), p, 0, p, p, 4, None, 0, None) == -1  # misaligned weights
    assert torso(C.byref(cfg), p, p, 0, p, C.c_void_p(66), 4, None, 0, None) == -1  # misaligned ee
    assert torso(C.byref(cfg), p, p, 0, p, p, -1, None, 0, None) == -1
    assert torso(C.byref(cfg), p, p, 0, p, p, 1 << 28, None, 0, None) == -1          # B x 25 workgroups: too large a grid
    assert b"too large a grid" in lib.tg_last_error()
    assert torso(C.byref(cfg), p, p, 0, p, p, 4, p, 0, None) == -1                   # need = 0 with flags
    assert b"need=0 with flags given" in lib.tg_last_error()
    assert torso(C.byref(cfg), p, p, 0, p, p, 4, p, 256, None) == -1
    assert torso(C.byref(bad), p, p, 0, p, p, 4, None, 0, None) == -2
    assert torso(C.byref(s16), p, p, 0, p, p, 4, None, 0, None) == -2
    assert torso(C.byref(cfg), p, None, 0, None, None, 0, None, 0, None) == 0        # B = 0 is a no-op
    sample = lib.tg_net_s25_sample
    tail = (None, None, None, None)  # uniforms, tokens, probs, q
    assert sample(C.byref(cfg), p, p, p, 4, 0, 0, 0, *tail, None, 0, None) == -2
    assert sample(C.byref(cfg), p, p, p, 4, 65, 0, 0, *tail, None, 0, None) == -2
    assert b"TG_NET_MAX_SAMPLES" in lib.tg_last_error()
    assert sample(C.byref(cfg), p, p, None, 4, 8, 0, 0, *tail, None, 0, None) == -1  # neither rows nor uniforms
    assert sample(C.byref(cfg), p, None, p, 4, 8, 0, 0, *tail, None, 0, None) == -1
    assert sample(C.byref(cfg), p, C.c_void_p(66), p, 4, 8, 0, 0, *tail, None, 0, None) == -1
    assert sample(C.byref(cfg), p, p, p, 4, 8, 0, 0, *tail, p, 0, None) == -1        # need = 0 with flags
    assert b"need=0 with flags given" in lib.tg_last_error()
    assert sample(C.byref(bad), p, p, p, 4, 8, 0, 0, *tail, None, 0, None) == -2
    assert sample(C.byref(s16), p, p, p, 4, 8, 0, 0, *tail, None, 0, None) == -2
    assert sample(C.byref(cfg), None, p, p, 4, 8, 0, 0, *tail, None, 0, None) == -1
    assert sample(C.byref(cfg), p, None, None, 0, 8, 0, 0, *tail, None, 0, None) == 0
    logits = lib.tg_net_s25_logits
    assert logits(C.byref(cfg), p, p, None, 4, None, None, None, None) == -1
    assert logits(C.byref(cfg), p, None, p, 4, None, None, None, None) == -1
    assert logits(C.byref(cfg), p, p, C.c_void_p(68), 4, None, None, None, None) == -1  # misaligned
    assert logits(C.byref(cfg), p, p, p, 4, C.c_void_p(66), None, None, None) == -1
    assert logits(C.byref(bad), p, p, p, 4, None, None, None, None) == -2
    assert logits(C.byref(s16), p, p, p, 4, None, None, None, None) == -2
    assert logits(C.byref(cfg), p, None, None, 0, None, None, None, None) == 0


def test_the_class_takes_that_size_only():
    """FusedAlphaTensor25 refuses before it touches a device; FusedAlphaTensor keeps refusing S = 25."""
    cfg = dims(CONFIGS["c25"])
    with pytest.raises(TensorGameError, match="tg_net_check"):
        net.FusedAlphaTensor25(dict(cfg, S=16, n_steps=48), None, 4)
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):
        net.FusedAlphaTensor(cfg, None, 4)
    with pytest.raises(TensorGameError, match="a ROCm device is required"):
        net.FusedAlphaTensor25.from_state_dict(make_weights(CONFIGS["c25"], 1), 4, device="cpu")
    assert net.infer_config(make_weights(CONFIGS["c25"], 1)) == cfg


@pytest.fixture(scope="module")
def net_cases(golden):
    return golden("net_s25_cases")


@pytest.mark.parametrize("name", RECORDED)
def test_restatement_reproduces_the_float64_reference_at_s25(net_cases, name):
    cfg = CONFIGS[name]
    assert int(net_cases[f"{name}_seed"].item()) == SEEDS_NET[name]
    ref = Ref(make_weights(cfg, SEEDS_NET[name]), cfg)
    n_out = net_cases[f"{name}_oo64"].shape[0]
    assert net_cases[f"{name}_xx"].shape == (4, cfg["dim_t"], 25, 25, 25) and n_out == 2
    assert tuple(net_cases[f"{name}_ee_slices"]) == EE_SLICES
    ee = ref.torso(net_cases[f"{name}_xx"][:n_out], net_cases[f"{name}_ss"][:n_out])
    kept = ee[:1].reshape(1, 25, 75, -1)[:, list(EE_SLICES)]  # rows i*75 .. i*75 + 74 of the first state
    assert net_cases[f"{name}_ee64"].shape == tuple(kept.shape)
    np.testing.assert_allclose(kept.numpy(), net_cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, net_cases[f"{name}_g_action"][:n_out])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), net_cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)
    # the reference's own float32 run against its float64 run, the e32 of the GPU tests' precision rule: printed, and
    # the same outputs in both precisions
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64, r32 = net_cases[f"{name}_{key}64"], net_cases[f"{name}_{key}32"]
        assert r32.shape == r64.shape and r32.dtype == np.float32 and r64.dtype == np.float64
        err = np.abs(r32.astype(np.float64) - r64).max()
        print(f"{name} {key}: e32 {err:.3e}, 1e-5 max(1, max|ref|) {1e-5 * max(1.0, np.abs(r64).max()):.3e}")
        assert np.isfinite(err)
