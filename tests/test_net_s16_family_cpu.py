"""CPU checks of the S = 16 network family (tests/net_s16_family.py): that the library accepts every row and refuses the
partner just outside with the restatement's byte counts, the weight blob's size, what the table reaches (computed from
launch_decode's rule, so that a later change of a plan cannot silently empty it), the float64 restatement against the
reference's own recorded outputs at e16 and f16 (tests/golden/net_s16_family_cases.npz), the eager float32 restatement's
distance to float64 (a tenth of the GPU tests' bound, so that their float32 fallback has no reason to trigger at this
size), and how many of the sampling tests' draws fall near a cumulative boundary.  No GPU needed."""
import functools
import re

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

import net_s16_family as F
from net_ref import Ref, dims, make_weights

ROWS = sorted(F.FAMILY16)
_NEEDS = re.compile(r"LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes")
TOL_GPU = 1e-5  # the GPU tests' bound per tensor, relative to max(1, max |ref|)


@pytest.fixture(scope="module")
def cases(golden):
    return golden("net_s16_family_cases")


# ---- the library's view of each row ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_the_library_accepts_each_row(name):
    m = dims(F.FAMILY16[name].cfg)
    assert m["S"] == _lib.TG_NET_WIDE2_S
    c = net.check_config(m)
    ops.net_check(c)
    assert ops.net_weights_size(c) == sum(v.size for k, v in make_weights(m, 0).items() if not k.endswith("pos_enc_fix"))
    assert net.infer_config(make_weights(m, 0)) == m


@pytest.mark.parametrize("name", ROWS)
def test_each_row_is_inside_160_kib_in_both_plans(name):
    m = dims(F.FAMILY16[name].cfg)
    torso, dec = F.inference_bytes(m)
    assert torso == 4 * F.slice_plan(m) <= F.LDS and dec == 4 * F.dec_plan(m, 1) <= F.LDS
    R, chunks, last, _ = F.geometry(name)
    k = F.FAMILY16[name].k
    # launch_decode's R: the largest of 1 .. min(k, 8) whose plan fits
    assert 4 * F.dec_plan(m, R) <= F.LDS and (R == min(8, k) or 4 * F.dec_plan(m, R + 1) > F.LDS)
    assert (chunks - 1) * R + last == k and 1 <= last <= R


def test_the_partner_just_outside_is_refused_with_the_restatements_byte_counts():
    inside, outside = dims(F.FAMILY16["wide16"].cfg), dims(F.WIDE16_OUTSIDE)
    assert {k for k in inside if inside[k] != outside[k]} == {"blocks"}
    assert F.inference_bytes(inside) == (51200, 150056)
    want = F.inference_bytes(outside)
    assert want == (51200, 260648) and want[0] <= F.LDS < want[1]
    for check in (net.check_config, lambda m: ops.net_check(_lib.NetConfig(**m))):
        with pytest.raises(TensorGameError, match="LDS plan") as e:
            check(outside)
        assert e.value.code == -2
        got = _NEEDS.search(str(e.value))
        assert got and (int(got.group(1)), int(got.group(2))) == want, str(e.value)


def test_the_family_reaches_what_a16_and_b16_share_one_value_of():
    ms = {n: dims(F.FAMILY16[n].cfg) for n in ROWS}
    geo = {n: F.geometry(n) for n in ROWS}
    assert {1, 4, 5, 8} <= {g[0] for g in geo.values()}, geo
    assert any(1 < last < R for R, _, last, _ in geo.values()), geo           # a partial last chunk of several samples
    assert {3, 4} <= {last for R, _, last, _ in geo.values() if last < R}, geo
    assert any(chunks >= 64 for _, chunks, _, _ in geo.values()), geo
    assert any(rh > 8 and rh % 8 for _, _, _, rh in geo.values()), geo         # team-softmax rows: > 8 teams, ragged
    assert any(rh > 8 and rh % 8 == 0 for _, _, _, rh in geo.values()), geo
    assert any(m["c"] > m["W"] for m in ms.values())                           # the wq = max(W, c) stride
    assert any(m["W"] % 4 for m in ms.values()) and any(m["c"] % 2 for m in ms.values())
    assert any(m["W"] % 2 for m in ms.values())
    assert {3, 4} <= {m["dim_s"] for m in ms.values()}
    assert any(m["T"] == 8 for m in ms.values())
    # T = 8: the 3 * S * cin input rows are the largest term of the slice plan's qkv
    assert any(3 * 16 * (16 * m["T"] + 1) > max(3 * 32 * m["torso_d"], 32 * m["torso_ff"]) for m in ms.values())
    assert any(m["n_steps"] == 1 for m in ms.values()) and any(1 < m["n_steps"] < 48 for m in ms.values())
    assert {1, 2, 8} <= {m["n_logits"] for m in ms.values()}
    assert {3, 5, 16} <= {m["n_quantile"] for m in ms.values()}
    assert any(m["torso_d"] != m["d"] for m in ms.values()) and any(m["torso_heads"] != m["heads"] for m in ms.values())
    assert set(ms["ones16"].values()) == {1, 16} and ms["ones16"]["S"] == 16


# ---- the restatement against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_restatement_reproduces_the_float64_reference(cases, name):
    cfg = F.FAMILY16[name].cfg
    m = dims(cfg)
    assert int(cases[f"{name}_seed"].item()) == F.SEEDS_NET[name] == F.seed(name)
    ref = Ref(make_weights(cfg, F.seed(name)), cfg)
    n_out, n_ee = cases[f"{name}_oo64"].shape[0], cases[f"{name}_ee64"].shape[0]
    assert n_out >= 1 and n_ee >= 1
    assert cases[f"{name}_xx"].shape[1:] == (m["T"], 16, 16, 16) and cases[f"{name}_ss"].shape[1:] == (m["dim_s"],)
    ee = ref.torso(cases[f"{name}_xx"][:n_out], cases[f"{name}_ss"][:n_out])
    np.testing.assert_allclose(ee[:n_ee].numpy(), cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, cases[f"{name}_g_action"][:n_out])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)
    # the reference's own float32 run is inside the GPU tests' bound, with a margin
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64 = cases[f"{name}_{key}64"]
        err = np.abs(cases[f"{name}_{key}32"].astype(np.float64) - r64).max()
        assert err < 1e-6 * max(1.0, np.abs(r64).max()), (key, err)


def outputs(name, dtype, B=3):
    ref = Ref(make_weights(F.FAMILY16[name].cfg, F.seed(name)), F.FAMILY16[name].cfg, dtype=dtype)
    xx, ss, ga = F.states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.double().numpy() for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


@pytest.mark.parametrize("name", ROWS)
def test_eager_float32_is_within_a_tenth_of_the_gpu_bound(name):
    """Measured: at most 3.5e-7 relative to max(1, max |ref|) over the five tensors at three states per row."""
    r64, r32 = outputs(name, torch.float64), outputs(name, torch.float32)
    for key, want in r64.items():
        e = float(np.abs(r32[key] - want).max()) / max(1.0, float(np.abs(want).max()))
        print(f"FAMILY-F32 {name} {key} {e:.3g}")
        assert e < 0.1 * TOL_GPU, (name, key, e)


# ---- the sampling tests' draws ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_draws(name):
    cfg = F.FAMILY16[name].cfg
    ref = Ref(make_weights(cfg, F.seed(name)), cfg)
    xx, ss, _ = F.states(name, F.sample_states(name))
    ee = ref.torso(xx, ss)
    return ref, ee, F.sample_own(ref, ee, F.uniforms(name).astype(np.float64))


@pytest.mark.parametrize("name", ROWS)
def test_few_of_the_sampling_tests_draws_are_near_a_boundary(name):
    """The GPU test excludes draws nearer than 1e-5 to a cumulative boundary and caps them at 1 % of all draws.  The
    restatement sampling its own tokens from the same uniforms stays under 0.1 %."""
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
    ref, ee, (tokens, probs, dist) = own_draws(name)
    assert tokens.shape == dist.shape == (F.sample_states(name), k, m["n_steps"])
    assert tokens.min() >= 0 and tokens.max() < m["n_logits"]
    near = int((dist < 1e-5).sum())
    print(f"{name}: {near} of {dist.size} draws within 1e-5 of a boundary")
    assert near < 0.001 * dist.size, (near, dist.size)
    assert dist.size >= 1000 or m["n_logits"] == 1
    # sample_own's one-position-at-a-time decode equals the rerun of the whole prefix on the tokens it drew
    B = 1
    tok = torch.from_numpy(tokens[:B]).reshape(B * k, -1)
    start = torch.full((B * k, 1), m["n_logits"], dtype=torch.long)
    oo, _ = ref.decode(ee[:B].repeat_interleave(k, 0), torch.cat([start, tok[:, :-1]], 1))
    np.testing.assert_allclose(torch.softmax(oo, -1).numpy().reshape(B, k, m["n_steps"], -1), probs[:B], rtol=0,
                               atol=1e-12)
