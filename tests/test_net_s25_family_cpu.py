"""CPU checks of the S = 25 network family (tests/net_s25_family.py): what the table reaches (computed from
tg_net_s25_sample's rule, so that a later change of a plan cannot silently empty it), that both plans of every row are
inside 160 KiB and those of the partners just outside are not, that tg_net_s25_check agrees (0 for every row,
TG_ERR_UNSUPPORTED with the restatement's two byte counts for a partner), the weight blob's size, the float64
restatement against the reference's own recorded outputs at e25 and f25 (tests/golden/net_s25_family_cases.npz), the
eager float32 restatement's distance to float64 (inside the GPU tests' bound for every row, so that their float32
fallback has no reason to trigger at this size), and how many of the sampling tests' draws fall near a cumulative
boundary.  No GPU needed."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, net, ops
from mat_mul_amd._lib import TensorGameError

import net_s25_family as F
from net_ref import Ref, dims, make_weights
from net_s25_ref import EE_SLICES

ROWS = sorted(F.FAMILY25)
PLAN_PARTNERS = ("lim25_c10", "c20_25_c21")  # refused by the LDS plan; e25_n76 by the steps bound
_NEEDS = re.compile(r"LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes")
TOL_GPU = 1e-5  # the GPU tests' bound per tensor, relative to max(1, max |ref|)
UNSUPPORTED = -2  # TG_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def cases(golden):
    return golden("net_s25_family_cases")


# ---- what each row reaches --------------------------------------------------------------------------------------------
def test_the_rows_reach_what_the_table_states():
    geo = {n: F.geometry(n) for n in ROWS}
    # (R, workgroups per game, samples of the last workgroup, R * heads)
    assert geo == {"e25": (2, 7, 1, 6), "f25": (4, 16, 4, 8), "odd25": (2, 6, 1, 10), "ones25": (1, 1, 1, 1),
                   "t8_25": (2, 10, 1, 16), "c13_25": (2, 4, 1, 6), "r8_25": (8, 3, 4, 16), "lim25": (1, 64, 1, 8),
                   "c20_25": (1, 4, 1, 1)}, geo
    # r8_25's further k: one full workgroup, 8 + 1, 8 + 8
    assert [F.geometry("r8_25", k)[:3] for k in (8, 9, 16, 20)] == [(8, 1, 8), (8, 2, 1), (8, 2, 8), (8, 3, 4)]
    ms = {n: dims(F.FAMILY25[n].cfg) for n in ROWS}
    assert all(m["S"] == _lib.TG_NET_WIDE3_S for m in ms.values())
    # the team loops' second pass (NT / 32 = 8 teams): ragged at odd25, two full passes at t8_25 and r8_25
    for name in ("odd25", "t8_25", "r8_25"):
        assert geo[name][3] > 8, (name, geo[name])
    assert geo["odd25"][3] % 8 and not geo["t8_25"][3] % 8 and not geo["r8_25"][3] % 8
    assert ms["c13_25"]["c"] > ms["c13_25"]["W"] and ms["c20_25"]["c"] > ms["c20_25"]["W"]  # wq = c
    assert {m["n_steps"] % 4 for m in ms.values()} == {0, 1, 2, 3}
    assert {1, 2, 4, 8} <= {g[0] for g in geo.values()}
    assert any(1 < last < R for R, _, last, _ in geo.values()) and any(last == 1 < R for R, _, last, _ in geo.values())
    assert any(chunks == 64 and R == 1 for R, chunks, _, _ in geo.values())
    assert any(m["T"] == 8 and m["dim_s"] == 4 for m in ms.values()) and {2, 3, 4} <= {m["dim_s"] for m in ms.values()}
    # T = 8: the 3 * S * cin input rows are the largest term of the slice plan's qkv
    assert any(3 * 25 * (25 * m["T"] + 1) > max(3 * 50 * m["torso_d"], 50 * m["torso_ff"]) for m in ms.values())
    assert any(m["W"] % 4 == 2 for m in ms.values()) and any(m["W"] % 2 for m in ms.values())
    assert any(m["c"] % 2 for m in ms.values())
    assert {1, 2, 5, 8} <= {m["n_logits"] for m in ms.values()} and {3, 5, 16} <= {m["n_quantile"] for m in ms.values()}
    assert any(m["n_steps"] == 1 for m in ms.values()) and any(m["n_steps"] == 75 for m in ms.values())
    assert any(m["torso_d"] != m["d"] for m in ms.values()) and any(m["torso_heads"] != m["heads"] for m in ms.values())
    assert max(m["blocks"] for m in ms.values()) == 4
    assert set(ms["ones25"].values()) == {1, 25} and ms["ones25"]["S"] == 25
    odd = {k: v for k, v in ms["odd25"].items() if k != "torso_layers"}  # every size; two torso layers
    assert all(v % 2 for v in odd.values()), odd


@pytest.mark.parametrize("name", ROWS)
def test_each_row_is_inside_160_kib_in_both_plans(name):
    m = dims(F.FAMILY25[name].cfg)
    torso, dec = F.inference_bytes(m)
    assert torso == 4 * F.slice_plan(m) <= F.LDS and dec == 4 * F.dec_plan_shared(m, 1) <= F.LDS
    R, chunks, last, _ = F.geometry(name)
    k = F.FAMILY25[name].k
    # tg_net_s25_sample's R: the largest of 1 .. min(k, 8) whose plan fits
    assert 4 * F.dec_plan_shared(m, R) <= F.LDS and (R == min(8, k) or 4 * F.dec_plan_shared(m, R + 1) > F.LDS)
    assert (chunks - 1) * R + last == k and 1 <= last <= R


def test_the_plans_the_table_states():
    plans = {n: F.inference_bytes(dims(F.FAMILY25[n].cfg)) for n in ROWS}
    assert plans["e25"][0] == 83500 and plans["lim25"] == (58300, 161588) and plans["c20_25"] == (92300, 158180)
    assert max(p[0] for p in plans.values()) == plans["c20_25"][0]          # the largest slice plan of the family
    assert 3 * 25 * 25 * 20 * 4 == 150000                                   # c20_25's resident copy, J x c floats
    for name in ("lim25", "c20_25"):                                        # each within 8 KiB of the limit
        assert F.LDS - 8192 < plans[name][1] <= F.LDS, plans[name]
    out = {n: F.inference_bytes(F.outside(n)) for n in F.OUTSIDE25}
    assert out["lim25_c10"] == (59400, 169088) and out["c20_25_c21"] == (93400, 165688)
    for name in PLAN_PARTNERS:
        assert out[name][0] <= F.LDS < out[name][1]
    assert max(out["e25_n76"]) <= F.LDS  # refused by TG_NET_WIDE3_MAX_STEPS, not by a plan


@pytest.mark.parametrize("name", sorted(F.OUTSIDE25))
def test_each_partner_outside_is_one_field_away(name):
    row, field, value = F.OUTSIDE25[name]
    inside, outside = dims(F.FAMILY25[row].cfg), F.outside(name)
    assert {k for k in inside if inside[k] != outside[k]} == {field} and outside[field] == value != inside[field]


# ---- the library's view -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_the_library_accepts_each_row(name):
    m = dims(F.FAMILY25[name].cfg)
    cfg = _lib.NetConfig(**m)
    assert _lib.lib.tg_net_s25_check(C.byref(cfg)) == 0
    c = net.check_config(m, ops.net_s25_check)
    sd = make_weights(m, 0)
    assert ops.net_s25_weights_size(c) == sum(v.size for k, v in sd.items() if not k.endswith("pos_enc_fix"))
    assert net.infer_config(sd) == m
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):  # the other header keeps refusing the size
        net.check_config(m)


@pytest.mark.parametrize("name", PLAN_PARTNERS)
def test_a_partner_outside_is_refused_with_the_restatements_byte_counts(name):
    m = F.outside(name)
    want = F.inference_bytes(m)
    cfg = _lib.NetConfig(**m)
    assert _lib.lib.tg_net_s25_check(C.byref(cfg)) == UNSUPPORTED
    got = _NEEDS.search(_lib.lib.tg_last_error().decode())
    assert got and (int(got.group(1)), int(got.group(2))) == want, _lib.lib.tg_last_error()
    with pytest.raises(TensorGameError, match="LDS plan") as e:
        net.check_config(m, ops.net_s25_check)
    assert e.value.code == UNSUPPORTED
    got = _NEEDS.search(str(e.value))
    assert got and (int(got.group(1)), int(got.group(2))) == want, str(e.value)


def test_the_steps_partner_is_refused_by_the_sizes_own_bound():
    m = F.outside("e25_n76")
    cfg = _lib.NetConfig(**m)
    assert _lib.lib.tg_net_s25_check(C.byref(cfg)) == UNSUPPORTED
    assert b"n_steps=76 above TG_NET_WIDE3_MAX_STEPS=75" in _lib.lib.tg_last_error()
    with pytest.raises(TensorGameError, match="TG_NET_WIDE3_MAX_STEPS") as e:
        net.check_config(m, ops.net_s25_check)
    assert e.value.code == UNSUPPORTED
    net.check_config(dict(m, n_steps=75), ops.net_s25_check)


# ---- the restatement against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_restatement_reproduces_the_float64_reference(cases, name):
    cfg = F.FAMILY25[name].cfg
    m = dims(cfg)
    assert int(cases[f"{name}_seed"].item()) == F.SEEDS_NET[name] == F.seed(name)
    ref = Ref(make_weights(cfg, F.seed(name)), cfg)
    n_out = cases[f"{name}_oo64"].shape[0]
    assert 1 <= n_out <= 2 and cases[f"{name}_xx"].shape == (n_out, m["T"], 25, 25, 25)
    assert cases[f"{name}_ss"].shape == (n_out, m["dim_s"]) and tuple(cases[f"{name}_ee_slices"]) == EE_SLICES
    ee = ref.torso(cases[f"{name}_xx"], cases[f"{name}_ss"])
    kept = ee[:1].reshape(1, 25, 75, -1)[:, list(EE_SLICES)]  # rows i*75 .. i*75 + 74 of the first state
    assert cases[f"{name}_ee64"].shape == tuple(kept.shape)
    np.testing.assert_allclose(kept.numpy(), cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, cases[f"{name}_g_action"])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)
    # the reference's own float32 run is inside the GPU tests' bound
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64, r32 = cases[f"{name}_{key}64"], cases[f"{name}_{key}32"]
        assert r32.shape == r64.shape and r32.dtype == np.float32 and r64.dtype == np.float64
        err = np.abs(r32.astype(np.float64) - r64).max()
        print(f"FAMILY-REF32 {name} {key} {err / max(1.0, np.abs(r64).max()):.3g}")
        assert err < TOL_GPU * max(1.0, np.abs(r64).max()), (key, err)


def outputs(name, dtype, B=1):
    ref = Ref(make_weights(F.FAMILY25[name].cfg, F.seed(name)), F.FAMILY25[name].cfg, dtype=dtype)
    xx, ss, ga = F.states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.double().numpy() for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


@pytest.mark.parametrize("name", ROWS)
def test_eager_float32_is_within_the_gpu_bound(name):
    """The eager float32 restatement is inside 1e-5 * max(1, max |ref|) of the float64 one on states(name, 1) for every
    row, so ``train_ref.within``'s fallback has no reason to trigger in the GPU tests.  Measured: at most 6.3e-7
    relative to max(1, max |ref|) over the five tensors and the nine rows (ee of c20_25)."""
    r64, r32 = outputs(name, torch.float64), outputs(name, torch.float32)
    for key, want in r64.items():
        e = float(np.abs(r32[key] - want).max()) / max(1.0, float(np.abs(want).max()))
        print(f"FAMILY-F32 {name} {key} {e:.3g}")
        assert e < TOL_GPU, (name, key, e)


# ---- the sampling tests' draws ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_draws(name):
    cfg = F.FAMILY25[name].cfg
    ref = Ref(make_weights(cfg, F.seed(name)), cfg)
    xx, ss, _ = F.states(name, F.sample_states(name))
    ee = ref.torso(xx, ss)
    return ref, ee, F.sample_own(ref, ee, F.uniforms(name).astype(np.float64))


@pytest.mark.parametrize("name", ROWS)
def test_few_of_the_sampling_tests_draws_are_near_a_boundary(name):
    """The GPU test excludes draws nearer than 1e-5 to a cumulative boundary and caps them at 1 % of all draws.  The
    restatement sampling its own tokens from the same uniforms stays under 0.1 %."""
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    ref, ee, (tokens, probs, dist) = own_draws(name)
    assert tokens.shape == dist.shape == (F.sample_states(name), k, m["n_steps"])
    assert tokens.min() >= 0 and tokens.max() < m["n_logits"]
    near = int((dist < 1e-5).sum())
    print(f"{name}: {near} of {dist.size} draws within 1e-5 of a boundary")
    assert near < 0.001 * dist.size, (near, dist.size)
    assert dist.size >= 2000 or m["n_logits"] == 1
    # sample_own's one-position-at-a-time decode equals the rerun of the whole prefix on the tokens it drew
    B = 1
    tok = torch.from_numpy(tokens[:B]).reshape(B * k, -1)
    start = torch.full((B * k, 1), m["n_logits"], dtype=torch.long)
    oo, _ = ref.decode(ee[:B].repeat_interleave(k, 0), torch.cat([start, tok[:, :-1]], 1))
    np.testing.assert_allclose(torch.softmax(oo, -1).numpy().reshape(B, k, m["n_steps"], -1), probs[:B], rtol=0,
                               atol=1e-12)
