"""CPU checks of the network family (tests/net_family.py): the float64 restatements against the reference's own recorded
outputs at its reachable rows (tests/golden/net_family_cases.npz, train_family_cases.npz), which rows the library
accepts, configuration inference and the weight blob at every row, the LDS plan restatement against the byte counts
the library prints over a seeded sweep of the family, and what the table covers.  No GPU needed."""
import re

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, ops
from mat_mul_amd._lib import TensorGameError
from mat_mul_amd.net import check_config, infer_config, pack_weights
from mat_mul_amd.train import unpack_weights

import net_family as F
from net_ref import FIELDS, P, Ref, dims, make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from train_ref import TrainRef, make_batch

ROWS = sorted(F.FAMILY)
TRAIN_ROWS = [r for r in F.REFERENCE_ROWS if F.FAMILY[r].train]


@pytest.fixture(scope="module")
def net_cases(golden):
    return golden("net_family_cases")


@pytest.fixture(scope="module")
def train_cases(golden):
    return golden("train_family_cases")


# ---- the restatements against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_restatement_reproduces_the_float64_reference(net_cases, name):
    cfg = F.FAMILY[name].cfg
    m = dims(cfg)
    ref = Ref(make_weights(cfg, int(net_cases[f"{name}_seed"].item())), cfg)
    n_out, n_ee = net_cases[f"{name}_oo64"].shape[0], net_cases[f"{name}_ee64"].shape[0]
    assert net_cases[f"{name}_xx"].shape == (16, m["T"], m["S"], m["S"], m["S"])
    ee = ref.torso(net_cases[f"{name}_xx"][:n_out], net_cases[f"{name}_ss"][:n_out])
    np.testing.assert_allclose(ee[:n_ee].numpy(), net_cases[f"{name}_ee64"], rtol=0, atol=1e-10)
    oo, zz0, q = ref.teacher(ee, net_cases[f"{name}_g_action"][:n_out])
    for got, key in ((oo, "oo"), (zz0, "zz0"), (q, "q"), (Ref.risk(q), "qq")):
        np.testing.assert_allclose(got.numpy(), net_cases[f"{name}_{key}64"], rtol=0, atol=1e-10, err_msg=key)


@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_reference_float32_is_within_the_precision_bound(net_cases, name):
    for key in ("ee", "oo", "zz0", "q", "qq"):
        r64 = net_cases[f"{name}_{key}64"]
        err = np.abs(net_cases[f"{name}_{key}32"].astype(np.float64) - r64).max()
        assert err < 1e-5 * max(1.0, np.abs(r64).max()), (key, err)


def _signs(seed, index, shape):  # make_golden_train.signs
    rng = np.random.default_rng([seed, index])
    return rng.integers(0, 2, size=(2,) + tuple(shape)).astype(np.float64) * 2.0 - 1.0


@pytest.mark.parametrize("name", TRAIN_ROWS)
def test_train_restatement_reproduces_the_reference_loss_and_gradient(train_cases, name):
    cfg = F.FAMILY[name].cfg
    seed = int(train_cases[f"{name}_seed"].item())
    keys = [k.decode() for k in train_cases[f"{name}_keys"]]
    ref = TrainRef(make_weights(cfg, seed), cfg)
    l_pol, l_val, grads = ref.loss_grad(*make_batch(cfg, 4, seed + 300))
    assert abs(l_pol - train_cases[f"{name}_l_pol"].item()) <= 1e-9 * abs(l_pol)
    assert abs(l_val - train_cases[f"{name}_l_val"].item()) <= 1e-9 * abs(l_val)
    norm, dot = train_cases[f"{name}_gnorm"], train_cases[f"{name}_gdot"]
    assert sorted(keys) == sorted(make_weights(cfg, seed))
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
    assert full
    for k in full:
        np.testing.assert_allclose(grads[k], train_cases[f"{name}_g_{k}"], rtol=0, atol=1e-9, err_msg=k)
    assert torch.isfinite(torch.tensor(train_cases[f"{name}_adam_loss"])).all()


# ---- the library's view of each row ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_the_library_accepts_or_refuses_each_row_as_flagged(name):
    row = F.FAMILY[name]
    c = check_config(dims(row.cfg))
    if row.train:
        ops.net_train_check(c)
    else:
        with pytest.raises(TensorGameError, match="training LDS plan"):
            ops.net_train_check(c)


@pytest.mark.parametrize("name", ROWS)
def test_config_inference_returns_the_row(name):
    cfg = F.FAMILY[name].cfg
    assert infer_config(make_weights(cfg, 0)) == dims(cfg)


@pytest.mark.parametrize("name", ROWS)
def test_unpack_inverts_pack_exactly(name):
    cfg = F.FAMILY[name].cfg
    sd = make_weights(cfg, 4)
    m = dims(cfg)
    theta = pack_weights(sd, m, fold_pos=False)
    assert theta.size == ops.net_weights_size(check_config(m))
    back = unpack_weights(theta, m, sd[P + "pos_enc_fix"])
    assert sorted(back) == sorted(sd)
    for k, v in sd.items():
        assert back[k].dtype == torch.float32 and np.array_equal(back[k].numpy(), v), k


# ---- the LDS plans --------------------------------------------------------------------------------------------------
_NEEDS = re.compile(r"LDS plan needs (\d+) \(torso\) / (\d+) \(decoder\) bytes")


def sweep(n, seed):
    """n configurations inside the TG_NET_MAX_* bounds, 30 % of them at S = 9.  Each configuration draws a size u: each
    of its fields is uniform in [1, bound] with probability u, log-uniform otherwise, so that small and large
    configurations, accepted and refused ones, all occur."""
    rng = np.random.default_rng(seed)
    lim = _lib.NET_LIMITS
    for _ in range(n):
        u = rng.random() ** 0.3
        m = {k: int(rng.integers(1, lim[k] + 1)) if rng.random() < u
             else min(lim[k], int(np.exp(rng.uniform(0.0, np.log(lim[k] + 1.0))))) for k in FIELDS}
        if rng.random() < 0.3:
            m["S"] = _lib.TG_NET_WIDE_S
            m["n_steps"] = int(rng.integers(1, _lib.TG_NET_WIDE_MAX_STEPS + 1))
        yield m


def library_bytes(check, m):
    """None if ``check`` accepts m, else the (torso, decoder) bytes of its refusal."""
    try:
        check(_lib.NetConfig(**m))
    except TensorGameError as e:
        got = _NEEDS.search(str(e))
        assert got, str(e)
        return int(got.group(1)), int(got.group(2))
    return None


def test_plan_restatement_matches_the_library_over_a_sweep():
    counts = dict(accepted=0, refused=0, train_accepted=0, train_refused=0, wide=0)
    rows = set()
    for m in sweep(3000, 2024):
        counts["wide"] += m["S"] == F.WIDE_S
        inf = library_bytes(ops.net_check, m)
        want = F.inference_bytes(m)
        if inf is not None:
            assert inf == want, (m, inf, want)
            counts["refused"] += 1
            continue
        assert F.fits(want), (m, want)
        counts["accepted"] += 1
        rows.add(F.decoder_rows(m, 8))
        tr = library_bytes(ops.net_train_check, m)
        want = F.training_bytes(m)
        if tr is not None:
            assert tr == want, (m, tr, want)
            counts["train_refused"] += 1
        else:
            assert F.fits(want), (m, want)
            if m["S"] == F.WIDE_S:
                assert F.torso_chunk(m) >= 1 and 4 * F.tplan(m, F.torso_chunk(m)) <= F.LDS
            counts["train_accepted"] += 1
    # the sweep reaches both sides of both checks, and R takes every value
    assert min(counts.values()) >= 100, counts
    assert rows == set(range(1, 9)), rows


@pytest.mark.parametrize("name", ROWS)
def test_plan_restatement_matches_the_library_at_each_row(name):
    m = dims(F.FAMILY[name].cfg)
    assert library_bytes(ops.net_check, m) is None and F.fits(F.inference_bytes(m))
    tr = library_bytes(ops.net_train_check, m)
    assert (tr is None) == F.FAMILY[name].train
    if tr is not None:
        assert tr == F.training_bytes(m)
    R = F.decoder_rows(m, F.FAMILY[name].k)
    assert 4 * F.dec_plan(m, R) <= F.LDS and (R == min(8, F.FAMILY[name].k) or 4 * F.dec_plan(m, R + 1) > F.LDS)


def test_the_family_covers_what_the_five_base_configurations_miss():
    ms = {name: dims(row.cfg) for name, row in F.FAMILY.items()}
    ks = {name: row.k for name, row in F.FAMILY.items()}
    R = {name: F.decoder_rows(ms[name], ks[name]) for name in ms}
    assert {1, 2, 4, 5, 8} <= set(R.values()), R
    assert any(ks[n] % R[n] for n in ms)
    assert any(k > 8 for k in ks.values())
    wide = [dims(c) for c in CONFIGS_S9.values()] + [ms[n] for n in ms if ms[n]["S"] == F.WIDE_S and F.FAMILY[n].train]
    assert {3, 5, 9} <= {F.torso_chunk(m) for m in wide}
    assert any(F.FAMILY[n].train and F.LDS - 1024 <= F.training_bytes(ms[n])[1] <= F.LDS for n in ms)
    assert any(m["W"] % 4 for m in ms.values())
    assert any(m["dim_s"] > 1 for m in ms.values())
    assert any(m["torso_d"] != m["d"] for m in ms.values())
    assert any(m["torso_heads"] != m["heads"] for m in ms.values())
    assert any(m["n_quantile"] != 8 for m in ms.values())
    assert {1, 8} <= {m["n_logits"] for m in ms.values()}
    assert ms["lim"] == _lib.NET_LIMITS and set(ms["ones"].values()) == {1}
