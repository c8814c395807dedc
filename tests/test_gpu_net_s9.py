"""The fused network at the 3x3 matmul tensor (S = TG_NET_WIDE_S = 9) on the MI355X, for the two S = 9 configurations
of net_s9_ref: the precision bound against the reference's float64 outputs and the float64 restatement at B = 1, 37
and 256, the sampling rule with given uniforms and with the internal stream, input dtypes and row subsets, and graph
capture."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor

from net_ref import Ref, make_inputs, make_weights, philox_uniforms, pick
from net_s9_ref import CONFIGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(CONFIGS)
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_s9_cases.npz"


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def states(name, B):
    """B = 16: the fixture's states; otherwise make_inputs'; with their g_action."""
    cfg = CONFIGS[name]
    f = fixture(name)
    if B == 16:
        return f["xx"], f["ss"], f["g_action"]
    xx, ss = make_inputs(cfg, B, 500 + B)
    ga = np.random.default_rng(600 + B).integers(0, cfg["n_logits"], size=(B, cfg["n_steps"])).astype(np.int8)
    return xx, ss, ga


@functools.lru_cache(maxsize=None)
def host(name, B):
    """The float64 restatement's outputs (ee, oo, zz0, q, qq) for states(name, B)."""
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, int(fixture(name)["seed"].item())), cfg, device=DEV)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.cpu() for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


def setup(name):
    cfg = CONFIGS[name]
    sd = make_weights(cfg, int(fixture(name)["seed"].item()))
    return cfg, sd, FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max()
    assert err <= 1e-5 * max(1.0, np.abs(ref).max()), (what, err)


@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_the_float64_reference(name):
    cfg, sd, net = setup(name)
    f = fixture(name)
    xx, ss, ga = (torch.from_numpy(a).to(DEV) for a in states(name, 16))
    ee = net.torso(xx.float(), ss)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = net.fwd_infer(xx.float(), ss, seed=1)
    assert tuple(aa.shape) == (16, cfg["n_samples"], 27) and tuple(pp.shape) == (16, cfg["n_samples"])
    for got, key in ((ee, "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        rec = f[f"{key}64"]
        close(got[:rec.shape[0]], rec, key)
        close(got, host(name, 16)[key].numpy(), key)


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_the_restatement_by_batch(name, B):
    cfg, sd, net = setup(name)
    xx, ss, ga = (torch.from_numpy(a).to(DEV) for a in states(name, B))
    h = host(name, B)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    _, _, qq = net.fwd_infer(xx, ss, seed=2)
    for got, key in ((net.torso(xx, ss), "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        close(got, h[key].numpy(), key)


def host_check(name, sd, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities."""
    cfg = CONFIGS[name]
    ref = Ref(sd, cfg, device=DEV)
    B, k, n = tokens.shape
    ee = host(name, 16)["ee"].to(DEV).repeat_interleave(k, 0)
    tok = tokens.to(torch.int64).reshape(B * k, n)
    start = torch.full((B * k, 1), cfg["n_logits"], dtype=torch.long, device=DEV)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).cpu().numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    np.testing.assert_allclose(pp.cpu().numpy(), p_chosen.prod(-1), rtol=1e-5, atol=0)
    assert (~keep).sum() < 0.01 * keep.size


@pytest.mark.parametrize("name", CASES)
def test_sampling_follows_the_host_rule(name):
    cfg, sd, net = setup(name)
    k, n = cfg["n_samples"], cfg["n_steps"]
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, 16))
    ee = net.torso(xx, ss)
    u = np.random.default_rng(5).random((16, k, n)).astype(np.float32)
    tokens, pp, _ = net.sample(ee, uniforms=torch.from_numpy(u).to(DEV))
    host_check(name, sd, tokens, pp, u.astype(np.float64))
    rows = torch.arange(16, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = net.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)  # steps 0 .. 26: Philox blocks 0 .. 6
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, n)
    t2, p2, q2 = net.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    host_check(name, sd, t1, p1, u)


@pytest.mark.parametrize("name", CASES)
def test_int8_frames_and_row_subsets(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, 16))
    ee8, eef = net.torso(xx, ss), net.torso(xx.float(), ss)
    assert torch.equal(ee8, eef)
    rows = torch.arange(16, device=DEV, dtype=torch.int64) + 1000
    full = net.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([15, 5, 7, 0, 10], device=DEV)
    part = net.sample(net.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)


@pytest.mark.parametrize("name", CASES)
def test_graph_capture_equals_eager(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = states(name, 16)
    x, s = torch.from_numpy(xx).to(DEV).float(), torch.from_numpy(ss).to(DEV)
    rows = torch.arange(16, device=DEV, dtype=torch.int64)
    want = net.sample(net.torso(x, s), rows=rows, seed=2, call=5)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        net.sample(net.torso(x, s), rows=rows, seed=2, call=5)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = net.sample(net.torso(x, s), rows=rows, seed=2, call=5)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
