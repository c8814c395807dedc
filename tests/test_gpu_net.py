"""The fused network on the MI355X (include/tensor_game_net.h, mat_mul_amd.net), for the three recorded
configurations: the precision bound against the reference's float64 outputs, the sampling rule with given uniforms and
with the internal stream, the distribution, self-consistency, input dtypes and row subsets, the search loop and graph
capture."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, search
from mat_mul_amd._lib import TensorGameError

from net_ref import CONFIGS, Ref, make_weights, philox_uniforms, pick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(CONFIGS)


@pytest.fixture(scope="module")
def cases(golden):
    return golden("net_cases")


@functools.lru_cache(maxsize=None)
def host(name):
    """The float64 restatement's outputs for all 64 fixture states (the fixture records the reference's outputs for the
    first few; test_net_cpu.py checks that the restatement reproduces them): ee, oo, zz0, q, qq."""
    cases = np.load(Path(__file__).resolve().parent / "golden" / "net_cases.npz")
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, int(cases[f"{name}_seed"].item())), cfg)
    ee = ref.torso(cases[f"{name}_xx"], cases[f"{name}_ss"])
    oo, zz0, q = ref.teacher(ee, cases[f"{name}_g_action"])
    return {"ee": ee, "oo": oo, "zz0": zz0, "q": q, "qq": Ref.risk(q)}


def setup(cases, name):
    cfg = CONFIGS[name]
    sd = make_weights(cfg, int(cases[f"{name}_seed"].item()))
    net = FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)
    xx = torch.from_numpy(cases[f"{name}_xx"]).to(DEV)
    ss = torch.from_numpy(cases[f"{name}_ss"]).to(DEV)
    return cfg, sd, net, xx, ss


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max()
    assert err <= 1e-5 * max(1.0, np.abs(ref).max()), (what, err)


@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_float64_reference(cases, name):
    """Against the reference's own float64 outputs where the fixture records them, and against the float64
    restatement on all 64 states."""
    cfg, sd, net, xx, ss = setup(cases, name)
    h = host(name)
    g = torch.from_numpy(cases[f"{name}_g_action"]).to(DEV)
    ee = net.torso(xx.float(), ss)
    oo, zz0, q = net.logits(xx, ss, g, with_q=True)
    aa, pp, qq = net.fwd_infer(xx.float(), ss, seed=1)
    assert aa.dtype == torch.int64 and tuple(aa.shape) == (64, cfg["n_samples"], cfg["n_steps"])
    assert pp.dtype == torch.float32 and tuple(pp.shape) == (64, cfg["n_samples"])
    assert qq.dtype == torch.float32 and tuple(qq.shape) == (64,)
    for got, key in ((ee, "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        rec = cases[f"{name}_{key}64"]
        close(got[:rec.shape[0]], rec, key)
        close(got, h[key].numpy(), key)


def host_check(cases, name, sd, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities (the device's
    own prefix as the input).  Returns the number of excluded draws."""
    cfg = CONFIGS[name]
    ref = Ref(sd, cfg)
    B, k, n = tokens.shape
    ee = host(name)["ee"].repeat_interleave(k, 0)
    tok = torch.from_numpy(tokens.cpu().numpy().astype(np.int64)).reshape(B * k, n)
    start = torch.full((B * k, 1), cfg["n_logits"], dtype=torch.long)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    np.testing.assert_allclose(pp.cpu().numpy(), p_chosen.prod(-1), rtol=1e-5, atol=0)
    return int((~keep).sum()), keep.size


@pytest.mark.parametrize("name", CASES)
def test_given_uniforms_follow_the_host_rule(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    k, n = cfg["n_samples"], cfg["n_steps"]
    u = np.random.default_rng(5).random((64, k, n)).astype(np.float32)
    ee = net.torso(xx, ss)
    tokens, pp, _ = net.sample(ee, uniforms=torch.from_numpy(u).to(DEV))
    excluded, total = host_check(cases, name, sd, tokens, pp, u.astype(np.float64))
    assert excluded < 0.01 * total


@pytest.mark.parametrize("name", CASES)
def test_internal_stream_is_the_host_philox_rule(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    k, n = cfg["n_samples"], cfg["n_steps"]
    rows = torch.arange(64, device=DEV, dtype=torch.int64) * 977 + 3
    ee = net.torso(xx, ss)
    t1, p1, q1 = net.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, n)
    t2, p2, q2 = net.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    excluded, total = host_check(cases, name, sd, t1, p1, u)
    assert excluded < 0.01 * total


@pytest.mark.parametrize("name", CASES)
def test_first_step_distribution(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    ee = net.torso(xx[:1], ss[:1]).repeat(8192, 1, 1).contiguous()
    tokens, _, _ = net.sample(ee, seed=9, call=0, k=8)
    first = tokens[:, :, 0].reshape(-1).long().cpu()
    counts = torch.bincount(first, minlength=cfg["n_logits"]).numpy().astype(np.float64)
    ref = Ref(sd, cfg)
    oo, _ = ref.decode(host(name)["ee"][:1],
                       torch.full((1, 1), cfg["n_logits"], dtype=torch.long))
    p = torch.softmax(oo[0, 0], -1).numpy()
    expect = p * counts.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    from scipy.stats import chi2 as chi2_dist
    assert chi2_dist.sf(chi2, cfg["n_logits"] - 1) > 1e-4, (counts, expect)


@pytest.mark.parametrize("name", CASES)
def test_logits_of_the_sampled_actions_reproduce_pp(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    k = cfg["n_samples"]
    aa, pp, _ = net.fwd_infer(xx, ss, seed=3)
    oo, _ = net.logits(xx.repeat_interleave(k, 0), ss.repeat_interleave(k, 0), aa.reshape(64 * k, -1))
    logp = torch.log_softmax(oo.double(), -1).gather(-1, aa.reshape(64 * k, -1, 1)).sum((1, 2))
    np.testing.assert_allclose(torch.exp(logp).cpu().numpy(), pp.reshape(-1).double().cpu().numpy(), rtol=1e-5)


@pytest.mark.parametrize("name", CASES)
def test_int8_frames_and_row_subsets(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    ee8, eef = net.torso(xx, ss), net.torso(xx.float(), ss)
    assert torch.equal(ee8, eef)
    rows = torch.arange(64, device=DEV, dtype=torch.int64) + 1000
    full = net.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([63, 5, 17, 0, 40], device=DEV)
    part = net.sample(net.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)


def test_self_play_search_with_the_fused_network(cases):
    cfg, sd, net, _, _ = setup(cases, "a")
    B, S, T, k = 4096, 4, cfg["dim_t"], cfg["n_samples"]
    rng = np.random.default_rng(0)
    start = torch.from_numpy(rng.integers(-1, 2, size=(B, T, S, S, S)).astype(np.int8)).to(DEV)
    runs = []
    for _ in range(2):
        forest = search.SearchForest(B, S, T, k=k, max_actions=4, n_sim=16, device=DEV)
        out = search.actor_prediction(net.policy(seed=7), start, 4, n_sim=16, n_bar=100, n_logits=3, k=k,
                                      forest=forest)
        assert int(forest.status.abs().sum()) == 0
        runs.append([t.cpu() for t in out])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    # a retried game asks again with the same frames and game index: the next call draws other candidates
    pol = net.policy(seed=7)
    frames = start[:256].float()
    sc = torch.zeros((256, 1), device=DEV)
    games = torch.arange(256, device=DEV)
    t1, _, q1 = pol(frames, sc, games)
    t2, _, q2 = pol(frames, sc, games)
    assert torch.equal(q1, q2)
    assert (t1 != t2).flatten(1).any(1).float().mean() > 0.9


@pytest.mark.parametrize("name", CASES)
def test_graph_capture_equals_eager(cases, name):
    cfg, sd, net, xx, ss = setup(cases, name)
    x, s = xx.float().clone(), ss.clone()
    rows = torch.arange(64, device=DEV, dtype=torch.int64)
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


def test_unsupported_configuration_is_refused_on_the_device_path():
    cfg = dict(CONFIGS["a"], dim_3d=6, n_steps=18)
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):
        FusedAlphaTensor.from_state_dict(make_weights(cfg, 0), 8, device=DEV)
