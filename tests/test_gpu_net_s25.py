"""The fused network at the 5x5 matmul tensor (S = TG_NET_WIDE3_S = 25, include/tensor_game_net_s25.h,
FusedAlphaTensor25) on the MI355X, for the three S = 25 configurations of net_s25_ref: the precision bound against the
reference's recorded float64 outputs and the float64 restatement, the sampling rule with given uniforms and with the
internal stream (75 steps: the 19th Philox block is used in part), input dtypes, row subsets and empty batches, the
independence of a row's result from the rows per workgroup R, of games and of slices, guarded outputs, the row mask,
graph capture, self-play through search.actor_prediction and sampled rollouts, and the shared-normalisation decoder
beside the product decoder at S = 9 and 16 in the A/B library."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedAlphaTensor25, SyntheticDemos, TensorGameEnv, ops, rollout, search
from mat_mul_amd._lib import TensorGameError

from guarded_buffers import check_flat, guarded
from net_ref import Ref, dims, make_inputs, make_weights, philox_uniforms, pick
from net_s25_ref import CONFIGS, EE_SLICES, RECORDED, SEEDS_NET, decoder_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
CASES = sorted(CONFIGS)
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_s25_cases.npz"
N = 4       # the fixture's input states (make_golden_net_s25.N), and the batch of most tests
S, J = 25, 1875
KEYS = ("ee", "oo", "zz0", "q", "qq")


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def states(name, B):
    """B = N at a recorded configuration: the fixture's states; otherwise make_inputs'; with their g_action."""
    cfg = CONFIGS[name]
    if B == N and name in RECORDED:
        f = fixture(name)
        return f["xx"], f["ss"], f["g_action"]
    xx, ss = make_inputs(cfg, B, 700 + B)
    ga = np.random.default_rng(800 + B).integers(0, cfg["n_logits"], size=(B, cfg["n_steps"])).astype(np.int8)
    return xx, ss, ga


@functools.lru_cache(maxsize=None)
def host(name, B):
    """The float64 restatement's outputs (ee, oo, zz0, q, qq) for states(name, B); computed once, never modified."""
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, SEEDS_NET[name]), cfg, device=DEV)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.cpu() for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


@functools.lru_cache(maxsize=None)
def setup(name):
    cfg = CONFIGS[name]
    sd = make_weights(cfg, SEEDS_NET[name])
    return cfg, sd, FusedAlphaTensor25.from_state_dict(sd, cfg["n_samples"], device=DEV)


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def close(got, ref, what, e32=None):
    """The project's bound 1e-5 * max(1, max|ref|) (test_gpu_net_s16.close).  e32, where the fixture has it, is the
    reference's own float32 error on the same inputs: printed beside the error."""
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max()
    bound = 1e-5 * max(1.0, np.abs(ref).max())
    print(f"{what}: err {err:.3e}, e32 {'-' if e32 is None else format(e32, '.3e')}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def forward(net, xx, ss, ga, seed):
    """The five checked outputs of one batch, and the sampled tokens and probabilities."""
    ee = net.torso(xx, ss)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = net.fwd_infer(xx, ss, seed=seed)
    return dict(ee=ee, oo=oo, zz0=zz0, q=q, qq=qq), aa, pp


@pytest.mark.parametrize("name", RECORDED)
def test_precision_bound_against_the_float64_reference(name):
    """Measured on the MI355X against the recorded float64 outputs (err / the reference's own float32 error e32 /
    bound), a25: ee 2.4e-6 / 2.0e-6 / 6.7e-5, oo 3.8e-7 / 4.3e-7 / 1.8e-5, zz0 7.1e-7 / 1.3e-6 / 5.7e-5,
    q 3.9e-8 / 4.9e-8 / 1e-5, qq 1.2e-8 / 9.7e-9 / 1e-5; b25: ee 1.1e-6 / 8.9e-7 / 4.4e-5, oo 5.1e-7 / 4.7e-7 / 2.1e-5,
    zz0 1.0e-6 / 1.0e-6 / 5.7e-5, q 3.0e-8 / 2.3e-8 / 1e-5, qq 5.0e-9 / 1.1e-8 / 1e-5.  The fp32 sums over 1875 keys and
    75 positions stay inside 1e-5 * max(1, max|ref|) by a factor of ten and more, at the reference's own float32
    error, so the bound is the project's, unchanged."""
    cfg, sd, net = setup(name)
    f = fixture(name)
    assert f["xx"].shape[0] == N and tuple(f["ee_slices"]) == EE_SLICES
    xx, ss, ga = dev(*states(name, N))
    out, aa, pp = forward(net, xx.float(), ss, ga, 1)
    assert tuple(aa.shape) == (N, cfg["n_samples"], 75) and tuple(pp.shape) == (N, cfg["n_samples"])
    assert tuple(out["ee"].shape) == (N, J, cfg["dim_c"]) and aa.dtype == torch.int64
    for key in KEYS:
        rec, rec32 = f[f"{key}64"], f[f"{key}32"]
        e32 = np.abs(rec32.astype(np.float64) - rec).max()
        got = out[key]
        if key == "ee":  # the fixture keeps slices i = 0, 12, 24 of the first state: rows i*75 .. i*75 + 74
            kept = got[:1].reshape(1, S, 3 * S, -1)[:, list(EE_SLICES)]
            close(kept, rec, f"{name} ee (recorded slices)", e32)
        else:
            close(got[:rec.shape[0]], rec, f"{name} {key} (recorded)", e32)
        close(got, host(name, N)[key].numpy(), f"{name} {key} (restatement)")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_the_restatement_by_batch(name, B):
    cfg, sd, net = setup(name)
    xx, ss, ga = dev(*states(name, B))
    out, aa, pp = forward(net, xx, ss, ga, 2)
    assert tuple(aa.shape) == (B, cfg["n_samples"], 75)
    assert int(aa.min()) >= 0 and int(aa.max()) < cfg["n_logits"] and bool((pp > 0).all())
    for key in KEYS:
        close(out[key], host(name, B)[key].numpy(), f"{name} B={B} {key}")


def host_check(name, sd, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities."""
    cfg = CONFIGS[name]
    ref = Ref(sd, cfg, device=DEV)
    B, k, n = tokens.shape
    ee = host(name, N)["ee"].to(DEV).repeat_interleave(k, 0)
    tok = tokens.to(torch.int64).reshape(B * k, n)
    start = torch.full((B * k, 1), cfg["n_logits"], dtype=torch.long, device=DEV)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).cpu().numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    print(f"{name}: {(~keep).sum()} of {keep.size} draws within 1e-5 of a boundary")
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    np.testing.assert_allclose(pp.cpu().numpy(), p_chosen.prod(-1), rtol=1e-5, atol=0)
    assert (~keep).sum() < 0.01 * keep.size


@pytest.mark.parametrize("name", CASES)
def test_sampling_follows_the_host_rule(name):
    cfg, sd, net = setup(name)
    k, n = cfg["n_samples"], cfg["n_steps"]
    xx, ss, _ = dev(*states(name, N))
    ee = net.torso(xx, ss)
    u = np.random.default_rng(5).random((N, k, n)).astype(np.float32)
    tbuf, tok = guarded((N, k, n), torch.int8)
    pbuf, prb = guarded((N, k), torch.float32)
    qbuf, qv = guarded((N,), torch.float32)
    tokens, pp, _ = ops.net_s25_sample(net.c, net.w, ee, torch.arange(N, device=DEV), k, 0, 0,
                                       uniforms=torch.from_numpy(u).to(DEV), tokens=tok, probs=prb, q=qv)
    for b, what in ((tbuf, "tokens"), (pbuf, "probs"), (qbuf, "q")):
        check_flat(b, what)
    host_check(name, sd, tokens, pp, u.astype(np.float64))
    rows = torch.arange(N, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = net.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)  # steps 0 .. 74: Philox blocks 0 .. 18
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, n)
    assert u.shape == (N, k, 75)
    t2, p2, q2 = net.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    host_check(name, sd, t1, p1, u)


@pytest.mark.parametrize("name", CASES)
def test_int8_frames_row_subsets_and_empty_batches(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = dev(*states(name, 5))
    ee8, eef = net.torso(xx, ss), net.torso(xx.float(), ss)
    assert torch.equal(ee8, eef)
    rows = torch.arange(5, device=DEV, dtype=torch.int64) + 1000
    full = net.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([4, 2, 0], device=DEV)
    part = net.sample(net.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)
    one = net.sample(net.torso(xx[3:4], ss[3:4]), rows=rows[3:4], seed=4, call=2)  # B = 1
    for a, b in zip(full, one):
        assert torch.equal(a[3:4], b)
    ee0 = net.torso(xx[:0], ss[:0])  # B = 0 is a no-op
    assert tuple(ee0.shape) == (0, J, cfg["dim_c"])
    t0, p0, q0 = net.sample(ee0, rows=rows[:0])
    assert tuple(t0.shape) == (0, cfg["n_samples"], 75) and p0.numel() == 0 and q0.numel() == 0
    oo, zz0 = net.logits(xx[:0], ss[:0], torch.zeros((0, 75), dtype=torch.int8, device=DEV))
    assert tuple(oo.shape) == (0, 75, cfg["n_logits"]) and zz0.shape[0] == 0


@pytest.mark.parametrize("name,ks", [("c25", (1, 4, 5, 6)), ("a25", (1, 8)), ("b25", (1, 3, 4))])
def test_a_samples_result_does_not_depend_on_the_rows_per_workgroup(name, ks):
    """The same uniforms for sample s whatever k: the workgroups hold R = decoder_rows(k) samples (c25: 1, 4, 5 and 5 + 1,
    a ragged last chunk; a25: 1 whatever k; b25: 1, 2 + 1 and 2 + 2), and sample s < k comes out bit for bit the same."""
    cfg, sd, net = setup(name)
    assert [decoder_rows(dims(cfg), k) for k in ks] == {"c25": [1, 4, 5, 5], "a25": [1, 1], "b25": [1, 2, 2]}[name]
    B, n = 3, cfg["n_steps"]
    xx, ss, _ = dev(*states(name, 3))
    ee = net.torso(xx, ss)
    u = torch.from_numpy(np.random.default_rng(9).random((B, max(ks), n)).astype(np.float32)).to(DEV)
    runs = {k: net.sample(ee, uniforms=u[:, :k].contiguous(), k=k) for k in ks}
    tw, pw, qw = runs[max(ks)]
    assert len({tuple(r.tolist()) for r in tw[0]}) > 1  # the samples differ from each other
    for k in ks:
        t, p, q = runs[k]
        assert torch.equal(t, tw[:, :k]) and torch.equal(p, pw[:, :k]) and torch.equal(q, qw), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_games_and_slices_are_independent_on_the_device(name):
    """One workgroup per (game, slice i) writes rows i*3S .. i*3S + 3S - 1 of its game: a batch equals its games run one
    by one, nothing is written outside ee, and another game's input changes no row of this one."""
    cfg, sd, net = setup(name)
    B = 5
    xx, ss, _ = dev(*states(name, B))
    buf, out = guarded((B, J, cfg["dim_c"]), torch.float32)
    ee = ops.net_s25_torso(net.c, net.w, xx, ss, out=out)
    check_flat(buf, "ee")
    assert ee.data_ptr() == out.data_ptr() and bool(torch.isfinite(ee).all())
    for g in range(B):
        assert torch.equal(net.torso(xx[g:g + 1], ss[g:g + 1])[0], ee[g]), g
    x2, s2 = xx.clone(), ss.clone()
    x2[2] = torch.roll(x2[2], 1, dims=-1) + 1
    s2[2] += 1.0
    ee2 = net.torso(x2, s2)
    keep = [0, 1, 3, 4]
    assert torch.equal(ee2[keep], ee[keep])
    # every slice of the changed game moves (the scalar reaches every position)
    moved = (ee2[2] != ee[2]).reshape(S, 3 * S * cfg["dim_c"]).any(1)
    assert bool(moved.all())
    # one slice of one grid of the input: frames[t, i] reaches grid 0 slice i, and every slice of grids 1 and 2
    x3 = xx.clone()
    x3[1, :, 7] += 1
    d = (net.torso(x3, ss)[1] != ee[1]).reshape(S, 3, S * cfg["dim_c"]).any(2)
    assert bool(d[7].all()) and bool(d.any(1).all())
    # the decoder: a batch equals its games one by one
    rows = torch.arange(B, device=DEV, dtype=torch.int64) + 50
    full = net.sample(ee, rows=rows, seed=6, call=1)
    for g in (0, 4):
        for a, b in zip(full, net.sample(ee[g:g + 1].contiguous(), rows=rows[g:g + 1], seed=6, call=1)):
            assert torch.equal(a[g:g + 1], b), g


@pytest.mark.parametrize("name", CASES)
def test_masked_rows_keep_their_sentinel(name):
    cfg, sd, net = setup(name)
    B, k, n = 5, cfg["n_samples"], cfg["n_steps"]
    xx, ss, _ = dev(*states(name, B))
    rows = torch.arange(B, device=DEV, dtype=torch.int64) + 7
    flags = torch.tensor([0x81, 0x01, 0xFF, 0x80, 0x00], dtype=torch.uint8, device=DEV)
    need, active = 0x81, [0, 2]
    idle = [1, 3, 4]
    ee_plain = net.torso(xx, ss)
    plain = net.sample(ee_plain, rows=rows, seed=8, call=3)
    ebuf, ee = guarded((B, J, cfg["dim_c"]), torch.float32)
    ee.fill_(-7.5)
    net.torso(xx, ss, out=ee, flags=flags, need=need)
    check_flat(ebuf, "ee")
    assert torch.equal(ee[active], ee_plain[active]) and bool((ee[idle] == -7.5).all())
    bufs = [guarded((B, k, n), torch.int8), guarded((B, k), torch.float32), guarded((B,), torch.float32)]
    tok, prb, qv = (b[1] for b in bufs)
    tok.fill_(-5), prb.fill_(-3.0), qv.fill_(-9.0)
    net.sample(ee_plain, rows=rows, seed=8, call=3, tokens=tok, probs=prb, q=qv, flags=flags, need=need)
    for (b, _), what in zip(bufs, ("tokens", "probs", "q")):
        check_flat(b, what)
    for got, want, sentinel in zip((tok, prb, qv), plain, (-5, -3.0, -9.0)):
        assert torch.equal(got[active], want[active]) and bool((got[idle] == sentinel).all())
    # without given outputs the inactive rows hold zeros
    t0, p0, q0 = net.sample(ee_plain, rows=rows, seed=8, call=3, flags=flags, need=need)
    assert not bool(t0[idle].any()) and not bool(p0[idle].any()) and torch.equal(t0[active], plain[0][active])
    with pytest.raises(TensorGameError, match="need=0 with flags given"):
        net.torso(xx, ss, flags=flags, need=0)
    with pytest.raises(TensorGameError, match="need=0 with flags given"):
        net.sample(ee_plain, rows=rows, flags=flags, need=0)


@pytest.mark.parametrize("name", CASES)
def test_graph_capture_equals_eager(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = dev(*states(name, N))
    x = xx.float()
    rows = torch.arange(N, device=DEV, dtype=torch.int64)
    want = net.fwd_infer(x, ss, seed=2, call=5, rows=rows)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        net.fwd_infer(x, ss, seed=2, call=5, rows=rows)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = net.fwd_infer(x, ss, seed=2, call=5, rows=rows)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def test_the_other_class_and_entries_keep_refusing_s25():
    cfg, sd, net = setup("c25")
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):
        FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)
    xx, ss, _ = dev(*states("c25", 1))
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S"):
        ops.net_torso(net.c, net.w, xx, ss)
    with pytest.raises(TensorGameError, match="tg_net_check"):
        FusedAlphaTensor25.from_state_dict(make_weights(dict(CONFIGS["c25"], dim_3d=4, n_steps=12), 1), 4, device=DEV)


def _rank_one_signed(d):
    """d (S,S,S) integer: a rank-1 tensor u x v x w with u, v, w in {-1, 0, 1} (zero included)."""
    d = d.astype(np.int64)
    if not d.any():
        return True
    if np.abs(d).max() > 1:
        return False
    i, j, k = np.argwhere(d)[0]
    return np.array_equal(d, np.einsum("i,j,k->ijk", d[:, j, k], d[i, :, k], d[i, j, :]))


def test_self_play_search_with_the_fused_network_at_s25():
    cfg, sd, net = setup("a25")
    B, T, k = 4, cfg["dim_t"], cfg["n_samples"]
    assert T == 2
    demos = SyntheticDemos(2, B, 1, S, device=DEV, seed=3)  # rank <= 2 targets
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.reshape(B, S, S, S)
    runs = []
    for masked in (False, False, True):
        forest = search.SearchForest(B, S, T, k=k, max_actions=3, n_sim=2, device=DEV)
        out = search.actor_prediction(net.policy(seed=0, masked=masked), start, max_actions=3, n_sim=2, n_bar=100,
                                      n_logits=3, k=k, forest=forest)
        assert int(forest.status.abs().sum()) == 0
        runs.append([t.cpu() for t in out] + [forest.final_heads().cpu()])
    for other in runs[1:]:  # a second run, and the masked policy, play the same games
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    st, pol, rewards, lengths, final = runs[0]
    assert tuple(st.shape) == (B, 3, T, S, S, S) and tuple(pol.shape) == (B, 3, 3 * S, 3)
    assert tuple(rewards.shape) == (B, 3) and tuple(lengths.shape) == (B,)
    assert bool((lengths >= 1).all()) and bool((lengths <= 3).all())
    st, final = st.numpy(), final.numpy()
    for b in range(B):
        n = int(lengths[b])
        assert np.array_equal(st[b, 0], start[b].cpu().numpy())
        assert not st[b, n:].any()
        for l in range(n):  # the move played at step l: head(l) - head(l + 1) is one signed rank-1 term
            nxt = st[b, l + 1, 0] if l + 1 < n else final[b]
            assert _rank_one_signed(st[b, l, 0].astype(np.int64) - nxt), (b, l)
        assert n == 3 or not final[b].any()  # a game shorter than max_actions ended at the zero tensor


def test_sampled_rollouts_with_the_fused_network_at_s25():
    cfg, sd, net = setup("a25")
    G, T, n, K = 3, cfg["dim_t"], 4, 2
    demos = SyntheticDemos(2, G, 1, S, device=DEV, seed=4)
    start = torch.zeros((G, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.reshape(G, S, S, S)
    scalars = torch.zeros((G, cfg["dim_s"]), device=DEV)
    res = rollout.sample_rollouts(net.rollout_policy(seed=2), start, scalars, n_samples=n, max_actions=K)
    again = rollout.sample_rollouts(net.rollout_policy(seed=2), start, scalars, n_samples=n, max_actions=K)
    assert torch.equal(res.actions, again.actions) and torch.equal(res.frames, again.frames)
    assert tuple(res.actions.shape) == (G * n, K, 3 * S)
    # the recorded tokens replayed by the environment reproduce the final heads, and the statistics follow from them
    env = TensorGameEnv(G * n, S, DEV)
    env.reset(start[:, 0].repeat_interleave(n, 0).contiguous())
    nnz = []
    for step in range(K):
        env.step(res.actions[:, step].contiguous())
        nnz.append(env.nnz().clone().view(G, n))
    assert torch.equal(env.state, res.frames[:, 0])
    assert torch.equal(res.frames[:, 1], _head_before_last(start, res.actions, n, K))
    nnz = torch.stack(nnz).to(torch.int64)  # (K, G, n)
    assert torch.equal(res.best_nnz.to(torch.int64), nnz.amin((0, 2)))
    assert res.lowest_rank.item() == nnz.min().item()
    solved = (nnz == 0).any(2)  # (K, G)
    assert res.num_solved.item() == int(solved.any(0).sum()) and res.num_hits.item() == int(solved.sum())
    groups, tokens, lens = res.solutions()
    assert groups.tolist() == torch.nonzero(solved.any(0)).flatten().tolist()
    for g, tok, L in zip(groups.tolist(), tokens, lens.tolist()):
        one = TensorGameEnv(1, S, DEV)
        one.reset(start[g:g + 1, 0].contiguous())
        for step in range(L):
            one.step(tok[step:step + 1].contiguous())
        assert not bool(one.state.any())


def _head_before_last(start, actions, n, K):
    """The head after K - 1 steps (the second frame of the final rows)."""
    B = actions.shape[0]
    env = TensorGameEnv(B, S, DEV)
    env.reset(start[:, 0].repeat_interleave(n, 0).contiguous())
    for step in range(K - 1):
        env.step(actions[:, step].contiguous())
    return env.state.clone()


# ---- the shared-normalisation decoder beside the product decoder at sizes both run (the A/B library's switch) ----------
AB_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from mat_mul_amd import FusedAlphaTensor, _lib
from net_ref import make_inputs, make_weights
import net_s9_ref, net_s16_ref
assert _lib.AB_VARIANT and "libtensorgame_ab.so" in open("/proc/self/maps").read()
other = np.load(sys.argv[3]) if len(sys.argv) > 3 else None
out = {}
B = 3
for name, cfg in sorted({**net_s9_ref.CONFIGS, **net_s16_ref.CONFIGS}.items()):
    k, n = cfg["n_samples"], cfg["n_steps"]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 7), k, device="cuda:0")
    xx, ss = make_inputs(cfg, B, 77)
    xx, ss = torch.from_numpy(xx).cuda(), torch.from_numpy(ss).cuda()
    rng = np.random.default_rng(78)
    ga = torch.from_numpy(rng.integers(0, cfg["n_logits"], size=(B, n)).astype(np.int8)).cuda()
    u = rng.random((B, k, n)).astype(np.float32)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    tokens, pp, qq = net.sample(net.torso(xx, ss), uniforms=torch.from_numpy(u).cuda())
    out.update({name + "_oo": oo.cpu().numpy(), name + "_zz0": zz0.cpu().numpy(), name + "_q": q.cpu().numpy(),
                name + "_qq": qq.cpu().numpy(), name + "_tokens": tokens.cpu().numpy(), name + "_pp": pp.cpu().numpy(),
                name + "_u": u})
    if other is not None:  # this decoder's logits along the other decoder's tokens, sample by sample
        tok = torch.from_numpy(other[name + "_tokens"]).cuda()
        out[name + "_oo_along"] = np.stack([net.logits(xx, ss, tok[:, s].contiguous())[0].cpu().numpy()
                                            for s in range(k)], 1)
np.savez(sys.argv[2], **out)
print("DECODE_OK")
'''


def test_shared_normalisation_decoder_beside_the_product_decoder_at_s9_and_s16(tmp_path):
    """TG_NET_DEC_SHARED_LN (A/B library only) makes tg_net_sample and tg_net_logits take the decoder of S = 25 at the
    sizes they serve.  Its oo, zz0 and q agree with the product decoder's within the precision rule (the product
    decoder as ref), and with the same uniforms its tokens are those of the host rule on the product decoder's
    probabilities along the same prefix, wherever the draw is at least 1e-5 from a boundary."""
    script = tmp_path / "decode_case.py"
    script.write_text(AB_SCRIPT)
    got = {}
    for tag, extra, more in (("shared", {"TG_NET_DEC_SHARED_LN": "1"}, []),
                             ("product", {}, [str(tmp_path / "shared.npz")])):
        env = {k: v for k, v in os.environ.items() if k != "TG_NET_DEC_SHARED_LN"}
        env.update(TG_LIB_VARIANT="ab", **extra)
        res = subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_path / f"{tag}.npz"), *more], env=env,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "DECODE_OK" in res.stdout, (res.stdout[-1000:], res.stderr[-3000:])
        got[tag] = np.load(tmp_path / f"{tag}.npz")
    names = sorted({f.split("_")[0] for f in got["product"].files})
    assert names == ["a16", "a9", "b16", "b9"]
    differs = False
    for name in names:
        for key in ("oo", "zz0", "q", "qq"):
            a, b = got["shared"][f"{name}_{key}"], got["product"][f"{name}_{key}"]
            assert a.shape == b.shape and np.isfinite(a).all()
            close(torch.from_numpy(a), b, f"{name} {key} (shared against product)")
            differs = differs or not np.array_equal(a, b)
        u = got["shared"][f"{name}_u"].astype(np.float64)
        assert np.array_equal(got["shared"][f"{name}_u"], got["product"][f"{name}_u"])
        oo = torch.from_numpy(got["product"][f"{name}_oo_along"]).double()  # (B, k, n, n_logits)
        want, dist = pick(u, torch.softmax(oo, -1).numpy())
        keep = dist >= 1e-5
        print(f"{name}: {(~keep).sum()} of {keep.size} draws within 1e-5 of a boundary")
        assert np.array_equal(got["shared"][f"{name}_tokens"][keep], want[keep])
        assert (~keep).sum() < 0.01 * keep.size
    assert differs  # the switch took the other decoder: somewhere the bits are not the product's
