"""tg_replay_add / tg_replay_items, ops.replay_add / replay_items, replay.GameBuffer / TensorGameData on the MI355X:
the device reproduces every __getitem__ the reference's PlayedGamesDataset and TensorGameDataset recorded
(tests/golden/replay_cases.npz), its synthetic rows are byte-equal to tg_demo_items, the ring, the best-game rule and the
bad rows follow the host restatement (tests/replay_ref.py), the resampling keeps the reference's rules, an epoch visits
every index once, captured calls equal eager ones, and self-play games flow from the search into training batches."""
import numpy as np
import pytest
import torch

import replay_ref as RR
import ring_cases as RC
from guarded_buffers import check_flat, guarded
from mat_mul_amd import GameBuffer, SyntheticDemos, TensorGameData, ops, search

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.int8, torch.float32, torch.float16, torch.bfloat16]


def i8(frames):
    f = frames.detach()
    return (f if f.dtype == torch.int8 else f.float()).cpu().numpy().astype(np.int8)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def check_items(got, frames, scalars, actions, rewards, what):
    f, sc, ac, rw = got
    assert np.array_equal(i8(f), frames), what
    assert np.array_equal(sc.cpu().numpy().reshape(-1), np.asarray(scalars, np.float32).reshape(-1)), what
    assert np.array_equal(ac.cpu().numpy(), np.asarray(actions).astype(np.int8)), what
    assert np.array_equal(rw.cpu().numpy().reshape(-1), np.asarray(rewards, np.float32).reshape(-1)), what


# ---- fixture parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S4_T2", "S16_T1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ring_reproduces_the_reference(golden, name, dtype):
    g = golden("replay_cases")
    st, po, rw, ln = (g[f"ring_{name}_{k}"] for k in ("states", "policy", "rewards", "lengths"))
    A, L, T, S = st.shape[0], st.shape[1], st.shape[2], st.shape[3]
    buf = GameBuffer(3, L, T, S, DEV)
    for a in range(A):  # across calls: one game per call
        buf.add_games(dev(st[a:a + 1]), dev(po[a:a + 1]), dev(rw[a:a + 1]), dev(ln[a:a + 1]))
        n = len(buf)
        snap = [g[f"ring_{name}_snap{a}_{k}"] for k in ("frames", "scalar", "action", "reward")]
        assert n == snap[0].shape[0]
        check_items(buf.items(torch.arange(n, device=DEV), dtype=dtype), *snap, (name, a))
    assert buf.games_added() == A and int(buf.status[0]) == 0
    once = GameBuffer(3, L, T, S, DEV)  # within one call: B > C
    once.add_games(dev(st), dev(po), dev(rw), dev(ln))
    for x, y in zip(once.items(torch.arange(len(once), device=DEV), dtype=dtype),
                    buf.items(torch.arange(len(buf), device=DEV), dtype=dtype)):
        assert torch.equal(x, y)
    state, scalar, action, reward = buf[len(buf) - 1]
    assert state.shape == (T, S, S, S) and scalar.shape == (1,) and action.shape == (3 * S,) and reward.shape == (1,)


def mix_data(g, seed=0):
    data = TensorGameData(dev(g["mix_tokens"], torch.int8), dev(g["mix_targets"], torch.int8), 40, 0.9, dim_t=2,
                          max_actions=4, seed=seed)
    st, po, rw, ln = (g[f"mix_{k}"] for k in ("states", "policy", "rewards", "lengths"))
    data.played.add_games(dev(st[:3]), dev(po[:3]), dev(rw[:3]), dev(ln[:3]))
    data.best.add_games(dev(st[3:]), dev(po[3:]), dev(rw[3:]), dev(ln[3:]))  # add_best_game of that one game
    return data


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixture_reproduces_the_reference(golden, k, dtype):
    g = golden("replay_cases")
    data = mix_data(g)
    data.set_fractions(*g[f"mix_{k}_fract"].tolist())
    data.set_indexes(g[f"mix_{k}_is_synth"], g[f"mix_{k}_index_synth"],
                     g[f"mix_{k}_index_played"] if g[f"mix_{k}_has_played"] else None,
                     g[f"mix_{k}_index_best"] if g[f"mix_{k}_has_best"] else None)
    got = data.items(torch.arange(40, device=DEV), dtype=dtype)
    check_items(got, g[f"mix_{k}_frames"].astype(np.int8), g[f"mix_{k}_scalar"], g[f"mix_{k}_action"],
                g[f"mix_{k}_reward"], k)
    assert int(data.status[0]) == 0
    state, scalar, action, reward = data[7]
    assert np.array_equal(state.cpu().numpy(), g[f"mix_{k}_frames"][7]) and float(scalar[0]) == g[f"mix_{k}_scalar"][7]


# ---- synthetic rows == tg_demo_items ----------------------------------------------------------------------------------
def random_games(rng, B, L, T, S, n_logits=3, short=True):
    st = rng.integers(-3, 4, size=(B, L, T, S, S, S)).astype(np.int8)
    po = rng.random((B, L, 3 * S, n_logits)).astype(np.float32)
    rw = -rng.integers(1, 9, size=(B, L)).astype(np.float32)
    ln = rng.integers(1 if short else L, L + 1, size=B).astype(np.int64)
    return st, po, rw, ln


@pytest.mark.parametrize("S, R, T, basis", [(3, 6, 1, False), (3, 6, 2, False), (4, 7, 1, False), (4, 7, 2, False),
                                            (5, 8, 2, False), (16, 12, 1, False), (16, 12, 2, True),
                                            (25, 10, 1, False), (25, 10, 2, False), (4, 300, 2, False)])
def test_synthetic_rows_equal_demo_items(S, R, T, basis):
    rng = np.random.default_rng(S * 100 + R + T)
    demos = SyntheticDemos.generate(24, S, R, DEV, dim_t=T, seed=S + T, random_basis=basis)
    L = 5
    played = GameBuffer(8, L, T, S, DEV)
    st, po, rw, ln = random_games(rng, 6, L, T, S)
    played.add_games(dev(st), dev(po), dev(rw), dev(ln))
    ring = RR.Ring(8, L)
    ring.add(st, po, rw, ln)
    N = 512
    n_synth, n_played = 24 * R, int(ln.sum())
    kind = rng.integers(0, 2, size=N).astype(np.uint8)
    src = np.where(kind == 0, rng.integers(0, n_synth, size=N), rng.integers(0, n_played, size=N)).astype(np.int64)
    idx = rng.permutation(N).astype(np.int64)
    for dtype in DTYPES:
        ovf = torch.zeros((N,), dtype=torch.uint8, device=DEV)
        got = ops.replay_items(dev(idx), T, S, DEV, tokens=demos.action_seq, targets=demos.target_tensor, played=played,
                               kind=dev(kind), src=dev(src), dtype=dtype, overflow=ovf)
        syn = kind[idx] == 0
        ovf_d = torch.zeros((N,), dtype=torch.uint8, device=DEV)
        want = ops.demo_items(demos.action_seq, demos.target_tensor, dev(src[idx]), T, dtype=dtype, overflow=ovf_d)
        sel = dev(np.nonzero(syn)[0])
        for x, y in zip(got, want):  # synthetic rows: byte-equal
            assert torch.equal(x[sel].contiguous().view(torch.uint8), y[sel].contiguous().view(torch.uint8))
        assert torch.equal(ovf[sel], ovf_d[sel])
        pl = np.nonzero(~syn)[0]  # played rows: the ring's items
        f, sc, ac, rr = (t.cpu() for t in got)
        for n in pl[:64].tolist():
            fr, s, a, r = ring.getitem(int(src[idx[n]]))
            assert np.array_equal(i8(f[n:n + 1])[0], fr) and float(sc[n, 0]) == s
            assert np.array_equal(ac[n].numpy(), a) and float(rr[n, 0]) == r
        assert not ovf[dev(pl)].any()


# ---- ring, best rule, bad rows -----------------------------------------------------------------------------------------
def buffer_items(buf):
    n = len(buf)
    f, sc, ac, rw = buf.items(torch.arange(n, device=DEV), dtype=torch.int8)
    return i8(f), sc.cpu().numpy()[:, 0], ac.cpu().numpy(), rw.cpu().numpy()[:, 0]


def ring_items(ring):
    items = [ring.getitem(i) for i in range(len(ring))]
    return (np.stack([x[0] for x in items]), np.array([x[1] for x in items]), np.stack([x[2] for x in items]),
            np.array([x[3] for x in items]))


@pytest.mark.parametrize("C, B, calls", [(5, 13, 1), (7, 4, 5), (64, 300, 2), (1, 3, 3)])
def test_ring_wraps_and_skips_like_the_restatement(C, B, calls):
    rng = np.random.default_rng(C * 7 + B)
    L, T, S = 6, 2, 4
    buf, ring = GameBuffer(C, L, T, S, DEV), RR.Ring(C, L)
    bits = 0
    for _ in range(calls):
        st, po, rw, ln = random_games(rng, B, L, T, S, n_logits=5)
        ln[rng.random(B) < 0.2] = 0          # length 0: skipped
        ln[0] = 0
        ln[rng.random(B) < 0.1] = L + 1      # longer than a slot: skipped
        po[rng.random(po.shape[:3]) < 0.1] = 0.5  # ties
        bits |= ring.add(st, po, rw, ln)
        buf.add_games(dev(st), dev(po), dev(rw), dev(ln))
        assert len(buf) == len(ring) and buf.games_added() == ring.added
        if len(ring):
            for x, y in zip(buffer_items(buf), ring_items(ring)):
                assert np.array_equal(x, y)
    assert int(buf.status[0]) == bits == 1
    off = buf.offset.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(buf.length.cpu().numpy())]))


@pytest.mark.parametrize("C", RC.EDGE_C)
@pytest.mark.parametrize("N", RC.EDGE_N)
def test_add_at_the_plan_chunk_and_slot_range_edges(N, C):
    RC.check_edges("add", N, C, DEV)


def test_best_rule_follows_act_step(golden):
    g = golden("replay_cases")
    L, T, S = 4, 1, 4
    buf, ring = GameBuffer(2, L, T, S, DEV), RR.Ring(2, L)
    rng = np.random.default_rng(3)
    for i in range(4):
        rw, ln = g[f"best_{i}_rewards"], g[f"best_{i}_lengths"]
        st, po, _, _ = random_games(rng, len(ln), L, T, S)
        buf.add_best(dev(st), dev(po), dev(rw), dev(ln))
        ring.add(st, po, rw, ln, select=True)
        assert buf.games_added() == ring.added
        if len(ring):
            for x, y in zip(buffer_items(buf), ring_items(ring)):
                assert np.array_equal(x, y)
    assert ring.added == 3 and int(buf.status[0]) == 0
    st, po, rw, ln = random_games(rng, 3, L, T, S)
    ln[1] = 0
    buf.add_best(dev(st), dev(po), dev(rw), dev(ln))
    assert int(buf.status[0]) == 1


def test_bad_rows_are_zero_with_status_and_stay_in_bounds():
    rng = np.random.default_rng(11)
    S, T, L = 4, 2, 4
    demos = SyntheticDemos(L, 8, T, S, DEV, seed=2)
    played = GameBuffer(4, L, T, S, DEV)
    st, po, rw, ln = random_games(rng, 3, L, T, S, short=False)
    played.add_games(dev(st), dev(po), dev(rw), dev(ln))
    n_played = int(ln.sum())
    kind = np.array([0, 1, 2, 5, 0, 1, 1, 0], np.uint8)
    src = np.array([3, 2, 0, 0, 8 * L, n_played, -1, -5], np.int64)
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 1, 0], np.int64)  # 8 and -1: outside the table
    N = len(idx)
    want_bad = np.array([0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], bool)  # best is absent: its row is bad too
    for dtype in DTYPES:
        bufs = [guarded((N, T, S, S, S), dtype), guarded((N, 1), torch.float32), guarded((N, 3 * S), torch.int8),
                guarded((N, 1), torch.float32), guarded((N,), torch.uint8), guarded((1,), torch.uint32)]
        (fb, f), (sb, sc), (ab, ac), (rb, rr), (ob, ov), (stb, status) = bufs
        ov.zero_()
        status.zero_()
        ops.replay_items(dev(idx), T, S, DEV, tokens=demos.action_seq, targets=demos.target_tensor, played=played,
                         kind=dev(kind), src=dev(src), dtype=dtype, out=f, scalars=sc, actions=ac, rewards=rr,
                         overflow=ov, status=status)
        torch.cuda.synchronize()
        for b, what in zip((fb, sb, ab, rb, ob, stb), ("frames", "scalars", "actions", "rewards", "overflow", "status")):
            check_flat(b, what)
        assert int(status[0]) == 1
        bad = dev(np.nonzero(want_bad)[0])
        assert not f[bad].any() and not sc[bad].any() and not ac[bad].any() and not rr[bad].any()
        good = demos.items(dev(np.array([3], np.int64)), dtype=dtype)
        assert torch.equal(f[0], good[0][0]) and torch.equal(f[11], good[0][0])
        assert float(sc[1, 0]) == 2.0 and float(sc[10, 0]) == 2.0  # played move index 2 of the first game
    # direct mode: outside the buffer gives zero items too
    f, sc, ac, rr = played.items(torch.tensor([0, n_played, -3], device=DEV))
    assert f[0].any() and not f[1:].any() and int(played.status[0]) == 1


# ---- resampling and epochs -----------------------------------------------------------------------------------------
def big_data(seed, len_data=300, played_games=6, best_games=2, L=6):
    demos = SyntheticDemos(L, 64, 2, 4, DEV, seed=9)
    data = TensorGameData.from_demos(demos, len_data, 0.7, seed=seed, played_capacity=64, best_capacity=8)
    rng = np.random.default_rng(5)
    st, po, rw, ln = random_games(rng, played_games + best_games, L, 2, 4, short=False)
    data.played.add_games(dev(st[:played_games]), dev(po[:played_games]), dev(rw[:played_games]),
                          dev(ln[:played_games]))
    data.best.add_games(dev(st[played_games:]), dev(po[played_games:]), dev(rw[played_games:]), dev(ln[played_games:]))
    return data


def test_resample_statistics_follow_the_reference_rules():
    empty = TensorGameData.from_demos(SyntheticDemos(6, 64, 2, 4, DEV, seed=9), 300, 0.7, seed=1)
    before = empty.index_synth.clone()
    empty.resample_buffer_indexes()  # the played buffer is empty: the epoch stays all synthetic
    assert torch.equal(empty.index_synth, before) and bool(empty.is_synth.all())
    assert len(set(before.tolist())) == 300 and int(before.max()) < 64 * 6
    with pytest.raises(ValueError):
        TensorGameData.from_demos(SyntheticDemos(6, 10, 2, 4, DEV, seed=9), 61, 0.7)

    data = big_data(1)
    n_played, n_best = len(data.played), len(data.best)
    data.resample_buffer_indexes()
    s = data.is_synth.cpu().numpy()
    isyn, ipl = data.index_synth.cpu().numpy(), data.index_played.cpu().numpy()
    assert len(isyn) == s.sum() and len(set(isyn.tolist())) == len(isyn)        # distinct synthetic draws
    assert len(ipl) == 300 - s.sum() and ipl.max() < n_played
    assert len(ipl) > n_played >= len(set(ipl.tolist()))                        # more than held: with replacement
    kind = data.kind.cpu().numpy()
    assert np.array_equal(kind == 0, s) and set(kind[~s].tolist()) == {1}
    data.set_fractions(0.95, 0.0)  # few played items: drawn without replacement
    data.resample_buffer_indexes()
    ipl = data.index_played.cpu().numpy()
    assert len(ipl) <= n_played and len(set(ipl.tolist())) == len(ipl)
    data.set_fractions(0.5, 0.2)   # the reference's split: len_played = int(0.3) * len_data = 0, all to best
    data.resample_buffer_indexes()
    s = data.is_synth.cpu().numpy()
    kind = data.kind.cpu().numpy()
    assert data.index_played.numel() == 0 and data.index_best.numel() == 300 - s.sum() > n_best
    assert set(kind[~s].tolist()) == {2} and int(data.index_best.max()) < n_best
    # deterministic per seed, different across seeds
    a, b, c = big_data(4), big_data(4), big_data(5)
    for d in (a, b, c):
        d.resample_buffer_indexes()
    assert torch.equal(a.kind, b.kind) and torch.equal(a.src, b.src)
    assert not (torch.equal(a.kind, c.kind) and torch.equal(a.src, c.src))


def test_an_epoch_visits_every_index_once():
    data = big_data(2, len_data=250)
    data.resample_buffer_indexes()
    gen = torch.Generator(device=DEV).manual_seed(9)
    batches = list(data.batches(64, generator=gen))
    assert [b[0].shape[0] for b in batches] == [64, 64, 64, 58]
    order = torch.randperm(250, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV)
    assert sorted(order.tolist()) == list(range(250))
    want = data.items(order)
    for j, x in enumerate(torch.cat([b[j] for b in batches]) for j in range(4)):
        assert torch.equal(x, want[j])
    assert [b[0].shape[0] for b in data.batches(64, drop_last=True)] == [64] * 3
    plain = list(data.batches(100, shuffle=False))
    assert torch.equal(torch.cat([b[0] for b in plain]), data.items(torch.arange(250, device=DEV))[0])


# ---- graph capture -------------------------------------------------------------------------------------------------
def test_captured_add_and_items_equal_eager():
    rng = np.random.default_rng(21)
    L, T, S, B = 6, 2, 4, 40
    st, po, rw, ln = (dev(x) for x in random_games(rng, B, L, T, S))
    bufs = [GameBuffer(32, L, T, S, DEV) for _ in range(2)]
    for b in bufs:
        b.add_games(st, po, rw, ln)  # warm-up, both the same
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        bufs[0].add_games(st[:3], po[:3], rw[:3], ln[:3])
        bufs[1].add_games(st[:3], po[:3], rw[:3], ln[:3])
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # capture runs nothing
        bufs[0].add_games(st[5:], po[5:], rw[5:], ln[5:])
    graph.replay()
    bufs[1].add_games(st[5:], po[5:], rw[5:], ln[5:])
    torch.cuda.synchronize()
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        assert torch.equal(getattr(bufs[0], name), getattr(bufs[1], name)), name

    data = big_data(3)
    data.resample_buffer_indexes()
    N = 128
    idx = torch.from_numpy(rng.integers(0, 300, size=N)).to(DEV)
    out = [torch.empty((N, 2, 4, 4, 4), dtype=torch.bfloat16, device=DEV), torch.empty((N, 1), device=DEV),
           torch.empty((N, 12), dtype=torch.int8, device=DEV), torch.empty((N, 1), device=DEV)]

    def run():
        ops.replay_items(idx, 2, 4, DEV, tokens=data.tokens, targets=data.targets, played=data.played, best=data.best,
                         kind=data.kind, src=data.src, dtype=torch.bfloat16, out=out[0], scalars=out[1],
                         actions=out[2], rewards=out[3])

    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        run()
    for seed in (1, 2):
        idx.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 300, size=N)))
        g2.replay()
        torch.cuda.synchronize()
        want = data.items(idx.clone(), dtype=torch.bfloat16)
        assert all(torch.equal(x, y) for x, y in zip(out, want))


# ---- end to end: search -> buffers -> batches -------------------------------------------------------------------------
def test_self_play_games_reach_the_training_batches():
    S, T, B, max_actions, n_sim, n_logits = 4, 2, 48, 5, 8, 3
    rng = np.random.default_rng(30)
    start = np.zeros((B, T, S, S, S), np.int8)
    start[:, 0] = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(B, S, S, S))
    pool = torch.from_numpy(rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2], size=(16, 3 * S)).astype(np.int8))
    forest = search.SearchForest(B, S, T, k=8, max_actions=max_actions, n_sim=n_sim, device=DEV)
    pol = search.keyed_policy(forest, pool, seed=3)
    states, policy, rewards, lengths = search.actor_prediction(pol, dev(start), max_actions, n_sim, 4, n_logits,
                                                               forest=forest)
    demos = SyntheticDemos(max_actions, 32, T, S, DEV, seed=1)
    data = TensorGameData.from_demos(demos, 120, 0.5, seed=2)
    data.add_act_step(states, policy, rewards, lengths)
    data.resample_buffer_indexes()
    gen = torch.Generator(device=DEV).manual_seed(4)
    batches = list(data.batches(32, generator=gen))
    order = torch.randperm(120, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV).cpu().numpy()
    kind, src = data.kind.cpu().numpy(), data.src.cpu().numpy()
    ln = lengths.cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(ln)])  # B < capacity: slot g holds game g (all games have moves)
    st_h, tok_h = forest.states().cpu().numpy(), policy.argmax(-1).to(torch.int8).cpu().numpy()
    rw_h = rewards.float().cpu().numpy()
    f, sc, ac, rr = (torch.cat([b[j] for b in batches]).cpu() for j in range(4))
    checked = 0
    for n, x in enumerate(order):
        if kind[x] != 1:
            continue
        gm = int(np.searchsorted(starts, src[x], side="right") - 1)
        m = int(src[x] - starts[gm])
        assert np.array_equal(i8(f[n:n + 1])[0], st_h[gm, m]) and float(sc[n, 0]) == m
        assert np.array_equal(ac[n].numpy(), tok_h[gm, m]) and float(rr[n, 0]) == rw_h[gm, m]
        checked += 1
    assert checked > 20 and (ln > 0).all()
    assert data.best.games_added() == 1 and data.played.games_added() == B
