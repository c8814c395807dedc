"""GPU checks of the batched search (include/tensor_game_search.h, mat_mul_amd.search).

* every game the reference's own actor_prediction played (tests/golden/search_games.npz), replayed on the device with a
  policy that answers from the fixture's call table (a miss fails): states, lengths, rewards, the roots' Q/N and the
  chosen indices bit-exact, the improved policy within 4 ulp (device and host pow/log may differ in the last bit);
* at scale, with the device stand-in ``search.keyed_policy``, against the host restatement (tests/search_ref.py) on
  game 0, the last game and 62 random games;
* edge cases: a terminal leaf, a forced cycle (status bit 1), a full pool (status bit 0), tokens >= n_logits (bit 2),
  k = 1 and k = 64, guarded output buffers; one simulation captured in a graph equals eager; PUCT with a prior."""
import numpy as np
import pytest
import torch

from mat_mul_amd import ops, search
from guarded_buffers import check_flat, guarded
import search_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["S4_T1", "S4_T2", "S4_T2_lowrank", "S3_T1", "S5_T2", "S16_T1"]


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def table_policy(g, case, forest):
    """Answers from the fixture's fwd_infer calls by (head bytes, attempt) for the games that need an expansion; any
    miss raises.  Rows of other games get zeros."""
    table = {}
    for head, att, scal, tok, q in zip(g[f"{case}_call_head"], g[f"{case}_call_attempt"], g[f"{case}_call_scalar"],
                                       g[f"{case}_call_tokens"], g[f"{case}_call_q"]):
        table[(head.tobytes(), int(att))] = (tok, np.float32(q), float(scal))
    used = set()

    def policy(frames, scalars, games):
        rows = games.cpu().numpy()
        need = ((forest.flags[games] & (search.EXPAND | search.PENDING)) == (search.EXPAND | search.PENDING)).cpu().numpy()
        att = forest.attempt[games].cpu().numpy()
        heads = frames[:, 0].to(torch.int8).cpu().numpy()
        sc = scalars[:, 0].cpu().numpy()
        tok = np.zeros((len(rows), forest.k, 3 * forest.S), np.int8)
        q = np.zeros(len(rows), np.float32)
        for i in range(len(rows)):
            if need[i]:
                key = (heads[i].tobytes(), int(att[i]))
                assert key in table, f"{case}: game {rows[i]} asked about a head/attempt the reference never saw"
                tok[i], q[i], s = table[key]
                assert s == float(sc[i]), (case, rows[i], s, sc[i])
                used.add(key)
        return torch.from_numpy(tok).to(DEV), None, torch.from_numpy(q).to(DEV)

    policy.used, policy.table = used, table
    return policy


@pytest.mark.parametrize("case", CASES)
def test_reference_games_on_device(golden, case):
    g = golden("search_games")
    S, T, k, n_sim, max_actions, n_bar, n_logits, horizon, games, _ = (int(x) for x in g[f"{case}_meta"])
    forest = search.SearchForest(games, S, T, k=k, max_actions=max_actions, n_sim=n_sim, horizon=horizon, device=DEV)
    pol = table_policy(g, case, forest)
    start = torch.from_numpy(g[f"{case}_start"]).to(DEV)
    states, policy, rewards, lengths = search.actor_prediction(pol, start, max_actions, n_sim, n_bar, n_logits,
                                                               horizon=horizon, k=k, forest=forest)
    assert pol.used == set(pol.table)  # every call the reference made was made here too
    assert np.array_equal(lengths.cpu().numpy(), g[f"{case}_lengths"])
    assert np.array_equal(states.cpu().numpy(), g[f"{case}_states"])
    assert np.array_equal(rewards.cpu().numpy(), g[f"{case}_rewards"])
    n, q, nc, choice = (t.cpu().numpy() for t in forest.root_stats())
    assert np.array_equal(nc, g[f"{case}_root_nc"]) and np.array_equal(choice, g[f"{case}_choice"])
    assert np.array_equal(n.view(np.int32), g[f"{case}_root_n"].view(np.int32))
    assert np.array_equal(q.view(np.int32), g[f"{case}_root_q"].view(np.int32))
    assert int(ulp_diff(policy.cpu().numpy(), g[f"{case}_policy"]).max()) <= 4
    assert not forest.status.any() and not forest.overflow.any()


def random_starts(rng, B, T, S):
    st = np.zeros((B, T, S, S, S), np.int8)
    st[:, 0] = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(B, S, S, S))
    return st


def random_pool(rng, P, S):
    return rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2], size=(P, 3 * S)).astype(np.int8)


def check_against_restatement(forest, start, pool, seed, n_sim, n_bar, n_logits, sample, out):
    states, policy, rewards, lengths = (t.cpu().numpy() for t in out)
    n, q, nc, choice = (t.cpu().numpy() for t in forest.root_stats())
    fn = R.keyed_policy(pool, forest.k, seed=seed)
    for gi in sample:
        r = R.play(fn, start[gi], forest.max_actions, n_sim, n_bar, n_logits, horizon=forest.horizon,
                   max_depth=forest.max_depth)
        L = r["length"]
        assert L == lengths[gi], gi
        assert np.array_equal(states[gi, :L], r["states"]) and not states[gi, L:].any(), gi
        assert np.array_equal(rewards[gi, :L], r["rewards"]), gi
        assert np.array_equal(choice[gi, :L], r["choice"]), gi
        for m in range(L):
            assert nc[gi, m] == len(r["root_N"][m])
            assert np.array_equal(n[gi, m, :nc[gi, m]].view(np.int32), r["root_N"][m].view(np.int32)), (gi, m)
            assert np.array_equal(q[gi, m, :nc[gi, m]].view(np.int32), r["root_Q"][m].view(np.int32)), (gi, m)
        assert int(ulp_diff(policy[gi, :L], r["policy"]).max()) <= 4, gi


@pytest.mark.parametrize("S, B, T, n_sim, max_actions, k", [(4, 4096, 2, 16, 6, 8), (16, 256, 2, 8, 4, 8),
                                                            (25, 64, 1, 8, 4, 8), (4, 64, 1, 8, 6, 1),
                                                            (4, 64, 2, 8, 6, 64)])
def test_keyed_policy_at_scale(S, B, T, n_sim, max_actions, k):
    rng = np.random.default_rng(S * 1000 + B + k)
    start = random_starts(rng, B, T, S)
    pool = random_pool(rng, 24, S)
    seed, n_bar, n_logits = 7, 4, 3
    forest = search.SearchForest(B, S, T, k=k, max_actions=max_actions, n_sim=n_sim, device=DEV)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    out = search.actor_prediction(pol, torch.from_numpy(start).to(DEV), max_actions, n_sim, n_bar, n_logits, k=k,
                                  forest=forest)
    assert not forest.status.any() and not forest.overflow.any()
    sample = sorted({0, B - 1} | set(rng.choice(B, size=min(B, 62), replace=False).tolist()))
    check_against_restatement(forest, start, pool, seed, n_sim, n_bar, n_logits, sample, out)


def simulate(forest, pol, prior_fn=None, max_retries=64):
    """select + commit for every game, asking again for the games whose candidates were all dropped."""
    frames, scalars = forest.select()
    games = torch.arange(forest.B, device=DEV)
    mask = None
    for _ in range(max_retries):
        tok, _, q = pol(frames, scalars, games)
        forest.commit(tok, q, prior=None if prior_fn is None else prior_fn(games), mask=mask)
        mask = ((forest.flags & search.RETRY) != 0).to(torch.uint8)
        if not mask.any():
            return frames, scalars
    raise AssertionError("retries did not end")


def fixed_policy(forest, tokens, q):
    """The same candidates and q for every leaf (device tensors)."""
    tok = torch.from_numpy(np.asarray(tokens, np.int8)).to(DEV)

    def policy(frames, scalars, games):
        b = games.shape[0]
        return tok[None].expand(b, -1, -1).contiguous(), None, torch.full((b,), q, dtype=torch.float32, device=DEV)

    return policy


def test_terminal_leaf_is_worth_zero():
    S = 4
    a = np.array([2, 1, 1, 1, 1, 2, 1, 1, 1, 1, 0, 1], np.int8)          # u = e0, v = e1, w = -e2
    b = np.array([1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2], np.int8)
    start = np.zeros((1, 1, S, S, S), np.int8)
    start[0, 0] = R.O.action_to_tensor(a).astype(np.int8)                # a rank-1 start: action a factorises it
    forest = search.SearchForest(1, S, 1, k=2, max_actions=3, n_sim=4, device=DEV)
    out = search.actor_prediction(fixed_policy(forest, [b, a], -5.0), torch.from_numpy(start).to(DEV), 3, 4, 100, 3,
                                  k=2, forest=forest)
    r = R.play(lambda *args: (np.stack([b, a]), np.float32(-5.0)), start[0], 3, 4, 100, 3)
    n, q, nc, choice = (t.cpu().numpy() for t in forest.root_stats())
    assert int(out[3][0]) == r["length"] == 1 and choice[0, 0] == 1
    assert np.array_equal(q[0, 0, :2], r["root_Q"][0]) and np.array_equal(n[0, 0, :2], r["root_N"][0])
    assert q[0, 0, 1] == -1.0                                             # (0 * 0 + (0 - 1)) / 1: the leaf value is 0
    assert int(out[2][0, 0]) == -1 and not forest.final_heads().any()


def test_forced_cycle_sets_status_bit_1():
    S = 4
    rng = np.random.default_rng(3)
    forest = search.SearchForest(2, S, 1, k=2, max_actions=4, n_sim=8, max_depth=16, device=DEV)
    forest.reset(torch.from_numpy(random_starts(rng, 2, 1, S)).to(DEV), 8)
    pool = random_pool(rng, 8, S)
    simulate(forest, search.keyed_policy(forest, torch.from_numpy(pool), seed=1))
    assert forest.node_count.tolist() == [1, 1]
    forest.child_key[0, 0, :] = forest.root_key[0]                        # game 0: every child of the root is the root
    forest.select()
    torch.cuda.synchronize()
    assert forest.status.tolist() == [2, 0]
    assert int(forest.flags[0]) == 0 and int(forest.sims_left[0]) == 6 and int(forest.depth[0]) == 16
    assert int(forest.flags[1]) & search.PENDING


def test_full_pool_sets_status_bit_0():
    S = 4
    rng = np.random.default_rng(4)
    forest = search.SearchForest(3, S, 1, k=4, max_actions=2, max_nodes=1, device=DEV)
    pool = random_pool(rng, 8, S)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=2)
    forest.play(pol, torch.from_numpy(random_starts(rng, 3, 1, S)).to(DEV), 4)
    assert (forest.status.cpu().numpy() & 1).all()
    assert forest.node_count.tolist() == [1, 1, 1]
    assert not forest.child_n[:, 0].any()                                # the root's expansion has no path to back up,
    assert forest.done.all() and forest.move.tolist() == [1, 1, 1]       # every later one was dropped


def test_tokens_beyond_n_logits_set_status_bit_2():
    S = 4
    rng = np.random.default_rng(5)
    forest = search.SearchForest(2, S, 1, k=4, max_actions=2, n_sim=4, device=DEV)
    pool = random_pool(rng, 8, S)
    pool[:, 0] = 2
    forest.play(search.keyed_policy(forest, torch.from_numpy(pool), seed=3),
                torch.from_numpy(random_starts(rng, 2, 1, S)).to(DEV), 4)
    assert not forest.status.any()
    p3 = forest.policy(3, 4)
    assert not forest.status.any()
    p2 = forest.policy(2, 4)
    assert (forest.status.cpu().numpy() & 4).all()
    assert torch.equal(p2, p3[..., :2])                                   # tokens in range are counted as before


def test_outputs_stay_inside_their_buffers():
    S, B, T = 5, 6, 2
    rng = np.random.default_rng(6)
    forest = search.SearchForest(B, S, T, k=4, max_actions=3, n_sim=4, device=DEV)
    forest.reset(torch.from_numpy(random_starts(rng, B, T, S)).to(DEV), 4)
    pol = search.keyed_policy(forest, torch.from_numpy(random_pool(rng, 8, S)), seed=4)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        mbuf, model_in = guarded((B, T, S, S, S), dtype)
        sbuf, scalars = guarded((B, 1), torch.float32)
        ops.search_select(forest, model_in, scalars)
        tok, _, q = pol(model_in, scalars, torch.arange(B, device=DEV))
        forest.commit(tok, q)
        torch.cuda.synchronize()
        check_flat(mbuf, f"model input {dtype}")
        check_flat(sbuf, "scalars")
        heads = R.O.state_hash(model_in[:, 0].float().to(torch.int8).cpu().numpy())
        assert np.array_equal(heads.view(np.int64), forest.leaf_key.cpu().numpy())
    pbuf, pol_out = guarded((B, 3, 3 * S, 3), torch.float32)
    forest.advance(4)
    ops.search_policy(forest, 3, 2, out=pol_out)
    torch.cuda.synchronize()
    check_flat(pbuf, "policy")


def forest_arrays(f):
    names = ["node_key", "node_frames", "node_nchild", "child_tokens", "child_key", "child_n", "child_q", "index_key",
             "index_node", "node_count", "root_frames", "root_key", "move", "done", "sims_left", "status", "overflow",
             "leaf_frames", "leaf_key", "path_node", "path_slot", "depth", "flags", "attempt"]
    return {n: getattr(f, n).clone() for n in names}


def test_simulation_in_a_graph_equals_eager():
    S, B, T = 4, 256, 2
    rng = np.random.default_rng(7)
    start = torch.from_numpy(random_starts(rng, B, T, S)).to(DEV)
    pool = torch.from_numpy(random_pool(rng, 16, S))
    forests = [search.SearchForest(B, S, T, k=8, max_actions=4, n_sim=8, device=DEV) for _ in range(2)]
    pols = [search.keyed_policy(f, pool, seed=5) for f in forests]
    games = torch.arange(B, device=DEV)

    def sim(f, pol):
        frames, scalars = f.select()
        tok, _, q = pol(frames, scalars, games)
        f.commit(tok, q)

    for f, pol in zip(forests, pols):
        f.reset(start, 8)
        for _ in range(3):
            simulate(f, pol)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # capture runs nothing
        sim(forests[0], pols[0])
    graph.replay()
    sim(forests[1], pols[1])
    torch.cuda.synchronize()
    a, b = forest_arrays(forests[0]), forest_arrays(forests[1])
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert int(forests[0].node_count.sum()) > 3 * B


def test_puct_choice_maximises_the_ucb():
    S, B = 4, 128
    rng = np.random.default_rng(8)
    forest = search.SearchForest(B, S, 1, k=8, max_actions=4, n_sim=12, prior=True, device=DEV)
    forest.reset(torch.from_numpy(random_starts(rng, B, 1, S)).to(DEV), 12)
    pol = search.keyed_policy(forest, torch.from_numpy(random_pool(rng, 16, S)), seed=6)

    def prior_fn(rows):
        return torch.softmax(torch.linspace(-1, 1, 8, device=DEV)[None] * (1 + (rows[:, None] % 5)), dim=1).contiguous()

    def root_view():                                                      # the root is node 0 of every game
        return (forest.child_n[:, 0].double().cpu().numpy(), forest.child_q[:, 0].double().cpu().numpy(),
                forest.child_prior[:, 0].double().cpu().numpy(), forest.node_nchild[:, 0].cpu().numpy())

    simulate(forest, pol, prior_fn)
    assert forest.node_count.tolist() == [1] * B
    for _ in range(11):
        n, q, p, nc = root_view()                                         # what this simulation's descent sees
        simulate(forest, pol, prior_fn)
        chosen = forest.path_slot[:, 0].cpu().numpy()
        assert (forest.depth.cpu().numpy() >= 1).all()
        for g in range(B):
            c = nc[g]
            tot = n[g, :c].sum()
            ucb = q[g, :c] + (1.25 + np.log((tot + 19652.0 + 1.0) / 19652.0)) * p[g, :c] * np.sqrt(tot) / (1 + n[g, :c])
            best = ucb.max()
            assert ucb[chosen[g]] >= best - 1e-6 * max(1.0, abs(best)), (g, ucb, chosen[g])
    assert not forest.status.any()
