"""GPU checks of the search forest's less travelled paths (mat_mul_amd/csrc/tg_search.hip), every game of every batch
compared exactly with the host restatement (tests/search_ref.py); only the improved policy keeps the 4 ulp of
test_gpu_search.py, for the reason given there.

* the model input ``select`` emits -- all T frames, in float32 / float16 / bfloat16 -- and its scalar equal the frames
  and scalar of the restatement's policy calls, call by call; rows of games not selected are not written;
* ``overflow`` is set for exactly the games in which a candidate child head left int8, stays set, and is cleared by
  ``reset``; the wrapped heads are part of the compared games; a candidate that is dropped counts too;
* ``shift = 2``; T up to 16; sizes whose last 16-byte chunk holds one hash word (S = 6, 7) and S = 9; ``root_key``;
* the per-game index at capacities below one 64-slot probe round, fully loaded, with probe chains of several rounds
  that wrap past the end of the table, and full (status bit 0);
* priors stored at the compacted slot of the candidate they belong to;
* horizons 0, 1 and beyond max_actions; games that start at an all-zero head.

One driver (``drive``) runs the reset / select / policy / commit / retry / advance loop the way ``SearchForest.play``
does, with hooks around ``select`` and after ``reset``, because some tests edit or read the forest in between."""
import numpy as np
import pytest
import torch

from mat_mul_amd import ops, search
from guarded_buffers import CANARY, GUARD, check_flat, guarded
import search_ref as R
from test_gpu_search import forest_arrays as sibling_forest_arrays
from test_gpu_search import random_pool, random_starts, ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEED = search.EXPAND | search.PENDING
N_BAR = 4
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def forest_arrays(f, skip=()):
    """test_gpu_search.forest_arrays plus the trajectory rows and the priors, without the names in ``skip``."""
    out = sibling_forest_arrays(f)
    for n in ("traj_frames", "traj_node", "traj_choice") + (("child_prior",) if f.child_prior is not None else ()):
        out[n] = getattr(f, n).clone()
    return {n: t for n, t in out.items() if n not in skip}


def drive(forest, pol, start, n_sim, n_logits=3, model_in=None, scalars=None, after_reset=None, before_select=None,
          after_select=None, prior_fn=None, max_retries=256):
    """``SearchForest.play`` and the tail of ``actor_prediction``, call by call: reset; per move, per simulation one
    select, the policy, commit, and commit again under a mask for the games that ask for a retry; advance.  ``model_in``
    / ``scalars`` replace the forest's own model-input buffers.  Returns (states, policy, rewards, lengths)."""
    forest.reset(torch.from_numpy(start).to(DEV), n_sim)
    if after_reset is not None:
        after_reset()
    games = torch.arange(forest.B, device=DEV)
    for _ in range(forest.max_actions):
        for _ in range(n_sim):
            if before_select is not None:
                before_select()
            if model_in is None:
                frames, sc = forest.select()
            else:
                ops.search_select(forest, model_in, scalars)
                frames, sc = model_in, scalars
            if after_select is not None:
                after_select()
            mask = None
            for _ in range(max_retries + 1):
                tok, _, q = pol(frames, sc, games)
                forest.commit(tok, q, prior=None if prior_fn is None else prior_fn(tok), mask=mask)
                retry = (forest.flags & search.RETRY) != 0
                if not bool(retry.any()):
                    break
                mask = retry.to(torch.uint8)
            else:
                raise AssertionError("retries did not end")
            if not bool(((forest.sims_left > 0) & (forest.done == 0)).any()):
                break
        forest.advance(n_sim)
        if bool(forest.done.all()):
            break
    lengths = forest.lengths()
    rank = ops.slice_rank(forest.final_heads())
    return forest.states(), forest.policy(n_logits, N_BAR), search.rewards_of(lengths, rank, forest.max_actions), lengths


def restate(forest, start, pool, seed, n_sim, n_logits=3, games=None):
    """The restatement's game for every game of the batch (or for ``games``): {game: result of search_ref.play}."""
    fn = R.keyed_policy(pool, forest.k, seed=seed)
    return {g: R.play(fn, start[g], forest.max_actions, n_sim, N_BAR, n_logits, horizon=forest.horizon,
                      max_depth=forest.max_depth, shift=forest.shift)
            for g in (range(forest.B) if games is None else games)}


def check_games(forest, out, refs):
    """The assertions of test_gpu_search.check_against_restatement on every game of ``refs``, plus the final head."""
    states, policy, rewards, lengths = (t.cpu().numpy() for t in out)
    n, q, nc, choice = (t.cpu().numpy() for t in forest.root_stats())
    final = forest.final_heads().cpu().numpy()
    for gi, r in refs.items():
        L = r["length"]
        assert L == lengths[gi], gi
        assert np.array_equal(states[gi, :L], r["states"]) and not states[gi, L:].any(), gi
        assert np.array_equal(rewards[gi, :L], r["rewards"]) and not rewards[gi, L:].any(), gi
        assert np.array_equal(choice[gi, :L], r["choice"]), gi
        for m in range(L):
            assert nc[gi, m] == len(r["root_N"][m])
            assert np.array_equal(n[gi, m, :nc[gi, m]].view(np.int32), r["root_N"][m].view(np.int32)), (gi, m)
            assert np.array_equal(q[gi, m, :nc[gi, m]].view(np.int32), r["root_Q"][m].view(np.int32)), (gi, m)
        assert int(ulp_diff(policy[gi, :L], r["policy"]).max()) <= 4 and not policy[gi, L:].any(), gi
        assert np.array_equal(final[gi], r["final"][0]), gi


def play_and_check(S, T, B, rng, n_sim=8, max_actions=4, k=8, shift=1, n_logits=3, seed=7, after_reset=None, **forest_kw):
    """One batch with the keyed policy against the restatement, every game.  Returns (forest, start, refs)."""
    start = random_starts(rng, B, T, S)
    pool = random_pool(rng, 24, S) + (shift - 1)                          # factor values -1, 0, 1 at any shift
    forest = search.SearchForest(B, S, T, k=k, max_actions=max_actions, n_sim=n_sim, shift=shift, device=DEV, **forest_kw)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    out = drive(forest, pol, start, n_sim, n_logits=n_logits,
                after_reset=None if after_reset is None else (lambda: after_reset(forest, start)))
    refs = restate(forest, start, pool, seed, n_sim, n_logits=n_logits)
    check_games(forest, out, refs)
    assert not forest.status.any()
    assert np.array_equal(forest.overflow.cpu().numpy() != 0, [refs[g]["overflow"] for g in range(B)])
    return forest, start, refs


# ---- 1. the model input -------------------------------------------------------------------------------------------

def model_input_case(S, T):
    """Starts with a full random history (frames 1.. are what ``select`` must pass on unchanged) and the pool."""
    B = 8 if S == 16 else 16
    rng = np.random.default_rng(100 * S + T)
    start = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(B, T, S, S, S)).astype(np.int8)
    return B, start, random_pool(rng, 24, S)


def as_bytes(frames, dtype):
    """The bytes of int8 frames converted to ``dtype`` (exact for every int8 value in all three types)."""
    return torch.from_numpy(np.ascontiguousarray(frames, np.int8)).to(dtype).contiguous().view(torch.uint8).numpy().ravel()


@pytest.mark.parametrize("S, T, dtype", [(4, 2, F32), (5, 3, F32), (5, 3, F16), (5, 3, BF16), (9, 4, F32), (9, 4, F16),
                                         (9, 4, BF16), (6, 2, F32), (16, 16, F32)])
def test_model_input_is_the_restatements_frames(S, T, dtype):
    B, start, pool = model_input_case(S, T)
    n_sim, seed = 8, 11
    forest = search.SearchForest(B, S, T, k=8, max_actions=4, n_sim=n_sim, device=DEV)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    mbuf, model_in = guarded((B, T, S, S, S), dtype)
    sbuf, scalars = guarded((B, 1), F32)
    log = {g: [] for g in range(B)}

    def before_select():                                                  # the pattern an unselected row must keep
        mbuf[GUARD:-GUARD].fill_(CANARY)
        sbuf[GUARD:-GUARD].fill_(CANARY)

    def after_select():
        flags, move = forest.flags.cpu().numpy(), forest.move.cpu().numpy()
        rows = mbuf[GUARD:-GUARD].view(B, -1).cpu().numpy()
        sc = sbuf[GUARD:-GUARD].view(B, 4).cpu().numpy()
        check_flat(mbuf, "model input")
        check_flat(sbuf, "scalars")
        for g in range(B):
            if not flags[g] & search.PENDING:
                assert flags[g] == 0 and (rows[g] == CANARY).all() and (sc[g] == CANARY).all(), g
            elif (flags[g] & NEED) == NEED:
                log[g].append((rows[g].copy(), float(sc[g].view(np.float32)[0]), int(move[g])))

    out = drive(forest, pol, start, n_sim, model_in=model_in, scalars=scalars, before_select=before_select,
                after_select=after_select)
    refs = restate(forest, start, pool, seed, n_sim)
    check_games(forest, out, refs)
    assert not forest.status.any()
    deep = history = False
    for g in range(B):
        want = [c for c in refs[g]["calls"] if c[2] == 0]                 # one first call per expansion
        assert len(log[g]) == len(want), g
        for (row, scalar, move), (frames, idx, _, _) in zip(log[g], want):
            assert np.array_equal(row, as_bytes(frames, dtype)), (g, idx)
            assert scalar == float(idx), (g, idx)
            deep |= idx - move >= 2
            history |= T >= 3 and bool(frames[2].any())
    assert deep and (history or T < 3)                                    # or the history shift was never exercised


# ---- 2. overflow and wrap -----------------------------------------------------------------------------------------

def overflow_case(S, T, B):
    rng = np.random.default_rng(200 * S + T)
    start = random_starts(rng, B, T, S)
    head = start[::2, 0]                                                  # even games sit at the ends of int8
    head[head == 1] = 127
    head[head == -1] = -128
    return rng, start


@pytest.mark.parametrize("S, T, shift, B", [(4, 2, 1, 32), (5, 3, 2, 16)])
def test_overflow_flag_and_wrapped_heads(S, T, shift, B):
    rng, start = overflow_case(S, T, B)
    pool = random_pool(rng, 24, S) + (shift - 1)
    n_sim, seed, n_logits, k = 8, 13, shift + 2, 8
    forest = search.SearchForest(B, S, T, k=k, max_actions=4, n_sim=n_sim, shift=shift, device=DEV)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    out = drive(forest, pol, start, n_sim, n_logits=n_logits)
    refs = restate(forest, start, pool, seed, n_sim, n_logits=n_logits)
    check_games(forest, out, refs)                                        # the wrapped heads are in these trajectories
    want = np.array([refs[g]["overflow"] for g in range(B)])
    assert np.array_equal(want, np.arange(B) % 2 == 0)                    # every even game and no odd one
    assert np.array_equal(forest.overflow.cpu().numpy(), want.astype(np.uint8))
    assert not forest.status.any() and all(refs[g]["length"] == 4 for g in range(B))
    heads = out[0].cpu().numpy()[:, :, 0].astype(np.int64)               # a move over the edge changes an entry by ~256
    assert (np.abs(np.diff(heads, axis=1)).reshape(B, -1).max(axis=1) > 128).any()
    # sticky: one more simulation in which no child leaves int8 (one entry of the leaf head moves towards zero).  The
    # games are over, so they are reopened at move 0 from their final roots: the leaves lie inside the horizon again
    forest.done.zero_()
    forest.move.zero_()
    forest.sims_left.fill_(1)
    forest.select()
    assert bool(((forest.flags & search.PENDING) != 0).all())
    leaf = forest.leaf_frames[:, 0, :S ** 3].cpu().numpy().reshape(B, S, S, S)
    tok = np.full((B, k, 3 * S), shift, np.int8)
    for g in range(B):
        if not leaf[g].any():
            continue                                                      # a terminal leaf takes no candidates
        i, j, l = np.argwhere(leaf[g] != 0)[0]
        tok[g, :, i], tok[g, :, S + j], tok[g, :, 2 * S + l] = shift + 1, shift + 1, shift + (1 if leaf[g, i, j, l] > 0 else -1)
    count = forest.node_count.clone()
    forest.commit(torch.from_numpy(tok).to(DEV), torch.zeros(B, device=DEV))
    assert bool((forest.node_count > count).any())                        # some game did form children here
    assert np.array_equal(forest.overflow.cpu().numpy(), want.astype(np.uint8))
    forest.reset(torch.from_numpy(start).to(DEV), n_sim)
    assert not forest.overflow.any()


def test_overflow_counts_the_candidates_that_are_dropped():
    """One hand-made expansion per game from a head with 127 at [0,0,0]: the candidate that takes it to 128 counts
    whether it is kept (game 2), dropped because its child is already in the index (game 0) or dropped together with
    every other candidate, which asks for a retry (game 3); without it nothing is set (game 1)."""
    S, B, k = 4, 4, 2
    minus = np.array([2, 1, 1, 1, 2, 1, 1, 1, 0, 1, 1, 1], np.int8)       # product -1 at [0,0,0]
    fresh = np.array([1, 2, 1, 1, 1, 2, 1, 1, 1, 2, 1, 1], np.int8)       # product +1 at [1,1,1]
    null = np.ones(3 * S, np.int8)
    start = np.zeros((B, 1, S, S, S), np.int8)
    start[:, 0, 0, 0, 0], start[:, 0, 1, 1, 1] = 127, 1
    wrapped = start[0, 0].copy()
    wrapped[0, 0, 0] = -128                                               # the child of `minus`, after the wrap
    forest = search.SearchForest(B, S, 1, k=k, max_actions=2, n_sim=2, device=DEV)
    forest.reset(torch.from_numpy(start).to(DEV), 2)
    key = R.O.state_hash(wrapped[None])
    slot = int(key[0] & np.uint64(forest.index_capacity - 1))
    forest.index_key[[0, 3], slot] = int(key.view(np.int64)[0])           # games 0 and 3 know that child already
    forest.select()
    tok = np.stack([[minus, fresh], [null, fresh], [minus, fresh], [minus, null]])
    forest.commit(torch.from_numpy(tok).to(DEV), torch.zeros(B, device=DEV))
    assert forest.overflow.tolist() == [1, 0, 1, 1]
    assert forest.node_count.tolist() == [1, 1, 1, 0] and forest.node_nchild[:, 0].tolist() == [1, 1, 2, 0]
    assert np.array_equal(forest.child_tokens[:3, 0, 0].cpu().numpy(), [fresh, fresh, minus])
    assert [int(f) & search.RETRY for f in forest.flags.tolist()] == [0, 0, 0, search.RETRY]
    assert forest.attempt.tolist() == [0, 0, 0, 1] and not forest.status.any()
    kids = forest.child_key[2, 0].cpu().numpy().view(np.uint64)
    assert kids[0] == key[0]                                              # the stored key is the wrapped head's


# ---- 3. shift = 2, 4. sizes and T, 7. horizon ------------------------------------------------------------------------

def root_key_is_the_head_hash(forest, start):
    assert np.array_equal(forest.root_key.cpu().numpy().view(np.uint64), R.O.state_hash(start[:, 0]))


@pytest.mark.parametrize("S, T", [(4, 2), (9, 2)])
def test_shift_two_games(S, T):
    play_and_check(S, T, 16, np.random.default_rng(300 * S + T), shift=2, n_logits=4)


@pytest.mark.parametrize("S, T", [(6, 2), (7, 1), (9, 4), (4, 16)])
def test_sizes_and_frame_counts(S, T):
    """S = 6 and 7 end in a 16-byte chunk with a single 8-byte hash word, S = 9 in one with 9 valid bytes."""
    play_and_check(S, T, 16, np.random.default_rng(400 * S + T), after_reset=root_key_is_the_head_hash)


@pytest.mark.parametrize("horizon", [0, 1, 9])
def test_horizon_bounds(horizon):
    """Expansion needs idx <= min(max_actions, move + horizon): horizon 0 and 1 bind at every move, max_actions + 3
    never does."""
    play_and_check(4, 2, 16, np.random.default_rng(700 + horizon), max_actions=6, horizon=horizon)


def test_games_that_start_at_zero():
    S, T, B, n_sim, seed = 4, 2, 5, 8, 17                                 # B = 5: one live wavefront in the last workgroup
    rng = np.random.default_rng(701)
    start = random_starts(rng, B, T, S)
    start[[0, 4]] = 0
    pool = random_pool(rng, 24, S)
    forest = search.SearchForest(B, S, T, k=8, max_actions=4, n_sim=n_sim, device=DEV)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    mbuf, model_in = guarded((B, T, S, S, S), F32)
    sbuf, scalars = guarded((B, 1), F32)

    def after_reset():
        assert forest.done.tolist() == [1, 0, 0, 0, 1] and forest.sims_left.tolist() == [0, n_sim, n_sim, n_sim, 0]

    def after_select():
        assert forest.flags[[0, 4]].tolist() == [0, 0]

    out = drive(forest, pol, start, n_sim, model_in=model_in, scalars=scalars, after_reset=after_reset,
                after_select=after_select)
    check_games(forest, out, restate(forest, start, pool, seed, n_sim, games=[1, 2, 3]))
    states, policy, rewards, lengths = out
    for g in (0, 4):
        assert int(lengths[g]) == 0 and not states[g].any() and not policy[g].any() and not rewards[g].any()
        assert int(forest.node_count[g]) == 0 and bool(forest.done[g])
    rows, sc = mbuf[GUARD:-GUARD].view(B, -1), sbuf[GUARD:-GUARD].view(B, 4)
    assert bool((rows[[0, 4]] == CANARY).all()) and bool((sc[[0, 4]] == CANARY).all())   # never written
    assert not bool((rows[1:4] == CANARY).all(dim=1).any())
    check_flat(mbuf, "model input")
    check_flat(sbuf, "scalars")
    assert not forest.status.any() and not forest.overflow.any()


# ---- 5. index geometry --------------------------------------------------------------------------------------------

DUMMY = 0x0123456789ABCDEF                                                # occupies a slot, equals no node key
HOLE = slice(100, 141)                                                    # the slots of the long-chain table left empty


def index_case(cap, M, n_sim, max_actions, fill=False, B=16, S=4, T=2, seed=19):
    """The same batch on a forest with the default index and on one with ``cap`` slots per game.  Returns both forests,
    the outputs of both runs, the restatement's games and the guarded model input of the second run."""
    rng = np.random.default_rng(500 + cap)
    start, pool = random_starts(rng, B, T, S), random_pool(rng, 24, S)
    runs = []
    for capacity in (None, cap):
        forest = search.SearchForest(B, S, T, k=8, max_actions=max_actions, max_nodes=M, index_capacity=capacity,
                                     device=DEV)
        pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
        mbuf, model_in = guarded((B, T, S, S, S), F32)
        sbuf, scalars = guarded((B, 1), F32)

        def occupy(forest=forest):                                        # caller-owned memory, the header's layout
            forest.index_key.fill_(DUMMY)
            forest.index_key[:, HOLE] = 0

        out = drive(forest, pol, start, n_sim, model_in=model_in, scalars=scalars,
                    after_reset=occupy if fill and capacity is not None else None)
        check_flat(mbuf, "model input")
        check_flat(sbuf, "scalars")
        runs.append((forest, out))
    assert runs[0][0].index_capacity >= 64 and runs[0][0].index_capacity >= 2 * M and runs[1][0].index_capacity == cap
    return runs, restate(runs[0][0], start, pool, seed, n_sim)


def same_forest(a, b):
    x, y = (forest_arrays(f, skip=("index_key", "index_node")) for f in (a, b))
    for n in x:
        assert torch.equal(x[n], y[n]), n


@pytest.mark.parametrize("cap, M, n_sim, max_actions", [(8, 8, 3, 2), (32, 32, 7, 4), (64, 64, 16, 4)])
def test_small_and_fully_loaded_index(cap, M, n_sim, max_actions):
    """Capacities below one 64-slot probe round (the lanes past the capacity take no part) and a table with as many
    slots as the pool has nodes."""
    runs, refs = index_case(cap, M, n_sim, max_actions)
    for forest, out in runs:
        check_games(forest, out, refs)
        assert not forest.status.any()
    same_forest(runs[0][0], runs[1][0])
    assert int(runs[1][0].node_count.max()) * 2 > cap                     # the small table did run at a high load


def test_probe_chains_of_several_rounds_that_wrap():
    cap, M = 512, 40
    runs, refs = index_case(cap, M, 8, 4, fill=True)
    for forest, out in runs:
        check_games(forest, out, refs)
        assert not forest.status.any()
    same_forest(runs[0][0], runs[1][0])
    forest = runs[1][0]
    count = forest.node_count.cpu().numpy()
    keys = forest.node_key.cpu().numpy().view(np.uint64)
    table = forest.index_key.cpu().numpy().view(np.uint64)
    nodes = forest.index_node.cpu().numpy()
    homes = []
    for g in range(forest.B):
        mine = keys[g, :count[g]]
        assert DUMMY not in mine and 0 not in mine
        homes += (mine & np.uint64(cap - 1)).tolist()
        hole = table[g, HOLE]
        assert (np.delete(table[g], np.arange(cap)[HOLE]) == DUMMY).all()         # nothing stored outside the hole
        assert sorted(hole[hole != 0].tolist()) == sorted(mine.tolist()), g      # every node exactly once inside it
        for slot in np.flatnonzero(hole != 0) + HOLE.start:
            assert keys[g, nodes[g, slot]] == table[g, slot], (g, slot)
    assert max(homes) > 140                                               # such a chain wraps past the end of the table
    assert min(homes) < 36                                                # and such a one needs a second 64-slot round


def test_full_index_sets_status_bit_0():
    """Sixteen slots for a game that wants more nodes: the header's behaviour for a full index.  The games whose tree
    outgrows the table in the restatement are the ones that meet it; the others play as if nothing happened."""
    cap = 16
    runs, refs = index_case(cap, 40, 8, 4)
    forest, out = runs[1]
    full = np.array([refs[g]["n_nodes"] > cap for g in range(forest.B)])
    status = forest.status.cpu().numpy()
    assert full.any() and np.array_equal(status, full.astype(status.dtype))       # bit 0 there, no bit anywhere else
    assert int(forest.node_count.max()) <= cap and bool(forest.done.all())
    assert bool(torch.isfinite(forest.child_n).all()) and bool(torch.isfinite(forest.child_q).all())
    check_games(forest, out, {g: r for g, r in refs.items() if not full[g]})
    check_games(*runs[0], refs)
    assert not runs[0][0].status.any()


# ---- 6. prior compaction ------------------------------------------------------------------------------------------

def prior_of_tokens(tok):
    """A prior that is a function of the candidate's own token row alone and differs for any two rows of tokens in
    {0,1,2}: the row read as a base-3 number (< 3^12 < 2^24, exact in float32), plus one, times 2^-20."""
    w = 3 ** np.arange(tok.shape[-1], dtype=np.int64)
    if isinstance(tok, torch.Tensor):
        v = (tok.to(torch.int64) * torch.from_numpy(w).to(tok.device)).sum(-1) + 1
        return (v.to(torch.float32) * 2.0 ** -20).contiguous()
    return ((np.asarray(tok, np.int64) * w).sum(-1) + 1).astype(np.float32) * np.float32(2.0 ** -20)


def prior_case(S=4, B=32):
    rng = np.random.default_rng(600)
    start = random_starts(rng, B, 1, S)
    pool = random_pool(rng, 24, S)
    pool[::3] = 1                                                         # a third of the pool: null actions
    return start, pool


def root_survivors(fn, head, shift=1):
    """The candidates of the first expansion of a game that survive the null filter (the tree is empty, so the other
    filter drops nothing), as indices into the k candidates, and their token rows."""
    key = R.head_key(head)
    for attempt in range(256):
        tokens, _ = fn(head, None, 0, attempt, key)
        kids = (head[None].astype(np.int64) - R.O.action_to_tensor(tokens, shift)).astype(np.int8)
        keep = np.flatnonzero((kids != head[None]).reshape(len(tokens), -1).any(axis=1))
        if len(keep):
            return keep, tokens[keep]
    raise AssertionError("no surviving candidate")


def test_prior_is_stored_with_its_own_candidate():
    S, B, k, n_sim, seed = 4, 32, 8, 8, 23
    start, pool = prior_case(S, B)
    forest = search.SearchForest(B, S, 1, k=k, max_actions=4, n_sim=n_sim, prior=True, device=DEV)
    pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=seed)
    drive(forest, pol, start, n_sim, prior_fn=prior_of_tokens)
    assert not forest.status.any()
    count, nchild = forest.node_count.cpu().numpy(), forest.node_nchild.cpu().numpy()
    tokens, prior = forest.child_tokens.cpu().numpy(), forest.child_prior.cpu().numpy()
    fn = R.keyed_policy(pool, k, seed=seed)
    moved = False
    for g in range(B):
        assert count[g] >= 1
        for node in range(count[g]):
            nc = nchild[g, node]
            assert 1 <= nc <= k
            assert np.array_equal(prior[g, node, :nc].view(np.int32),
                                  prior_of_tokens(tokens[g, node, :nc]).view(np.int32)), (g, node)
        keep, rows = root_survivors(fn, start[g, 0])                      # node 0 is the root's expansion
        assert nchild[g, 0] == len(keep) and np.array_equal(tokens[g, 0, :len(keep)], rows), g
        moved |= bool((keep > np.arange(len(keep))).any())
    assert moved                                                          # a survivor was stored below its candidate index
