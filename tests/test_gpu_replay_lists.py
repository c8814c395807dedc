"""GPU checks of move lists stored as games (include/tensor_game_replay_lists.h, ops.replay_add_lists,
GameBuffer.add_lists, TensorGameData.add_solutions) on the MI355X: bit for bit against the host restatement
(tests/replay_lists_ref.py) over the sizes, history depths and list lengths at which the kernels take another path; every
class of invalid list between valid ones; the ring's wrap; the best-list rule; equivalence with the composed path
(env steps, stacked frames, a one-hot policy, ops.replay_add) on the device; the ring protocol of the three entries that store games (the edges of
the plan's chunk and of the rebuild's slot ranges, one ring from the three input forms, a folded ring[0]); addressing at odd byte offsets between
guard bytes; graph capture; and the solution search end to end into the dataset, its batches and a saved run."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_io_ref as IO
import replay_lists_ref as LR
import replay_ref as RR
import ring_cases as RC
from guarded_buffers import CANARY, GUARD, check_flat
from ring_cases import assert_ring
from mat_mul_amd import (FusedTrainer, GameBuffer, SolutionArchive, SyntheticDemos, TensorGameData, TensorGameError, _lib,
                         ops, replay_io, rollout)
from net_ref import CONFIGS, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.cpu().numpy()


def term_sum(tokens, n, S, shift):
    return -LR.heads_of(np.zeros((S, S, S), np.int32), tokens, n, shift)[-1]


def make_lists(rng, S, T, K, M, shift, shared):
    """Valid lists, solvable by construction (a start's frame 0 is the sum of its list's terms; the history frames are
    random).  ``shared``: two lists per group, in reversed order, the second with its terms reversed; else one group per
    list and no groups array.  Lengths include 1 and K.  (starts, tokens, lengths, groups or None)."""
    G = (M + 1) // 2 if shared else M
    own = rng.integers(0, 3, size=(G, K, 3 * S)).astype(np.int8) + np.int8(shift - 1)
    glen = rng.integers(1, K + 1, size=G).astype(np.int64)
    glen[0], glen[-1] = 1, K
    starts = rng.integers(-3, 4, size=(G, T, S, S, S)).astype(np.int8)
    for g in range(G):
        starts[g, 0] = term_sum(own[g], int(glen[g]), S, shift)
    if not shared:
        tokens = own.copy()
        for g in range(G):
            tokens[g, glen[g]:] = rng.integers(0, 4, size=(K - glen[g], 3 * S))  # rows behind a list are not read
        return starts, tokens, glen, None
    groups = np.array([(M - 1 - m) // 2 for m in range(M)], np.int64)
    tokens, lengths = np.zeros((M, K, 3 * S), np.int8), glen[groups]
    for m, g in enumerate(groups):
        n = int(glen[g])
        tokens[m, :n] = own[g, :n] if m % 2 == 0 else own[g, :n][::-1]
    return starts, tokens, lengths, groups


def run_both(buf, want, starts, tokens, lengths, groups, shift, select=False, what=""):
    stored = ops.replay_add_lists(buf, dev(starts), dev(tokens), dev(lengths), None if groups is None else dev(groups),
                                  shift=shift, select=select, status=buf.status)
    want_stored, want_status = LR.add_lists(want, starts, tokens, lengths, groups, shift, select)
    assert host(stored).tolist() == want_stored.tolist(), what
    assert_ring(buf, want, what)
    return want_status


# ---- bit for bit against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("S", [4, 5, 9, 16, 25])
def test_bit_for_bit_against_the_restatement(S, T, K):
    rng = np.random.default_rng(100 * S + 10 * T + K)
    M = 37 if S <= 9 else 5
    buf, want = GameBuffer(M + 3, K + 1, T, S, DEV), RR.Ring(M + 3, K + 1)  # the second call wraps the ring
    status = 0
    for shift, shared in ((1, False), (2, True)):
        starts, tokens, lengths, groups = make_lists(rng, S, T, K, M, shift, shared)
        assert {1, K} <= set(lengths.tolist())
        status |= run_both(buf, want, starts, tokens, lengths, groups, shift, what=(shift, shared))
    assert status == 0 == int(buf.status) and want.added == 2 * M


# ---- invalid lists ---------------------------------------------------------------------------------------------------
def test_every_class_of_invalid_list_between_valid_ones():
    S, T, K, L, M, G = 4, 2, 258, 256, 17, 17
    rng = np.random.default_rng(3)
    starts, short, lengths, _ = make_lists(rng, S, T, 8, M, 1, False)
    tokens = np.ones((M, K, 3 * S), np.int8)
    tokens[:, :8] = short
    groups = np.arange(M, dtype=np.int64)
    e0 = lambda u: np.array([u] + [0] * (S - 1) + ([1] + [0] * (S - 1)) * 2, np.int8) + 1  # u e0 (x) e0 (x) e0
    lengths[1] = 0
    lengths[3] = K + 1
    lengths[5] = L + 1                               # <= K, longer than a slot
    groups[7], groups[9] = -1, G
    starts[11, 0], tokens[11, :256], lengths[11] = 0, e0(1), 256   # an int8 stepper wraps -256 to 0 and reports it solved
    starts[13, 0] = 0
    starts[13, 0, 0, 0, 0] = -128
    tokens[13, :3], lengths[13] = (e0(1), e0(-1), e0(-128)), 3     # -129, -128, 0: leaves int8 and comes back
    starts[15, 0, -1, -1, -1] += 1                                 # ends one entry away from zero
    buf, want = GameBuffer(16, L, T, S, DEV), RR.Ring(16, L)
    before = host(buf.frames).copy()
    status = run_both(buf, want, starts, tokens, lengths, groups, 1)
    bits = [0, 1, 0, 1, 0, 1, 0, 4, 0, 4, 0, 8 | 16, 0, 8, 0, 16, 0]
    for m in range(M):
        assert LR.list_flags(starts, tokens[m], int(lengths[m]), int(groups[m]), K, L, 1)[0] == bits[m], m
    assert status == 29 == int(buf.status) and want.added == 9 == int(buf.ring[1])
    assert np.array_equal(host(buf.frames)[9:], before[9:])       # nothing stored for them: 9 games, slots 0 .. 8
    # the valid neighbours are stored exactly as they are without the invalid lists between them
    alone, valid = RR.Ring(16, L), [m for m in range(M) if not bits[m]]
    LR.add_lists(alone, starts, tokens[valid], lengths[valid], groups[valid], 1)
    assert_ring(buf, alone)


# ---- wrap ------------------------------------------------------------------------------------------------------------
def test_more_valid_lists_than_slots():
    S, T, K, M = 5, 2, 3, 8
    rng = np.random.default_rng(8)
    starts, tokens, lengths, groups = make_lists(rng, S, T, K, M, 1, False)
    buf, want = GameBuffer(3, K, T, S, DEV), RR.Ring(3, K)
    run_both(buf, want, starts[:2], tokens[:2], lengths[:2], None, 1)  # the ring's pointer is not at 0
    run_both(buf, want, starts[2:], tokens[2:], lengths[2:], None, 1)  # 6 valid lists into 3 slots: the last 3
    assert int(buf.ring[1]) == 8 and int(buf.ring[0]) == 8 % 3
    for j, m in enumerate((5, 6, 7)):                                  # lists 5, 6, 7 in slots 2, 0, 1
        slot = (2 + 3 + j) % 3
        assert np.array_equal(host(buf.tokens)[slot, :lengths[m]], tokens[m, :lengths[m]])


@pytest.mark.parametrize("capacity", [3, 2048])
def test_more_lists_than_one_plan_chunk_with_and_without_stored(capacity):
    S, T, K, M = 4, 1, 2, 1100
    rng = np.random.default_rng(capacity)
    starts, tokens, lengths, _ = make_lists(rng, S, T, K, M, 1, False)
    lengths[(rng.random(M) < 0.2) & (np.arange(M) != 1030)] = 0
    starts[1030, 0, 0, 0, 0] += 1                                      # not zero at the end
    want = RR.Ring(capacity, K)
    want_stored, want_status = LR.add_lists(want, starts, tokens, lengths)
    assert want_status == 17 and want.added > 800
    for with_stored in (True, False):
        buf = GameBuffer(capacity, K, T, S, DEV)
        args = [dev(starts), dev(tokens), dev(lengths)]
        if with_stored:
            stored = ops.replay_add_lists(buf, *args, status=buf.status)
            assert host(stored).tolist() == want_stored.tolist()
        else:  # the C entry without `stored`: the plan replays the lists itself
            with torch.cuda.device(DEV):
                _lib.call("tg_replay_add_lists", C.byref(buf.desc), args[0].data_ptr(), M, None, args[1].data_ptr(),
                          args[2].data_ptr(), M, K, 1, 0, None, buf.status.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        assert_ring(buf, want, with_stored)
        assert int(buf.status) == want_status


# ---- select ----------------------------------------------------------------------------------------------------------
def test_select_takes_the_first_shortest_valid_list():
    S, T, K, M = 4, 2, 4, 6
    rng = np.random.default_rng(12)
    starts, tokens, _, _ = make_lists(rng, S, T, K, M, 1, False)
    lengths = np.array([3, 2, 2, 1, 4, 2], np.int64)
    for m in range(M):
        starts[m, 0] = term_sum(tokens[m], int(lengths[m]), S, 1)
    starts[3, 0, 0, 0, 0] += 1                                         # the shortest list is invalid
    buf, want = GameBuffer(3, K, T, S, DEV), RR.Ring(3, K)
    for _ in range(2):                                                 # twice: the second lands in the next slot
        status = run_both(buf, want, starts, tokens, lengths, None, 1, select=True)
    assert status == 16 == int(buf.status) and want.added == 2
    stored = ops.replay_add_lists(buf, dev(starts), dev(tokens), dev(lengths), select=True)
    assert host(stored).tolist() == [0, 1, 0, 0, 0, 0]                 # the tie of lists 1, 2 and 5 goes to the lowest index
    # nothing valid: nothing stored, the buffer unchanged
    keep = [getattr(buf, n).clone() for n in ("frames", "tokens", "rewards", "length", "offset", "ring")]
    none = lengths.copy()
    none[[0, 1, 2, 4, 5]] = 0
    stored = ops.replay_add_lists(buf, dev(starts), dev(tokens), dev(none), select=True, status=buf.status)
    assert not host(stored).any() and int(buf.status) == 17
    for n, t in zip(("frames", "tokens", "rewards", "length", "offset", "ring"), keep):
        assert torch.equal(getattr(buf, n), t), n


# ---- equivalence with the composed path, on the device ---------------------------------------------------------------
@pytest.mark.parametrize("S,T,shared", [(4, 2, True), (5, 4, False), (25, 2, True)])
def test_equals_the_composed_path_on_the_device(S, T, shared):
    K, M, shift = 5, 6, 1
    rng = np.random.default_rng(S)
    starts, tokens, lengths, groups = make_lists(rng, S, T, K, M, shift, shared)
    tokens = np.where(np.arange(K)[None, :, None] < lengths[:, None, None], tokens, 1).astype(np.int8)
    d = [dev(starts), dev(tokens), dev(lengths), None if groups is None else dev(groups)]
    for select in (False, True):
        a, b = GameBuffer(4, K + 2, T, S, DEV), GameBuffer(4, K + 2, T, S, DEV)  # 6 lists into 4 slots
        a.add_lists(d[0], d[1], d[2], groups=d[3], shift=shift, best=select)
        LR.composed_add(b, d[0], d[1], d[2], d[3], shift=shift, select=select)
        for x, y in zip(a.pack(), b.pack()):
            assert torch.equal(x, y)
        n = len(a)
        assert n == len(b) > 0
        idx = torch.arange(n, device=DEV)
        for x, y in zip(a.items(idx), b.items(idx)):
            assert torch.equal(x, y)
        assert int(a.status) == int(b.status) == 0


# ---- the ring protocol the three entries share (csrc/tg_ring.h) --------------------------------------------------------
@pytest.mark.parametrize("C", RC.EDGE_C)
@pytest.mark.parametrize("N", RC.EDGE_N)
def test_add_lists_at_the_plan_chunk_and_slot_range_edges(N, C):
    RC.check_edges("add_lists", N, C, DEV)


@pytest.mark.parametrize("C, held", [(3, 0), (5, 4)])
def test_the_three_entries_leave_one_ring(C, held):
    """The same games as padded states with a one-hot policy, as packed rows and as move lists, each into a zeroed ring
    of 3 slots and into one of 5 that already holds four games: one ring, whichever entry stored them."""
    S, T, K = 2, 2, 3
    rng = np.random.default_rng(C)
    before = RC.three_forms(*RC.solvable_lists(rng, held, S, T, K), K)["add_packed"] if held else None
    forms = RC.three_forms(*RC.solvable_lists(rng, 4, S, T, K), K)     # 4 games: both rings wrap
    want = RR.Ring(C, K)
    if held:
        IO.add_packed(want, *before)
    IO.add_packed(want, *forms["add_packed"])
    assert want.added == held + 4 and len(want.slots) == C and want.pointer == (held + 4) % C
    left = {}
    for entry in RC.ENTRIES:
        for select in (False, True) if entry != "add_packed" else (False,):
            buf = RC.guarded_buffer(C, K, T, S, DEV)
            if held:
                RC.call_entry("add_packed", buf, before)
            RC.call_entry(entry, buf, forms[entry], select, buf.status)
            left[entry, select] = RC.ring_of(buf)
            for name in RC.ARRAYS:
                check_flat(buf.guards[name], (entry, select, name))
            assert int(buf.status) == 0
    for (entry, select), ring in left.items():                         # (equal to one ring: equal pairwise)
        other = left["add", select]
        assert IO.rings_equal(ring, other), (entry, select)
        if not select:
            assert IO.rings_equal(ring, want), entry
    assert left["add", True].added == held + 1                         # the first shortest list = the best final reward


@pytest.mark.parametrize("entry", RC.ENTRIES)
def test_a_ring_pointer_outside_the_ring_is_folded_into_it(entry):
    """ring[0] outside [0, C) in a caller-owned descriptor: every entry takes it modulo C, so the call equals the one
    made from the folded value and nothing outside the six arrays is written."""
    C, N = 5, 7                                                        # 6 valid candidates: the ring wraps
    args = RC.edge_case(entry, N)
    for select in (False, True) if entry != "add_packed" else (False,):
        for raw in (-1, -C - 2, C, 3 * C + 1):
            want, status, _ = RC.restate(entry, args, C, raw % C, select)
            assert want.added == (1 if select else 6) and status
            bufs = [RC.guarded_buffer(C, RC.L, RC.T, RC.S, DEV) for _ in (0, 1)]
            for buf, first in zip(bufs, (raw, raw % C)):
                buf.ring[0] = first
                RC.call_entry(entry, buf, args, select, buf.status)
                assert_ring(buf, want, (select, raw, first))
                for name in RC.ARRAYS:
                    check_flat(buf.guards[name], (select, raw, first, name))
            for name in RC.ARRAYS + ("status",):                       # the poison outside the stored moves included
                x, y = getattr(bufs[0], name), getattr(bufs[1], name)
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (select, raw, name)


# ---- addressing ------------------------------------------------------------------------------------------------------
def odd(shape, dtype, offset):
    """(buffer, tensor of ``shape``) ``offset`` bytes behind GUARD canary bytes, more canaries behind it."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + offset + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD + offset:GUARD + offset + n].view(dtype).view(shape)


@pytest.mark.parametrize("S,T,off", [(5, 2, 1), (16, 4, 3), (25, 1, 7), (4, 2, 0)])
def test_addressing_at_odd_offsets_between_guards(S, T, off):
    K, M, Cc = 3, 5, 4
    rng = np.random.default_rng(S + off)
    starts, tokens, lengths, groups = make_lists(rng, S, T, K, M, 1, True)
    buf, want = GameBuffer(Cc, K + 1, T, S, DEV), RR.Ring(Cc, K + 1)   # the last move of every slot stays unwritten
    raws = {}
    for name, o in (("frames", off), ("tokens", off + 2), ("rewards", 4 * off)):
        raws[name], view = odd(getattr(buf, name).shape, getattr(buf, name).dtype, o)
        view.copy_(dev(rng.integers(-100, 100, size=tuple(view.shape)).astype(host(view).dtype)))
        setattr(buf, name, view)
    buf.desc = _lib.ReplayBufferDesc(buf.C, buf.L, buf.T, buf.S, *(t.data_ptr() for t in (
        buf.frames, buf.tokens, buf.rewards, buf.length, buf.offset, buf.ring)))
    raws["starts"], d_starts = odd(starts.shape, torch.int8, off + 1)
    raws["list tokens"], d_tokens = odd(tokens.shape, torch.int8, off + 4)
    raws["stored"], d_stored = odd((M,), torch.uint8, 1)
    d_starts.copy_(dev(starts)), d_tokens.copy_(dev(tokens))
    before = {n: host(getattr(buf, n)).copy() for n in ("frames", "tokens", "rewards")}
    ops.replay_add_lists(buf, d_starts, d_tokens, dev(lengths), dev(groups), stored=d_stored, status=buf.status)
    LR.add_lists(want, starts, tokens, lengths, groups)
    assert_ring(buf, want)
    assert int(buf.status) == 0 and want.added == M and host(d_stored).tolist() == [1] * M
    for name, raw in raws.items():
        lead = GUARD + {"frames": off, "tokens": off + 2, "rewards": 4 * off, "starts": off + 1, "list tokens": off + 4,
                        "stored": 1}[name]
        assert bool((raw[:lead] == CANARY).all()) and bool((raw[-GUARD:] == CANARY).all()), name
    length = host(buf.length)
    for name in ("frames", "tokens", "rewards"):                       # nothing behind a slot's length is written
        now = host(getattr(buf, name))
        for s in range(Cc):
            assert length[s] <= K and np.array_equal(now[s, length[s]:], before[name][s, length[s]:]), (name, s)


# ---- graph capture, empty calls --------------------------------------------------------------------------------------
def test_graph_capture_and_empty_calls():
    S, T, K, M = 5, 2, 3, 7
    rng = np.random.default_rng(21)
    starts, tokens, lengths, groups = make_lists(rng, S, T, K, M, 1, True)
    lengths[2] = 0
    d = [dev(starts), dev(tokens), dev(lengths), dev(groups)]
    eager, graphed = GameBuffer(4, K, T, S, DEV), GameBuffer(4, K, T, S, DEV)
    stored_e = [ops.replay_add_lists(eager, *d, status=eager.status).clone() for _ in range(2)]
    stored = torch.zeros((M,), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.replay_add_lists(GameBuffer(4, K, T, S, DEV), *d, stored=stored)  # warm-up on another buffer
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.replay_add_lists(graphed, *d, stored=stored, status=graphed.status)
    assert int(graphed.ring[1]) == 0                                   # captured, not run
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for n in ("frames", "tokens", "rewards", "length", "offset", "ring", "status"):
        assert torch.equal(getattr(graphed, n), getattr(eager, n)), n
    assert torch.equal(stored, stored_e[1]) and int(eager.ring[1]) == 12
    # M = 0 and G = 0 store nothing
    keep = [getattr(eager, n).clone() for n in ("frames", "tokens", "rewards", "length", "offset", "ring")]
    none = ops.replay_add_lists(eager, d[0], d[1][:0], d[2][:0], d[3][:0], status=eager.status)
    assert none.shape == (0,)
    no_group = ops.replay_add_lists(eager, d[0][:0], d[1], d[2], d[3], status=eager.status)
    assert not host(no_group).any() and int(eager.status) == 1 | 4
    for n, t in zip(("frames", "tokens", "rewards", "length", "offset", "ring"), keep):
        assert torch.equal(getattr(eager, n), t), n
    with pytest.raises(TensorGameError, match="groups"):
        ops.replay_add_lists(eager, d[0][:3], d[1], d[2])


# ---- the solution search into the dataset ----------------------------------------------------------------------------
def test_add_solutions_end_to_end_at_s4(tmp_path):
    S, R, G, n, T = 4, 5, 24, 2, 2
    demos = SyntheticDemos(R, G, T, S, DEV, seed=31)
    states = torch.zeros((G, T, S, S, S), dtype=torch.int8, device=DEV)
    states[:, 0] = demos.target_tensor
    states[:, 1] = torch.from_numpy(np.random.default_rng(1).integers(-2, 3, size=(G, S, S, S)).astype(np.int8)).to(DEV)
    scalars = torch.zeros((G, 1), device=DEV)
    null = torch.ones((3 * S,), dtype=torch.int8, device=DEV)
    plays = (torch.arange(G, device=DEV) % 3 != 1)                     # the other groups only play null actions
    hard = demos.target_tensor.flatten(1).any(1)                       # (a target that is zero already never counts)

    def policy(frames, scal, rows, step):  # a group's samples un-do its demonstration, last action first, or play nulls
        g = rows // n
        return torch.where(plays[g][:, None], demos.action_seq[g, R - 1 - step], null[None]).contiguous()

    res = rollout.solve_states(policy, states, scalars, n, R, chunk_groups=10)
    solved = host(res.groups)
    assert 0 < len(solved) < G and not set(solved) & set(host(torch.nonzero(~plays & hard).flatten()).tolist())
    data = TensorGameData.from_demos(demos, 32, 0.5, seed=2, played_capacity=G + 2, best_capacity=2, max_actions=R)
    stored = data.add_solutions(res, states)
    want_played, want_best = RR.Ring(G + 2, R), RR.Ring(2, R)
    args = [host(states), host(res.tokens), host(res.lengths), solved, 1]
    want_stored, status = LR.add_lists(want_played, *args)
    LR.add_lists(want_best, *args, select=True)
    assert status == 0 and host(stored).tolist() == want_stored.tolist() == [1] * len(solved)
    assert_ring(data.played, want_played)
    assert_ring(data.best, want_best)
    assert want_best.added == 1 and len(want_best.slots[0][2]) == int(res.lengths.min())
    assert data.played.games_added() == len(solved) and int(data.played.status) == int(data.best.status) == 0
    # the archive proves the same lists
    rep = SolutionArchive(S=S, max_rank=16, capacity=256, device=DEV).add_result(res, states)
    assert host(rep.proven).tolist() == host(stored).astype(bool).tolist()
    # the batches of the next epoch hold their moves
    data.resample_buffer_indexes()
    kinds = host(data.kind)
    assert (kinds == RR.PLAYED).any()
    seen = 0
    for state, scalar, action, reward in data.batches(8, shuffle=False):
        lo = seen
        seen += state.shape[0]
        for x in np.nonzero(kinds[lo:seen] == RR.PLAYED)[0]:
            f, sc, a, r = want_played.getitem(int(data.src[lo + x]))
            assert np.array_equal(host(state[x]), f.astype(np.float32)) and float(scalar[x]) == sc
            assert np.array_equal(host(action[x]), a) and float(reward[x]) == r
    assert seen == 32 and int(data.status) == 0
    # a saved run gives the games back
    cfg = dict(CONFIGS["b"], dim_3d=4, n_steps=12)
    tr = FusedTrainer.from_state_dict(make_weights(cfg, 41), dropout_p=0.0, seed=6, device=DEV)
    replay_io.save_run(tmp_path / "run", tr, None, data)
    back = replay_io.load_run(tmp_path / "run", DEV).data
    idx = torch.arange(len(data.played), device=DEV)
    for x, y in zip(back.played.items(idx), data.played.items(idx)):
        assert torch.equal(x, y)
    assert_ring(back.played, want_played)
    assert_ring(back.best, want_best)
    # refusals name the argument
    with pytest.raises(TensorGameError, match="states"):
        data.add_solutions(res, states[:, :1])
    with pytest.raises(TensorGameError, match="shift"):
        TensorGameData.from_demos(demos, 32, 0.5, shift=2, max_actions=R).add_solutions(
            rollout.sample_rollouts(policy, states, scalars, n, R), states)
    with pytest.raises(TensorGameError, match="max_actions"):
        TensorGameData.from_demos(demos, 32, 0.5, max_actions=R - 1).add_solutions(res, states)
