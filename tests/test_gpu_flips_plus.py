"""GPU checks of the plus transitions (include/tensor_game_flips_plus.h): ``ops.flip_advance_plus`` bit for bit against
the host restatement (flips_plus_ref.py) on all nine state tensors, in unaligned, canary-guarded buffers; the exact proof
of every walk's lists, which does not go through the restatement; the cap and the last slot at one and at two terms per
lane; plus_slack = 0 against ``ops.flip_advance``; continuation, sharding and the Philox words; odd sizes; walks that
are not walked; more walks than workgroups; ``FlipWalks`` and ``reduce_archive`` with plus; graph capture."""
import io

import numpy as np
import pytest
import torch

from mat_mul_amd import FlipWalks, SolutionArchive, flips, ops, reduce_archive

import flips_ref as FR
import flips_plus_ref as PR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


class Guarded:
    """The nine state tensors in guarded buffers (the two lists one byte behind an aligned allocation), filled from a
    host state, and the check that the guards survived."""

    def __init__(self, host):
        self.bufs, self.st = {}, {}
        for name, dtype in ops._FLIP_PLUS_STATE:
            x = dev(host[name])
            assert x.dtype == dtype, name
            if dtype == torch.int8:
                n = x.numel()
                buf = torch.full((GUARD + 1 + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
                view = buf[GUARD + 1:GUARD + 1 + n].view(torch.int8).view(x.shape)
                assert view.data_ptr() % 16 == 1
            else:
                buf, view = guarded(tuple(x.shape), dtype)
            view.copy_(x)
            self.bufs[name], self.st[name] = buf, view

    def check(self):
        for name, buf in self.bufs.items():
            if self.st[name].dtype == torch.int8:
                n = self.st[name].numel()
                assert bool((buf[:GUARD + 1] == CANARY).all()) and bool((buf[GUARD + 1 + n:] == CANARY).all()), name
            else:
                check_flat(buf, name)

    def advance(self, n_steps, plus_after, plus_slack, bound, seed, walk0=0, step0=0):
        ops.flip_advance_plus(self.st, n_steps, plus_after, plus_slack, bound=bound, shift=bound, seed=seed, walk0=walk0,
                              step0=step0)
        self.check()
        return to_np(self.st)


def to_np(st, names=PR.STATE_NAMES):
    return {k: st[k].cpu().numpy() for k in names}


def assert_state(got, want, what="", names=PR.STATE_NAMES):
    for k in names:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[:8])


def assert_proven(tokens, L, shift, st):
    """Independent of the restatement: every walk's cur and best list is a proven factorisation of what the start list
    sums to, of rank cur_rank and best_rank."""
    W = st["cur"].shape[0]
    target = flips.term_sum(dev(tokens[None]), dev(np.array([L], dtype=np.int64)), shift).expand(W, -1, -1, -1).contiguous()
    for rows, rank in (("best", "best_rank"), ("cur", "cur_rank")):
        _, canon_rank, _, res = ops.solution_canon(target, st[rows].contiguous(), st[rank].to(torch.int64), shift=shift)
        assert bool((res == 0).all()) and torch.equal(canon_rank, st[rank]), rows


# ---- the cases of the table: bit for bit against the restatement -----------------------------------------------------
@pytest.mark.parametrize("name", list(PR.CASES))
def test_advance_plus_equals_the_restatement(name):
    """2x2 and 3x3; the inert list; the cap and slot 63 at one term per lane; the append into slot 64 (a lane's second
    slot) at K = 65 and K = 128; slot 127.  test_flips_plus_cpu.py asserts the events each case reaches."""
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, must = PR.CASES[name]
    tokens, L, st, want, events = PR.case_ref(name)
    for e in must:
        assert events[e] >= PR.MIN_EVENTS, (e, events[e])
    g = Guarded(st)
    got = g.advance(n_steps, plus_after, plus_slack, bound, seed)
    assert_state(got, want, name)
    assert_proven(tokens, L, bound, g.st)
    if name != "inert full":
        assert (got["pluses"] > 0).all() and (got["state"] == 0).all()


def test_begin_on_the_device_gives_the_start_states_of_the_cases():
    for name in ("2x2", "slot64 K128"):
        kind, S, K, L, bound, W = PR.CASES[name][:6]
        tokens, L, st = PR.start_state(name)
        got = ops.flip_begin(dev(tokens[None]), dev(np.array([L], dtype=np.int64)), src=torch.zeros(W, dtype=torch.int64, device=DEV),
                             bound=bound, shift=bound)
        assert_state(to_np(got, FR.STATE_NAMES), st, name, FR.STATE_NAMES)


def test_an_inert_list_is_stuck_under_the_plain_entry_and_walks_on_under_plus():
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES["inert"]
    tokens, L, st, want, _ = PR.case_ref("inert")
    plain = {k: dev(st[k]) for k in FR.STATE_NAMES}
    ops.flip_advance(plain, n_steps, bound=bound, shift=bound, seed=seed)
    assert bool((plain["state"] == 1).all()) and not bool(plain["flips"].any())
    assert torch.equal(plain["cur"], dev(st["cur"]))
    got = Guarded(st).advance(n_steps, plus_after, plus_slack, bound, seed)
    assert (got["pluses"] > 0).all() and (got["state"] == 0).all() and (got["flips"] > 0).any()


def test_walks_the_plain_entry_leaves_stuck_on_7_terms_move_on(golden):
    """Strassen's list has no match: the plain entry stops there, the new one takes a forced plus and goes on."""
    tokens = np.zeros((9, 12), dtype=np.int8)
    tokens[:7] = golden("strassen")["tokens"]
    W, n_steps = 16, 200
    begun, status = FR.begin(tokens[None], [7], np.zeros(W, dtype=np.int64), 1, 1)
    assert status == 0 and (begun["cur_rank"] == 7).all()
    plain = {k: dev(begun[k]) for k in FR.STATE_NAMES}
    ops.flip_advance(plain, n_steps, bound=1, shift=1, seed=3)
    assert bool((plain["state"] == 1).all()) and torch.equal(plain["cur"], dev(begun["cur"]))
    st = PR.with_plus(begun)
    want = PR.advance(PR.copy_state(st), 3, 0, 0, n_steps, 1, 1, 1000, 2)
    g = Guarded(st)
    got = g.advance(n_steps, 1000, 2, 1, 3)
    assert_state(got, want)
    assert (got["pluses"] > 0).all() and (got["flips"] > 0).all() and (got["best_rank"] == 7).all()
    assert_proven(tokens, 7, 1, g.st)


# ---- plus_slack = 0 and a plus_after that never comes: the plain walks -----------------------------------------------
def test_plus_slack_0_equals_flip_advance_stuck_walks_included():
    tokens, L = FR.standard_matmul(2)
    begun, _ = FR.begin(tokens[None], [L], np.zeros(8, dtype=np.int64), 1, 1)
    plain = {k: dev(begun[k]) for k in FR.STATE_NAMES}
    ops.flip_advance(plain, 1500, bound=1, shift=1, seed=0)       # walks 5, 6 and 7 reach rank 7 and are stuck
    assert plain["state"].cpu().tolist()[5:] == [1, 1, 1]
    st = PR.with_plus(begun)
    st["pluses"][:] = 5
    g = Guarded(st)
    got = g.advance(1500, 1, 0, 1, 0)
    assert_state(got, to_np(plain, FR.STATE_NAMES), "slack 0", FR.STATE_NAMES)
    assert (got["pluses"] == 5).all() and (got["since"][:5] > 0).all()


def test_a_plus_after_that_never_comes_equals_flip_advance():
    tokens, L = FR.standard_matmul(3, K=30)
    begun, _ = FR.begin(tokens[None], [L], np.zeros(8, dtype=np.int64), 1, 1)
    plain = {k: dev(begun[k]) for k in FR.STATE_NAMES}
    ops.flip_advance(plain, 200, bound=1, shift=1, seed=4)
    assert not bool(plain["state"].any())                          # nothing gets stuck
    got = Guarded(PR.with_plus(begun)).advance(200, 2 ** 31 - 1, 3, 1, 4)
    assert_state(got, to_np(plain, FR.STATE_NAMES), "never", FR.STATE_NAMES)
    assert not got["pluses"].any() and (got["since"] > 0).all()


# ---- continuation, sharding, the Philox words ------------------------------------------------------------------------
def test_continuation_37_then_91_equals_128():
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES["slot64 K128"]
    tokens, L, st, want, _ = PR.case_ref("slot64 K128")
    assert n_steps == 128
    g = Guarded(st)
    mid = g.advance(37, plus_after, plus_slack, bound, seed)
    assert (mid["pluses"] > 0).all()                               # since and pluses are carried
    got = g.advance(91, plus_after, plus_slack, bound, seed, step0=37)
    assert_state(got, want)


@pytest.mark.parametrize("walk0, step0, n_steps", [(0, 37, 100), (5, 63, 2), ((1 << 40) + 5, 1000, 70), (2 ** 32 - 3, 0, 65),
                                                   (0, 2 ** 32 - 70, 70)])
def test_walk_ids_and_steps_reach_the_three_philox_words(walk0, step0, n_steps):
    """step0 is no multiple of 64 and the launches end inside a block of draws: o.x, o.y and o.z of step t sit in the
    lane the step reads; the id's high word and its wrap reach the counter."""
    tokens, L, st = PR.start_state("inert")
    st = {k: v[:8] for k, v in st.items()}
    want = PR.advance(PR.copy_state(st), 9, walk0, step0, n_steps, 2, 2, 3, 2)
    got = Guarded(st).advance(n_steps, 3, 2, 2, 9, walk0=walk0, step0=step0)
    assert_state(got, want, (walk0, step0, n_steps))
    assert got["pluses"].sum() > 0


def test_sharding_two_halves_equal_the_whole():
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES["2x2"]
    tokens, L, st, want, _ = PR.case_ref("2x2")
    for lo in (0, 32):
        part = {k: v[lo:lo + 32] for k, v in st.items()}
        got = Guarded(part).advance(n_steps, plus_after, plus_slack, bound, seed, walk0=lo)
        assert_state(got, {k: v[lo:lo + 32] for k, v in want.items()}, lo)


# ---- odd sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, K, L", [(3, 12, 8), (16, 16, 10), (25, 15, 9), (32, 16, 10)])
def test_sizes_equal_the_restatement(S, K, L):
    """Partly filled dwords (S = 3, 25), whole ones (16, 32) and TG_MAX_S; values in {-1, 0, 1} under bound 2."""
    W, n_steps, bound = 8, 32, 2
    tokens, L = FR.pool_list(np.random.default_rng(S), S, K, L, 4, bound, nnz=min(S, 3))
    begun, status = FR.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), bound, bound)
    assert status == 0
    st = PR.with_plus(begun)
    want = PR.advance(PR.copy_state(st), 1, 0, 0, n_steps, bound, bound, 3, 4)
    assert want["pluses"].sum() >= PR.MIN_EVENTS and want["flips"].sum() >= PR.MIN_EVENTS
    g = Guarded(st)
    got = g.advance(n_steps, 3, 4, bound, 1)
    assert_state(got, want, S)
    assert_proven(tokens, L, bound, g.st)


# ---- walks that are not walked ---------------------------------------------------------------------------------------
def test_walks_with_a_state_or_a_rank_outside_0_K_are_left_as_they_are():
    tokens, L, st = PR.start_state("inert")
    st = {k: v[:8].copy() for k, v in st.items()}
    K = st["cur"].shape[1]
    st["state"][1], st["state"][2] = 1, -1
    st["cur_rank"][4], st["cur_rank"][6] = K + 1, -1
    idle = [1, 2, 4, 6]
    for w in idle:
        st["cur"][w], st["best"][w] = 0x55, 0x33
        st["since"][w], st["pluses"][w], st["flips"][w], st["best_step"][w] = 11 + w, 100 + w, 7, 9
    want = PR.advance(PR.copy_state(st), 2, 0, 0, 40, 2, 2, 3, 2)
    got = Guarded(st).advance(40, 3, 2, 2, 2)
    for k in PR.STATE_NAMES:
        assert np.array_equal(got[k][idle], st[k][idle]), k
    assert_state(got, want)
    assert (got["pluses"][[0, 3, 5, 7]] > 0).all()


# ---- more walks than workgroups ---------------------------------------------------------------------------------------
def test_a_workgroup_loops_over_walks():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    W = 32 * cus + 77
    tokens, L, one = PR.start_state("inert")
    st = {k: np.repeat(v[:1], W, axis=0) for k, v in one.items()}
    st["state"][5::7] = 1                                          # and some that are left alone
    whole = Guarded(st).advance(4, 1000, 2, 2, 6)
    sample = np.concatenate([np.arange(40), np.arange(W - 24, W)])
    part = {k: v[sample] for k, v in st.items()}
    for i, w in enumerate(sample):                                 # the restatement of 64 walks, each under its own id
        row = {k: v[i:i + 1] for k, v in part.items()}
        PR.advance(row, 6, int(w), 0, 4, 2, 2, 1000, 2)
    assert_state({k: v[sample] for k, v in whole.items()}, part, "sample")
    assert whole["pluses"].sum() > W // 2 and not whole["pluses"][st["state"] == 1].any()
    lo = 32 * cus - 100                                            # a second run, sharded across the grid's edge
    for a, b in ((0, lo), (lo, W)):
        got = Guarded({k: v[a:b] for k, v in st.items()}).advance(4, 1000, 2, 2, 6, walk0=a)
        assert_state(got, {k: v[a:b] for k, v in whole.items()}, (a, b))


# ---- FlipWalks and reduce_archive ------------------------------------------------------------------------------------
def test_flipwalks_with_plus_round_trip_continues_bit_for_bit():
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES["3x3"]
    tokens, L, st, want, _ = PR.case_ref("3x3")
    lists, lengths = dev(tokens[None]), dev(np.array([L], dtype=np.int64))
    start = dict(walks_per_list=W, bound=bound, shift=bound, seed=seed, plus_after=plus_after, plus_slack=plus_slack)
    whole = FlipWalks.start(lists, lengths, **start).advance(n_steps)
    assert_state(to_np(whole._st), want)
    assert whole.since is whole._st["since"] and whole.pluses is whole._st["pluses"] and int(whole.pluses.sum()) > 0
    part = FlipWalks.start(lists, lengths, **start).advance(100)
    f = io.BytesIO()
    torch.save({"flips": part.state_dict()}, f)
    f.seek(0)
    sd = torch.load(f, weights_only=True)["flips"]
    assert sd["version"] == flips.STATE_VERSION_PLUS == 2 and (sd["plus_after"], sd["plus_slack"]) == (plus_after, plus_slack)
    back = FlipWalks.from_state_dict(sd, DEV)
    assert (back.steps_done, back.plus_after, back.plus_slack) == (100, plus_after, plus_slack)
    back.advance(n_steps - 100)
    assert_state(to_np(back._st), want)


def test_plain_flipwalks_keep_version_1_and_their_keys():
    tokens, L = FR.standard_matmul(2)
    walks = FlipWalks.start(dev(tokens[None]), dev(np.array([L], dtype=np.int64)), walks_per_list=4).advance(10)
    sd = walks.state_dict()
    assert sd["version"] == flips.STATE_VERSION == 1 and walks.plus_after is None
    assert set(sd) == {"version", "bound", "shift", "seed", "walk0", "steps_done", "status", "src", *FR.STATE_NAMES}
    with pytest.raises(AttributeError):
        walks.since
    back = FlipWalks.from_state_dict(sd, DEV)
    assert back.plus_after is None and set(back._st) == set(FR.STATE_NAMES)


def test_reduce_archive_with_plus_adds_only_what_is_proven():
    std, L = FR.standard_matmul(2, K=9)
    arch = SolutionArchive(S=4, max_rank=9, capacity=64, device=DEV, shift=1)
    lists, lengths = dev(std[None]), dev(np.array([L], dtype=np.int64))
    target = flips.term_sum(lists, lengths, 1)
    rep = arch.add(target, lists, lengths)
    assert bool(rep.proven[0]) and int(arch.lowest_rank) == 8
    entry = arch.entries()[0].cpu().numpy()
    begun, _ = FR.begin(entry, [8], np.zeros(8, dtype=np.int64), 1, 1)
    want = PR.advance(PR.with_plus(begun), 0, 0, 0, 1500, 1, 1, 16, 2)
    rep, walks = reduce_archive(arch, 1500, walks_per_entry=8, seed=0, plus_after=16, plus_slack=2)
    assert_state(to_np(walks._st), want)
    assert int(walks.pluses.sum()) > 0 and bool(rep.proven.all())
    assert int(arch.lowest_rank) <= 8 and int(arch.lowest_rank) == min(8, int(want["best_rank"].min()))
    tokens, rank, _, _ = arch.entries()
    assert torch.equal(flips.term_sum(tokens.contiguous(), rank.to(torch.int64), 1), target.expand(len(rank), 4, 4, 4))


# ---- capture ---------------------------------------------------------------------------------------------------------
def test_a_captured_graph_of_the_entry_replays_to_the_eager_result():
    """One kernel node, no parallel branches."""
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES["inert"]
    tokens, L, st, want, _ = PR.case_ref("inert")
    g = Guarded(st)
    start = {k: v.clone() for k, v in g.st.items()}

    def call():
        ops.flip_advance_plus(g.st, n_steps, plus_after, plus_slack, bound=bound, shift=bound, seed=seed)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()                                                     # warm-up, off the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert_state(to_np(g.st), want, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k, v in start.items():
        g.st[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    g.check()
    assert_state(to_np(g.st), want, "replay")
