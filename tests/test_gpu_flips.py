"""GPU checks of the flip-graph walks (include/tensor_game_flips.h): ``ops.flip_begin`` and ``ops.flip_advance`` bit for
bit against the host restatement (flips_ref.py) on unaligned, canary-guarded buffers; continuation, sharding, stuck and
bad walks; the exact proof of every walk's best list, which does not go through the restatement; ``FlipWalks`` and
``reduce_archive``; gadget lists that reach the rule events plausible lists do not (null terms, cancels, merges, moves
between a lane's two slots); S = 16, 25, 32 and S < 4; more walks than workgroups; the Philox words and step tails; the
cur_rank guard and graph capture."""
import io

import numpy as np
import pytest
import torch

from mat_mul_amd import FlipWalks, SolutionArchive, SymmetryGroup, flips, ops, reduce_archive

import flips_ref as FR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0   # the seed test_flips_cpu.py chose: walks from the standard <2,2,2> list reach rank 7 with it


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def odd(x):
    """A copy of int8 ``x`` one byte behind an aligned allocation (with canaries around it): (buffer, view)."""
    n = x.numel()
    buf = torch.full((GUARD + 1 + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + 1:GUARD + 1 + n].view(torch.int8).view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 1
    return buf, view


class Guarded:
    """The seven state tensors in guarded buffers (the two lists unaligned), and the check that the guards survived."""

    def __init__(self, W, K, S):
        self.bufs, self.st = {}, {}
        for name, dtype in ops._FLIP_STATE:
            if dtype == torch.int8:
                self.bufs[name], self.st[name] = odd(torch.zeros((W, K, 3 * S), dtype=torch.int8, device=DEV))
            else:
                self.bufs[name], self.st[name] = guarded((W,), dtype)

    def check(self):
        for name, buf in self.bufs.items():
            if self.st[name].dtype == torch.int8:
                n = self.st[name].numel()
                assert bool((buf[:GUARD + 1] == CANARY).all()) and bool((buf[GUARD + 1 + n:] == CANARY).all()), name
            else:
                check_flat(buf, name)


def to_np(st):
    return {k: st[k].cpu().numpy() for k in FR.STATE_NAMES}


def assert_state(got, want, what=""):
    for k in FR.STATE_NAMES:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[:8])


def gpu_begin(tokens, lengths, src, bound, shift):
    """(Guarded, status bits) of ``ops.flip_begin`` on unaligned inputs and guarded outputs."""
    M, K, A3 = tokens.shape
    W = M if src is None else len(src)
    g = Guarded(W, K, A3 // 3)
    _, tok = odd(dev(tokens))
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.flip_begin(tok, dev(np.asarray(lengths, dtype=np.int64)), src=None if src is None else dev(np.asarray(src, np.int64)),
                         bound=bound, shift=shift, status=status, **g.st)
    assert all(out[k] is g.st[k] for k in FR.STATE_NAMES)
    g.check()
    return g, int(status.cpu().view(torch.int32).item())


def gpu_advance(g, n_steps, bound, shift, seed, walk0=0, step0=0):
    ops.flip_advance(g.st, n_steps, bound=bound, shift=shift, seed=seed, walk0=walk0, step0=step0)
    g.check()
    return to_np(g.st)


def assert_proven(tokens, lengths, src, shift, st, reduced=True):
    """Independent of the restatement: every walk's best list is a proven factorisation of what its start list sums to,
    of rank best_rank.  (``reduced=False``: a hand-written list that holds a term and its negative -- the canonical
    form drops such a pair, so its rank is not the list's; the sum is still proven.)"""
    targets = flips.term_sum(dev(tokens), dev(np.asarray(lengths, np.int64)), shift)
    idx = torch.arange(len(lengths), device=DEV) if src is None else dev(np.asarray(src, np.int64))
    good = st["state"] >= 0
    _, rank, _, res = ops.solution_canon(targets[idx].contiguous(), st["best"].contiguous(), st["best_rank"].to(torch.int64),
                                         shift=shift)
    assert bool((res[good] == 0).all()) and (not reduced or torch.equal(rank[good], st["best_rank"][good]))
    _, rank, _, res = ops.solution_canon(targets[idx].contiguous(), st["cur"].contiguous(), st["cur_rank"].to(torch.int64),
                                         shift=shift)
    assert bool((res[good] == 0).all()) and (not reduced or torch.equal(rank[good], st["cur_rank"][good]))


# ---- begin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, K", [(4, 8), (5, 7), (9, 27), (4, 64), (4, 65), (5, 128)])
def test_begin_on_planted_lists(S, K):
    bound = shift = 1 + S % 2
    rng = np.random.default_rng(100 * S + K)
    M = 8
    tokens = np.zeros((M, K, 3 * S), dtype=np.int8)
    lengths = np.full(M, K, dtype=np.int64)
    for m in range(6):
        tokens[m] = FR.planted_list(rng, S, K, bound, shift, rot=m)[0]
    tokens[6] = FR.planted_list(rng, S, K, bound, shift, rot=2)[0]
    lengths[6] = K // 2                                           # the rows behind the length are not read
    tokens[6, K // 2:] = 127
    lengths[7] = 0                                                # an empty list
    src = np.array([7, 0, 0, 3, 1, 2, 4, 5, 6, 2, 5], dtype=np.int64)   # repeats, W != M
    want, wstatus = FR.begin(tokens, lengths, src, bound, shift)
    assert wstatus == 0 and (want["cur_rank"][1:8] < lengths[src[1:8]]).all()      # every planted list lost terms
    assert want["cur_rank"][0] == 0 and want["state"][0] == 0
    g, status = gpu_begin(tokens, lengths, src, bound, shift)
    assert status == 0
    assert_state(to_np(g.st), want, (S, K))
    assert_proven(tokens, lengths, src, shift, g.st)
    g2, status = gpu_begin(tokens, lengths, None, bound, shift)   # src = NULL: walk w starts from list w
    assert status == 0
    assert_state(to_np(g2.st), FR.begin(tokens, lengths, None, bound, shift)[0], (S, K, "no src"))


# ---- advance ---------------------------------------------------------------------------------------------------------
def _start_lists(case):
    rng = np.random.default_rng(7)
    if case == "2x2":
        return (*FR.standard_matmul(2), 4, 64, 512, 1, 1)
    if case == "3x3":
        return (*FR.standard_matmul(3), 9, 16, 256, 1, 1)
    if case == "pool70":                                          # matches are plentiful
        return (*FR.pool_list(rng, 5, 70, 70, 4, 2), 5, 8, 128, 2, 2)
    return (*FR.pool_list(rng, 5, 128, 128, 40, 2), 5, 4, 64, 2, 2)   # "pool128": both of a lane's slots stay live


_REF = {}


def advanced_ref(case):
    """(tokens, L, S, W, n_steps, bound, shift, restatement's state after n_steps, its trace) -- computed once."""
    if case not in _REF:
        tokens, L, S, W, n_steps, bound, shift = _start_lists(case)
        st, status = FR.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), bound, shift)
        assert status == 0
        trace = []
        FR.advance(st, SEED, 0, 0, n_steps, bound, shift, trace=trace)
        _REF[case] = (tokens, L, S, W, n_steps, bound, shift, st, trace)
    return _REF[case]


@pytest.mark.parametrize("case", ["2x2", "3x3", "pool70", "pool128"])
def test_advance_equals_the_restatement(case):
    tokens, L, S, W, n_steps, bound, shift, want, trace = advanced_ref(case)
    assert {v for _, _, v, _ in trace} == set(range(8))                               # all eight variants were drawn
    assert {a for _, _, _, a in trace} == {False, True}                               # accepted and refused flips
    if case == "pool128":
        assert want["cur_rank"].min() > 64
    src = np.zeros(W, dtype=np.int64)
    g, status = gpu_begin(tokens[None], [L], src, bound, shift)
    assert status == 0
    got = gpu_advance(g, n_steps, bound, shift, SEED)
    assert_state(got, want, case)
    assert_proven(tokens[None], [L], src, shift, g.st)


def test_continuation_100_then_156_equals_256():
    tokens, L, S, W, n_steps, bound, shift, want, _ = advanced_ref("3x3")
    g, _ = gpu_begin(tokens[None], [L], np.zeros(W, dtype=np.int64), bound, shift)
    gpu_advance(g, 100, bound, shift, SEED)
    got = gpu_advance(g, 156, bound, shift, SEED, step0=100)
    assert_state(got, want)


def test_sharding_two_halves_equal_the_whole():
    tokens, L, S, W, n_steps, bound, shift, want, _ = advanced_ref("2x2")
    for lo in (0, 32):
        g, _ = gpu_begin(tokens[None], [L], np.zeros(32, dtype=np.int64), bound, shift)
        got = gpu_advance(g, n_steps, bound, shift, SEED, walk0=lo)
        assert_state(got, {k: v[lo:lo + 32] for k, v in want.items()}, lo)


# ---- stuck and bad walks ---------------------------------------------------------------------------------------------
def test_strassen_is_stuck_and_a_walk_that_reaches_rank_7_stays_frozen(golden):
    gs = golden("strassen")
    tokens = np.zeros((1, 8, 12), dtype=np.int8)
    tokens[0, :7] = gs["tokens"]
    g, status = gpu_begin(tokens, [7], None, 1, 1)
    before = to_np(g.st)
    assert status == 0 and before["cur_rank"][0] == 7 and before["state"][0] == 0
    after = gpu_advance(g, 50, 1, 1, SEED)
    assert after["state"][0] == 1                                                     # C = 0
    for k in FR.STATE_NAMES[:-1]:
        assert np.array_equal(after[k], before[k]), k
    # walks 5, 6 and 7 reach rank 7 inside the first launch (after 1097, 1392 and 942 steps)
    std, L = FR.standard_matmul(2)
    want, _ = FR.begin(std[None], [L], np.zeros(8, dtype=np.int64), 1, 1)
    FR.advance(want, SEED, 0, 0, 1500, 1, 1)
    assert (want["state"][5:] == 1).all() and (want["best_step"][5:] < 1500).all() and (want["state"][:2] == 0).all()
    g, _ = gpu_begin(std[None], [L], np.zeros(8, dtype=np.int64), 1, 1)
    got = gpu_advance(g, 1500, 1, 1, SEED)
    assert_state(got, want)
    again = gpu_advance(g, 200, 1, 1, SEED, step0=1500)                               # and the next launch
    frozen = got["state"] == 1
    for k in FR.STATE_NAMES:
        assert np.array_equal(again[k][frozen], got[k][frozen]), k
    assert (again["flips"][~frozen] > got["flips"][~frozen]).all()


def test_bad_rows_set_their_bit_and_touch_nothing_else():
    S, K, bound, shift = 4, 8, 1, 1
    std, L = FR.standard_matmul(2)
    tokens = np.repeat(std[None], 4, axis=0)
    good, _ = FR.begin(tokens, [L] * 4, None, bound, shift)
    for lengths, src, edit, bit, bad in (
            ([L, K + 1, L, -1], None, None, FR.BAD_LENGTH, [1, 3]),
            ([L] * 4, [0, 4, 1, -1, 2], None, FR.BAD_SRC, [1, 3]),
            ([L] * 4, None, (2, 5, 3, 2 + shift), FR.BAD_RANGE, [2]),                 # a value of 2 at bound 1
            ([L] * 4, None, (2, 5, 3, -2 + shift), FR.BAD_RANGE, [2])):
        tok = tokens.copy()
        if edit:
            tok[edit[:3]] = edit[3]
        want, wstatus = FR.begin(tok, lengths, src, bound, shift)
        assert wstatus == bit and list(np.flatnonzero(want["state"] == -1)) == bad
        g, status = gpu_begin(tok, lengths, src, bound, shift)
        got = to_np(g.st)
        assert status == bit
        assert_state(got, want, bit)
        ok = got["state"] == 0
        assert not got["cur"][~ok].any() and not got["cur_rank"][~ok].any() and (got["cur"][ok] == good["cur"][0]).all()
        # advance leaves a -1 walk exactly as it is (whatever its rows hold) and walks the others
        g.st["cur"][bad[0]].fill_(3)
        marked = to_np(g.st)
        FR.advance(want, SEED, 0, 0, 64, bound, shift)
        after = gpu_advance(g, 64, bound, shift, SEED)
        for k in FR.STATE_NAMES:
            assert np.array_equal(after[k][~ok], marked[k][~ok]), k
            assert np.array_equal(after[k][ok], want[k][ok]), k
    # the bits are sticky: a status that holds one keeps it
    status = torch.full((1,), 8, dtype=torch.int32, device=DEV).view(torch.uint32)
    ops.flip_begin(dev(tokens), dev(np.array([L, K + 1, L, L])), status=status)
    assert int(status.cpu().view(torch.int32).item()) == 8 | FR.BAD_LENGTH


# ---- FlipWalks and reduce_archive ------------------------------------------------------------------------------------
def test_flipwalks_state_dict_round_trip_continues_bit_for_bit():
    tokens, L, S, W, n_steps, bound, shift, want, _ = advanced_ref("3x3")
    lists, lengths = dev(tokens[None]), dev(np.array([L]))
    whole = FlipWalks.start(lists, lengths, walks_per_list=W, bound=bound, shift=shift, seed=SEED).advance(n_steps)
    assert whole.steps_done == n_steps and whole.W == W and not bool(whole.src.any())
    assert_state(to_np(whole._st), want)
    part = FlipWalks.start(lists, lengths, walks_per_list=W, bound=bound, shift=shift, seed=SEED).advance(100)
    f = io.BytesIO()
    torch.save({"flips": part.state_dict()}, f)
    f.seek(0)
    back = FlipWalks.from_state_dict(torch.load(f, weights_only=True)["flips"], DEV)
    assert back.steps_done == 100 and (back.bound, back.shift, back.seed, back.walk0) == (bound, shift, SEED, 0)
    back.advance(n_steps - 100)
    assert_state(to_np(back._st), want)
    assert torch.equal(back.src, whole.src) and back.steps_done == n_steps


def test_flipwalks_advance_70000_takes_two_launches():
    std, L = FR.standard_matmul(2, shift=2)                      # at bound 2 some walks are still walking after 70 000 steps
    walks = FlipWalks.start(dev(std[None]), dev(np.array([L])), walks_per_list=4, bound=2, shift=2, seed=SEED)
    walks.advance(70000)
    assert walks.steps_done == 70000
    want, _ = FR.begin(std[None], [L], np.zeros(4, dtype=np.int64), 2, 2)
    FR.advance(want, SEED, 0, 0, 65536, 2, 2)
    FR.advance(want, SEED, 0, 65536, 70000 - 65536, 2, 2)
    assert list(want["best_rank"]) == [7, 7, 7, 8] and list(want["state"]) == [1, 1, 1, 0]   # walk 3 walks all the way
    assert_state(to_np(walks._st), want)


@pytest.mark.parametrize("with_group", [False, True])
def test_reduce_archive_lowers_the_standard_algorithm_to_rank_7(with_group):
    std, L = FR.standard_matmul(2, K=8)
    group = SymmetryGroup.matmul(2, DEV) if with_group else None
    arch = SolutionArchive(S=4, max_rank=8, capacity=64, device=DEV, shift=1, group=group)
    lists, lengths = dev(std[None]), dev(np.array([L]))
    target = flips.term_sum(lists, lengths, 1)
    rep = arch.add(target, lists, lengths)
    assert bool(rep.proven[0]) and bool(rep.fresh[0]) and int(arch.count) == 1 and int(arch.lowest_rank) == 8
    # the restatement from the archive's own entry: which of the 8 walks reach rank 7
    entry = arch.entries()[0].cpu().numpy()
    want, _ = FR.begin(entry, [8], np.zeros(8, dtype=np.int64), 1, 1)
    FR.advance(want, SEED, 0, 0, 3000, 1, 1)
    assert want["best_rank"].min() == 7
    rep, walks = reduce_archive(arch, 3000, walks_per_entry=8, seed=SEED)
    assert_state(to_np(walks._st), want)
    assert int(arch.lowest_rank) == 7 and int(arch.count) > 1
    fresh = rep.fresh.cpu().numpy()
    assert fresh.any() and bool(rep.proven.all()) and (rep.rank.cpu().numpy()[fresh] == 7).all()
    assert not fresh[want["best_rank"] == 8].any()                                    # the entry itself is not new
    tokens, rank, _, _ = arch.entries()
    assert torch.equal(flips.term_sum(tokens.contiguous(), rank.to(torch.int64), 1), target.expand(len(rank), 4, 4, 4))


# ---- the rule events: gadget lists whose slots decide the branch (flips_ref.GADGET_CASES) -----------------------------
@pytest.mark.parametrize("name", list(FR.GADGET_CASES))
def test_gadget_walks_equal_the_restatement(name):
    """Null a' and b' with the hi/lo removal order, cancelling pairs and merges inside a walk, moves between a lane's
    two slots: test_flips_cpu.py asserts that the restatement reaches each at least MIN_EVENTS times on this list."""
    tokens, L, W, n_steps, want, events = FR.gadget_ref(name)
    for e in FR.ALWAYS + FR.GADGET_CASES[name][7]:
        assert events[e] >= FR.MIN_EVENTS, (e, events[e])
    src = np.zeros(W, dtype=np.int64)
    g, status = gpu_begin(tokens[None], [L], src, FR.GADGET_BOUND, FR.GADGET_BOUND)
    assert status == 0
    got = gpu_advance(g, n_steps, FR.GADGET_BOUND, FR.GADGET_BOUND, FR.GADGET_SEED)
    assert_state(got, want, name)
    assert_proven(tokens[None], [L], src, FR.GADGET_BOUND, g.st)


# ---- the sizes of the workload and the limits ------------------------------------------------------------------------
def _size_list(case):
    rng = np.random.default_rng(21)
    if case == "4x4":                                             # 4 full dwords per vector, K = 64 = L: one-word masks, full
        return (*FR.standard_matmul(4), 16, 80)
    if case == "5x5":                                             # 7 dwords, 125 terms
        return (*FR.standard_matmul(5, K=128), 25, 64)
    if case == "S32":                                             # TG_MAX_S; sparse vectors, or no flip stays inside bound 1
        return (*FR.pool_list(rng, 32, 128, 128, 12, 1, nnz=2), 32, 64)
    S = int(case[1:])                                             # S < 4: one partly filled dword
    return (*FR.pool_list(rng, S, 24, 24, 3, 1), S, 96)


@pytest.mark.parametrize("case", ["4x4", "5x5", "S32", "S1", "S2", "S3"])
def test_sizes_equal_the_restatement(case):
    tokens, L, S, n_steps = _size_list(case)
    K, W, bound, shift, split = tokens.shape[0], 4, 1, 1, 37
    src = np.zeros(W, dtype=np.int64)
    want, wstatus = FR.begin(tokens[None], [L], src, bound, shift)
    g, status = gpu_begin(tokens[None], [L], src, bound, shift)
    assert status == wstatus == 0
    assert_state(to_np(g.st), want, (case, "begin"))
    trace = []
    FR.advance(want, SEED + 5, 0, 0, split, bound, shift, trace=trace)
    FR.advance(want, SEED + 5, 0, split, n_steps - split, bound, shift, trace=trace)
    gpu_advance(g, split, bound, shift, SEED + 5)
    got = gpu_advance(g, n_steps - split, bound, shift, SEED + 5, step0=split)
    # At S = 1 and bound 1 every normalised vector is (1): a flip's n_q(a) + eps n_q(b) is 2, or it is 0 and then the
    # other term's mode r holds s_b + s_a = +-2, because the reduce left no two terms of opposite sign.  No flip is
    # ever accepted there; everywhere else both outcomes occur.
    assert {a for _, _, _, a in trace} == ({False} if S == 1 else {False, True})
    assert (want["state"] == 0).all() and len(trace) == W * n_steps
    if case in ("5x5", "S32"):
        assert want["cur_rank"].min() > 64
    assert_state(got, want, case)
    assert_proven(tokens[None], [L], src, shift, g.st)


# ---- more walks than workgroups ---------------------------------------------------------------------------------------
def test_a_workgroup_loops_over_walks_of_mixed_length_and_state(golden):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    W = 2 * 32 * cus + 77
    assert W > 32 * cus                                           # the launch starts at most 32 workgroups per CU
    S, K, bound, shift, n_steps = 4, 8, 1, 1, 2
    std, L = FR.standard_matmul(2)
    tokens = np.zeros((7, K, 3 * S), dtype=np.int8)
    tokens[0] = std                                               # the standard list
    tokens[1, :7] = golden("strassen")["tokens"]                  # stuck at once
    tokens[3] = std                                               # 2: empty; 3: K/2 terms and rows behind them
    tokens[4] = std                                               # a bad length
    tokens[5] = std
    tokens[5, 6, 7] = 2 + shift                                   # a value out of range
    tokens[6] = FR.pool_list(np.random.default_rng(5), S, K, K, 3, shift)[0]
    lengths = np.array([L, 7, 0, K // 2, K + 1, L, K], dtype=np.int64)
    src = np.arange(W, dtype=np.int64) % 7                        # 7 does not divide the grid: a workgroup meets them all
    one, wstatus = FR.begin(tokens, lengths, None, bound, shift)  # once per list
    want = {k: v[src] for k, v in one.items()}
    assert wstatus == FR.BAD_LENGTH | FR.BAD_RANGE and list(one["state"]) == [0, 0, 0, 0, -1, -1, 0]
    g, status = gpu_begin(tokens, lengths, src, bound, shift)
    assert status == wstatus
    assert_state(to_np(g.st), want, "begin")
    FR.advance(want, SEED, 0, 0, n_steps, bound, shift)
    assert {int(s) for s in want["state"]} == {-1, 0, 1} and (want["state"][src == 1] == 1).all()
    assert (want["state"][src == 2] == 1).all() and (want["flips"][src == 6] > 0).any()
    got = gpu_advance(g, n_steps, bound, shift, SEED)
    assert_state(got, want, "advance")
    assert_proven(tokens, np.clip(lengths, 0, K), src, shift, g.st)


def test_advance_does_not_depend_on_what_the_lds_held():
    """At S = 5 a vector fills a dword and a quarter: the list's padding bytes must be the kernel's own zeros, not
    what an earlier launch with the same LDS footprint (S = 8: the same two dwords per vector, all bytes used) left."""
    tokens, L, S, W, n_steps, bound, shift, want, _ = advanced_ref("pool70")
    K = tokens.shape[0]
    g, _ = gpu_begin(tokens[None], [L], np.zeros(W, dtype=np.int64), bound, shift)
    rng = np.random.default_rng(9)
    dense = (rng.integers(1, 3, size=(1, K, 24)) * rng.choice([-1, 1], size=(1, K, 24)) + shift).astype(np.int8)
    slots = 32 * torch.cuda.get_device_properties(DEV).multi_processor_count
    d = ops.flip_begin(dev(dense), dev(np.array([K])), src=torch.zeros(slots, dtype=torch.int64, device=DEV), bound=bound,
                       shift=shift)
    ops.flip_advance(d, 1, bound=bound, shift=shift)
    assert int(d["cur_rank"].min()) == K
    got = gpu_advance(g, n_steps, bound, shift, SEED)
    assert_state(got, want)


# ---- the Philox words and the step tails -----------------------------------------------------------------------------
def _philox_run(seed, walk0, step0, n_steps):
    std, L = FR.standard_matmul(2)
    src = np.zeros(8, dtype=np.int64)
    want, _ = FR.begin(std[None], [L], src, 1, 1)
    FR.advance(want, seed, walk0, step0, n_steps, 1, 1)
    g, _ = gpu_begin(std[None], [L], src, 1, 1)
    got = gpu_advance(g, n_steps, 1, 1, seed, walk0=walk0, step0=step0)
    assert_state(got, want, (seed, walk0, step0, n_steps))
    return got


@pytest.mark.parametrize("step0, n_steps", [(0, 1), (0, 63), (0, 65), (37, 100), (2 ** 32 - 70, 70)])
def test_step_tails_and_the_last_step_index(step0, n_steps):
    got = _philox_run(SEED, 0, step0, n_steps)
    assert got["flips"].sum() > 0


def test_high_words_of_seed_and_walk_id_reach_philox():
    low_seed, high_seed = _philox_run(3, 0, 0, 100), _philox_run((9 << 32) | 3, 0, 0, 100)
    low_walk, high_walk = _philox_run(SEED, 5, 0, 100), _philox_run(SEED, (1 << 40) + 5, 0, 100)
    for a, b in ((low_seed, high_seed), (low_walk, high_walk)):
        assert not np.array_equal(a["cur"], b["cur"]) and not np.array_equal(a["flips"], b["flips"])
    _philox_run(SEED, 2 ** 32 - 3, 0, 100)                        # the id's low word wraps inside the call


# ---- cur_rank outside [0, K]; capture --------------------------------------------------------------------------------
def test_a_walk_whose_cur_rank_is_outside_0_K_is_left_as_it_is():
    std, L = FR.standard_matmul(2)
    K, W = std.shape[0], 6
    src = np.zeros(W, dtype=np.int64)
    g, _ = gpu_begin(std[None], [L], src, 1, 1)
    for w, rank in ((1, K + 1), (4, -1)):
        g.st["cur_rank"][w] = rank
        g.st["cur"][w].fill_(0x55)
        g.st["best"][w].fill_(0x55)
    marked = to_np(g.st)
    assert list(marked["state"]) == [0] * W
    want = FR.copy_state(marked)
    FR.advance(want, SEED, 0, 0, 64, 1, 1)
    got = gpu_advance(g, 64, 1, 1, SEED)
    for k in FR.STATE_NAMES:
        assert np.array_equal(got[k][[1, 4]], marked[k][[1, 4]]), k
    assert_state(got, want)
    assert (got["flips"][[0, 2, 3, 5]] > 0).all()


def test_captured_graph_of_begin_and_two_advances_equals_the_eager_calls():
    tokens, L, S, W, n_steps, bound, shift, want, _ = advanced_ref("3x3")
    K = tokens.shape[0]
    _, tok = odd(dev(tokens[None]))
    lens, src = dev(np.array([L], dtype=np.int64)), torch.zeros(W, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    g = Guarded(W, K, S)

    def call():
        ops.flip_begin(tok, lens, src=src, bound=bound, shift=shift, status=status, **g.st)
        ops.flip_advance(g.st, 100, bound=bound, shift=shift, seed=SEED)
        ops.flip_advance(g.st, n_steps - 100, bound=bound, shift=shift, seed=SEED, step0=100)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    eager = to_np(g.st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for name, _ in ops._FLIP_STATE:
        g.st[name].fill_(0x33)                                    # the replay starts from rubbish, as begin may
    graph.replay()
    torch.cuda.synchronize()
    g.check()
    got = to_np(g.st)
    assert_state(got, eager, "eager")
    assert_state(got, want, "restatement")
    assert int(status.cpu().view(torch.int32).item()) == 0


@pytest.mark.parametrize("K", list(FR.ANTIPAIR_CASES))
def test_both_terms_null_removes_the_higher_slot_first(K):
    """No walk from a reduced list nulls both terms of a flip (test_flips_cpu.py), so the state is written by hand: a
    term and its negative among inert terms.  The rule is the header's all the same."""
    start, want, events = FR.antipair_ref(K)
    assert events["null_both"] >= FR.MIN_EVENTS
    W, S, bound = len(start["state"]), FR.GADGET_S, FR.GADGET_BOUND
    g = Guarded(W, K, S)
    for name in FR.STATE_NAMES:
        g.st[name].copy_(dev(start[name]))
    got = gpu_advance(g, FR.ANTIPAIR_STEPS, bound, bound, FR.GADGET_SEED)
    assert_state(got, want, K)
    assert_proven(start["cur"], start["cur_rank"], None, bound, g.st, reduced=False)
