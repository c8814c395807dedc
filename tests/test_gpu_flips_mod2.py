"""GPU checks of the flip-graph walks over Z_2 (include/tensor_game_flips_mod2.h): ``ops.flip2_begin`` and
``ops.flip2_advance`` bit for bit against the host restatement (flips_mod2_ref.py), all nine tensors, on canary-guarded
buffers at deliberately odd offsets; after every run the independent proof, ``ops.flip2_residual`` of ``best`` and of
``cur`` against the start list's own sum, which does not go through the restatement; continuation, sharding, plus
transitions, stuck, frozen and bad walks; K = 64, 65, 70 and 128; S = 1 .. 32 with bit 31 in use; more walks than
workgroups; the Philox words and step tails; ``tg_flip2_residual`` against numpy; ``Mod2Walks``, ``reduce_archive_mod2``
and graph capture."""
import io
from collections import Counter

import numpy as np
import pytest
import torch

from mat_mul_amd import Mod2Walks, SolutionArchive, TensorGameError, flips, ops, reduce_archive_mod2, reduce_mod2

import flips_mod2_ref as F2
import flips_ref as FR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0   # the seed test_flips_mod2_cpu.py chose: walks from the standard <2,2,2> list reach rank 7 with it


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def odd(x, skew=1):
    """A copy of ``x`` ``skew`` bytes behind an aligned allocation (with canaries around it): (buffer, view)."""
    n = x.numel() * x.element_size()
    buf = torch.full((GUARD + skew + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + skew:GUARD + skew + n].view(x.dtype).view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == skew
    return buf, view


class Guarded:
    """The nine state tensors in guarded buffers (the two lists 4 bytes behind a 16-byte boundary: rows of 12 bytes that
    no wider access may assume aligned), and the check that the guards survived."""

    def __init__(self, W, K):
        self.bufs, self.st = {}, {}
        for name, dtype in ops._FLIP2_STATE:
            if name in ("cur", "best"):
                self.bufs[name], self.st[name] = odd(torch.zeros((W, K, 3), dtype=torch.int32, device=DEV), 4)
            else:
                self.bufs[name], self.st[name] = guarded((W,), dtype)

    def check(self):
        for name, buf in self.bufs.items():
            if name in ("cur", "best"):
                n = self.st[name].numel() * 4
                assert bool((buf[:GUARD + 4] == CANARY).all()) and bool((buf[GUARD + 4 + n:] == CANARY).all()), name
            else:
                check_flat(buf, name)


def to_np(st):
    return {k: st[k].cpu().numpy() for k in F2.STATE_NAMES}


def assert_state(got, want, what="", names=F2.STATE_NAMES):
    for k in names:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[:8])


def gpu_begin(tokens, lengths, src, shift):
    """(Guarded, status bits) of ``ops.flip2_begin`` on unaligned inputs and guarded outputs."""
    M, K, A3 = tokens.shape
    W = M if src is None else len(src)
    g = Guarded(W, K)
    _, tok = odd(dev(tokens))
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.flip2_begin(tok, dev(np.asarray(lengths, dtype=np.int64)), src=None if src is None else dev(np.asarray(src, np.int64)),
                          shift=shift, status=status, **g.st)
    assert all(out[k] is g.st[k] for k in F2.STATE_NAMES)
    g.check()
    return g, int(status.cpu().view(torch.int32).item())


def gpu_advance(g, n_steps, S, seed, walk0=0, step0=0, plus_after=0, plus_slack=1):
    ops.flip2_advance(g.st, n_steps, S, plus_after, plus_slack, seed=seed, walk0=walk0, step0=step0)
    g.check()
    return to_np(g.st)


def assert_proven(tokens, lengths, src, shift, st):
    """Independent of the restatement: ``tg_flip2_residual`` of every good walk's best list and of its current list
    against the sum of the list it started from is 0."""
    M, K, A3 = tokens.shape
    S = A3 // 3
    targets = dev(np.stack([F2.target_of(tokens[m], int(np.clip(lengths[m], 0, K)), S, shift) for m in range(M)]))
    idx = torch.arange(M, device=DEV) if src is None else dev(np.clip(np.asarray(src, np.int64), 0, M - 1))
    good = st["state"] >= 0
    assert bool(good.any())
    for which in ("best", "cur"):
        res = ops.flip2_residual(targets[idx].contiguous(), st[which].contiguous(), st[which + "_rank"].contiguous())
        assert bool((res[good] == 0).all()), which


# ---- begin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, K, shift", [(4, 8, 0), (5, 7, 1), (9, 27, 2), (4, 64, 0), (4, 65, 1), (5, 128, 2), (32, 16, 1)])
def test_begin_on_planted_lists(S, K, shift):
    rng = np.random.default_rng(100 * S + K)
    M = 9
    tokens = np.zeros((M, K, 3 * S), dtype=np.int8)
    lengths = np.full(M, K, dtype=np.int64)
    for m in range(6):
        tokens[m] = FR.planted_list(rng, S, K, 2, shift, rot=m)[0]     # bound 2: values -2 .. 2
    tokens[6] = FR.planted_list(rng, S, K, 2, shift, rot=2)[0]
    lengths[6] = K // 2                                           # the rows behind the length are not read
    tokens[6, K // 2:] = 127
    lengths[7] = 0                                                # an empty list
    tokens[8] = rng.integers(-2, 3, size=(K, 3 * S)) + shift      # the parity of negatives, even non-zero values
    src = np.array([7, 0, 0, 3, 1, 2, 4, 5, 6, 2, 5, 8], dtype=np.int64)   # repeats, W != M
    want, wstatus = F2.begin(tokens, lengths, src, shift)
    assert wstatus == 0 and (want["cur_rank"][1:9] < lengths[src[1:9]]).all()      # every planted list lost terms
    assert want["cur_rank"][0] == 0 and want["state"][0] == 0
    if S == 32:
        assert (want["cur"] < 0).any()                            # bit 31 is in use
    g, status = gpu_begin(tokens, lengths, src, shift)
    assert status == 0
    assert_state(to_np(g.st), want, (S, K))
    assert_proven(tokens, lengths, src, shift, g.st)
    g2, status = gpu_begin(tokens, lengths, None, shift)          # src = NULL: walk w starts from list w
    assert status == 0
    assert_state(to_np(g2.st), F2.begin(tokens, lengths, None, shift)[0], (S, K, "no src"))
    assert_proven(tokens, lengths, None, shift, g2.st)


# ---- advance ---------------------------------------------------------------------------------------------------------
def _with_bit_31(tokens, L, shift):
    tokens = tokens.copy()
    tokens[:L, 31::32] = 1 + shift                                # every vector holds bit 31: the matching ones and the others
    return tokens, L


def _start_lists(case):
    """(tokens, L, S, W, n_steps, shift)"""
    rng = np.random.default_rng(7)
    if case == "2x2":
        return (*FR.standard_matmul(2), 4, 64, 512, 1)
    if case == "3x3":
        return (*FR.standard_matmul(3), 9, 16, 256, 1)
    if case == "4x4":                                             # S = 16, K = 64 = L: one-word masks, full
        return (*FR.standard_matmul(4), 16, 4, 48, 1)
    if case == "5x5":                                             # S = 25, 125 terms
        return (*FR.standard_matmul(5, K=128), 25, 4, 48, 1)
    if case == "pool70":
        return (*FR.pool_list(rng, 7, 70, 70, 60, 2), 7, 4, 64, 2)
    if case == "pool128":                                         # both of a lane's slots stay live
        return (*FR.pool_list(rng, 8, 128, 128, 40, 2), 8, 4, 64, 2)
    if case == "S32":                                             # TG_MAX_S
        return (*_with_bit_31(*FR.pool_list(rng, 32, 128, 128, 40, 1), 1), 32, 4, 48, 1)
    S = int(case[1:])                                             # S = 1, 2, 3: a few bits of one word
    return (*FR.pool_list(rng, S, 24, 24, 3, 1), S, 4, 96, 1)


_REF = {}


def advanced_ref(case):
    """(tokens, L, S, W, n_steps, shift, restatement's state after begin, after n_steps, its trace) -- computed once;
    the states are shared, so nobody changes them."""
    if case not in _REF:
        tokens, L, S, W, n_steps, shift = _start_lists(case)
        st, status = F2.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), shift)
        assert status == 0
        begun = F2.copy_state(st)
        trace = []
        F2.advance(st, SEED, 0, 0, n_steps, trace=trace)
        _REF[case] = (tokens, L, S, W, n_steps, shift, begun, st, trace)
    return _REF[case]


@pytest.mark.parametrize("case", ["2x2", "3x3", "pool70", "pool128", "4x4", "5x5", "S32", "S1", "S2", "S3"])
def test_advance_equals_the_restatement(case):
    tokens, L, S, W, n_steps, shift, begun, want, trace = advanced_ref(case)
    if S > 3:
        assert {v for _, _, _, v in trace} == set(range(4))                           # all four variants were drawn
        assert want["flips"].sum() == len(trace) > 0
    if case == "pool70":
        assert begun["cur_rank"].min() > 64
    if case in ("pool128", "5x5", "S32"):
        assert want["cur_rank"].min() > 64
    if case == "S32":                                             # bit 31 in every vector of the start, matching or not
        assert (begun["cur"][:, :64] < 0).mean() > 0.9            # (a merge or a flip XORs two of them: it goes and comes)
        assert all((want["cur"][w, :want["cur_rank"][w]] >= 0).any() for w in range(W))
    src = np.zeros(W, dtype=np.int64)
    g, status = gpu_begin(tokens[None], [L], src, shift)
    assert status == 0
    assert_state(to_np(g.st), begun, (case, "begin"))
    got = gpu_advance(g, n_steps, S, SEED)
    assert_state(got, want, case)
    assert_proven(tokens[None], [L], src, shift, g.st)


def test_continuation_100_then_156_equals_256():
    tokens, L, S, W, n_steps, shift, _, want, _ = advanced_ref("3x3")
    g, _ = gpu_begin(tokens[None], [L], np.zeros(W, dtype=np.int64), shift)
    gpu_advance(g, 100, S, SEED)
    got = gpu_advance(g, 156, S, SEED, step0=100)
    assert_state(got, want)
    assert_proven(tokens[None], [L], None, shift, {k: v[:1] for k, v in g.st.items()})


def test_sharding_two_halves_equal_the_whole():
    tokens, L, S, W, n_steps, shift, _, want, _ = advanced_ref("2x2")
    for lo in (0, 32):
        g, _ = gpu_begin(tokens[None], [L], np.zeros(32, dtype=np.int64), shift)
        got = gpu_advance(g, n_steps, S, SEED, walk0=lo)
        assert_state(got, {k: v[lo:lo + 32] for k, v in want.items()}, lo)
        assert_proven(tokens[None], [L], np.zeros(32, dtype=np.int64), shift, g.st)


# ---- the Philox words and the step tails -----------------------------------------------------------------------------
def _philox_run(seed, walk0, step0, n_steps):
    std, L = FR.standard_matmul(2)
    src = np.zeros(8, dtype=np.int64)
    want, _ = F2.begin(std[None], [L], src, 1)
    F2.advance(want, seed, walk0, step0, n_steps)
    g, _ = gpu_begin(std[None], [L], src, 1)
    got = gpu_advance(g, n_steps, 4, seed, walk0=walk0, step0=step0)
    assert_state(got, want, (seed, walk0, step0, n_steps))
    assert_proven(std[None], [L], src, 1, g.st)
    return got


@pytest.mark.parametrize("step0, n_steps", [(0, 1), (0, 63), (0, 65), (37, 100), (2 ** 32 - 70, 70)])
def test_step_tails_and_the_last_step_index(step0, n_steps):
    got = _philox_run(SEED, 0, step0, n_steps)
    assert (got["flips"] == n_steps).all() or (got["state"] == 1).any()


def test_high_words_of_seed_and_walk_id_reach_philox():
    low_seed, high_seed = _philox_run(3, 0, 0, 100), _philox_run((9 << 32) | 3, 0, 0, 100)
    low_walk, high_walk = _philox_run(SEED, 5, 0, 100), _philox_run(SEED, (1 << 40) + 5, 0, 100)
    for a, b in ((low_seed, high_seed), (low_walk, high_walk)):
        assert not np.array_equal(a["cur"], b["cur"])
    _philox_run(SEED, 2 ** 32 - 3, 0, 100)                        # the id's low word wraps inside the call


# ---- plus transitions ------------------------------------------------------------------------------------------------
def _plus_start(start, golden):
    """(tokens (K,3S), L) with K one above the start length: Strassen's list (stuck at once) or the standard one."""
    if start == "stuck":
        tokens = np.zeros((8, 12), dtype=np.int8)
        tokens[:7] = golden("strassen")["tokens"]
        return tokens, 7
    return FR.standard_matmul(2, K=9)


@pytest.mark.parametrize("start", ["stuck", "walking"])
@pytest.mark.parametrize("plus_after, plus_slack", [(1, 1), (1, 2), (50, 1), (50, 2)])
def test_plus_steps_equal_the_restatement(start, plus_after, plus_slack, golden):
    tokens, L = _plus_start(start, golden)
    W, n = 16, 150
    src = np.zeros(W, dtype=np.int64)
    want, _ = F2.begin(tokens[None], [L], src, 1)
    assert (want["cur_rank"] == L).all()
    trace = []
    F2.advance(want, SEED, 0, 0, n, plus_after, plus_slack, trace=trace)
    F2.advance(want, SEED, 0, n, n, plus_after, plus_slack, trace=trace)
    assert want["pluses"].min() > 0 and {v for _, _, kind, v in trace if kind == "plus"} == set(range(12))
    if plus_after == 50 and start == "walking":
        assert want["since"].max() > 0 and want["flips"].min() > 0
    g, status = gpu_begin(tokens[None], [L], src, 1)
    assert status == 0
    gpu_advance(g, n, 4, SEED, plus_after=plus_after, plus_slack=plus_slack)
    got = gpu_advance(g, n, 4, SEED, step0=n, plus_after=plus_after, plus_slack=plus_slack)
    assert_state(got, want, (start, plus_after, plus_slack))
    assert_proven(tokens[None], [L], src, 1, g.st)


def test_plus_slack_0_a_full_list_and_a_single_term_take_no_plus():
    tokens, L = FR.standard_matmul(2, K=9)
    src = np.zeros(16, dtype=np.int64)
    plain, _ = F2.begin(tokens[None], [L], src, 1)
    F2.advance(plain, SEED, 0, 0, 300)
    g, _ = gpu_begin(tokens[None], [L], src, 1)
    got = gpu_advance(g, 300, 4, SEED, plus_after=1, plus_slack=0)
    assert_state(got, plain, "plus_slack 0", [k for k in F2.STATE_NAMES if k != "since"])
    assert_proven(tokens[None], [L], src, 1, g.st)
    # L = K: no slot for a plus, however due it is
    full, L = FR.standard_matmul(2)
    want, _ = F2.begin(full[None], [L], src, 1)
    F2.advance(want, SEED, 0, 0, 100, plus_after=1, plus_slack=4)
    assert not want["pluses"].any() and (want["cur_rank"] == 8).all()
    g, _ = gpu_begin(full[None], [L], src, 1)
    assert_state(gpu_advance(g, 100, 4, SEED, plus_after=1, plus_slack=4), want, "L = K")
    assert_proven(full[None], [L], src, 1, g.st)
    # L < 2: one term has no pair; the walk is stuck
    one = full.copy()
    want, _ = F2.begin(one[None], [1], src, 1)
    F2.advance(want, SEED, 0, 0, 10, plus_after=1, plus_slack=4)
    assert (want["state"] == 1).all() and not want["pluses"].any() and (want["cur_rank"] == 1).all()
    g, _ = gpu_begin(one[None], [1], src, 1)
    assert_state(gpu_advance(g, 10, 4, SEED, plus_after=1, plus_slack=4), want, "L = 1")
    assert_proven(one[None], [1], src, 1, g.st)


# ---- stuck, frozen and bad walks -------------------------------------------------------------------------------------
def test_a_walk_that_gets_stuck_inside_a_launch_is_frozen_in_the_next(golden):
    std, L = FR.standard_matmul(2)
    src = np.zeros(16, dtype=np.int64)
    want, _ = F2.begin(std[None], [L], src, 1)
    F2.advance(want, SEED, 0, 0, 1500)
    frozen = want["state"] == 1
    assert frozen.sum() >= 4 and (~frozen).sum() >= 2 and (want["best_step"][frozen] > 0).all()
    g, _ = gpu_begin(std[None], [L], src, 1)
    got = gpu_advance(g, 1500, 4, SEED)
    assert_state(got, want)
    F2.advance(want, SEED, 0, 1500, 200)
    again = gpu_advance(g, 200, 4, SEED, step0=1500)
    assert_state(again, want, "next launch")
    for k in F2.STATE_NAMES:
        assert np.array_equal(again[k][frozen], got[k][frozen]), k
    assert (again["flips"][~frozen] > got["flips"][~frozen]).all()
    assert_proven(std[None], [L], src, 1, g.st)


def test_bad_rows_set_their_bit_and_touch_nothing_else():
    S, K, shift = 4, 8, 1
    std, L = FR.standard_matmul(2)
    tokens = np.repeat(std[None], 4, axis=0)
    good, _ = F2.begin(tokens, [L] * 4, None, shift)
    for lengths, src, bit, bad in (([L, K + 1, L, -1], None, F2.BAD_LENGTH, [1, 3]),
                                   ([L] * 4, [0, 4, 1, -1, 2], F2.BAD_SRC, [1, 3])):
        want, wstatus = F2.begin(tokens, lengths, src, shift)
        assert wstatus == bit and list(np.flatnonzero(want["state"] == -1)) == bad
        g, status = gpu_begin(tokens, lengths, src, shift)
        got = to_np(g.st)
        assert status == bit
        assert_state(got, want, bit)
        ok = got["state"] == 0
        assert not got["cur"][~ok].any() and not got["cur_rank"][~ok].any() and (got["cur"][ok] == good["cur"][0]).all()
        # advance leaves a -1 walk exactly as it is (whatever its tensors hold) and walks the others
        for k in ("cur", "best", "since", "pluses", "flips"):
            g.st[k][bad[0]].fill_(3)
        marked = to_np(g.st)
        want = {k: v.copy() for k, v in marked.items()}
        F2.advance(want, SEED, 0, 0, 64, plus_after=5)
        after = gpu_advance(g, 64, S, SEED, plus_after=5)
        for k in F2.STATE_NAMES:
            assert np.array_equal(after[k][~ok], marked[k][~ok]), k
        assert_state(after, want, "advance")
        assert_proven(tokens, lengths, src, shift, g.st)
    # the bits are sticky: a status that holds one keeps it
    status = torch.full((1,), 8, dtype=torch.int32, device=DEV).view(torch.uint32)
    ops.flip2_begin(dev(tokens), dev(np.array([L, K + 1, L, L])), status=status)
    assert int(status.cpu().view(torch.int32).item()) == 8 | F2.BAD_LENGTH


def test_walks_of_state_1_or_minus_1_or_a_rank_outside_0_K_are_left_as_they_are():
    std, L = FR.standard_matmul(2, K=9)
    K, W = std.shape[0], 8
    src = np.zeros(W, dtype=np.int64)
    g, _ = gpu_begin(std[None], [L], src, 1)
    for w, rank, state in ((1, K + 1, 0), (4, -1, 0), (2, L, 1), (6, L, -1)):
        g.st["cur_rank"][w] = rank
        g.st["state"][w] = state
        for k in ("cur", "best"):
            g.st[k][w].fill_(0x55555555)
        for k in ("since", "pluses", "flips", "best_step"):
            g.st[k][w] = 77
    marked = to_np(g.st)
    want = F2.copy_state(marked)
    F2.advance(want, SEED, 0, 0, 64, plus_after=3, plus_slack=1)
    got = gpu_advance(g, 64, 4, SEED, plus_after=3, plus_slack=1)
    for k in F2.STATE_NAMES:
        assert np.array_equal(got[k][[1, 2, 4, 6]], marked[k][[1, 2, 4, 6]]), k
    assert_state(got, want)
    assert (got["flips"][[0, 3, 5, 7]] > 0).all() and (got["pluses"][[0, 3, 5, 7]] > 0).all()
    walked = {k: v[[0, 3, 5, 7]] for k, v in g.st.items()}
    assert_proven(std[None], [L], np.zeros(4, dtype=np.int64), 1, walked)


@pytest.mark.parametrize("K, L, twin, near", [(8, 8, (0, 7), (2, 5)), (8, 7, (5, 6), (0, 1)), (128, 128, (63, 127), (64, 126)),
                                              (128, 100, (98, 99), (3, 64))])
def test_hand_written_unreduced_lists_reach_the_null_branches_of_a_flip(K, L, twin, near):
    """No state the entries made holds two terms that share two modes, so no flip of theirs leaves a null term.  A list
    written into ``cur`` by hand does: a term twice (a flip on the pair nulls a', b' or, after the first, is followed by
    a cancel) and two terms that differ in one mode, among terms that share nothing.  The removals' order shows in the
    rows, and the restatement decides."""
    S, W = 32, 32
    rng = np.random.default_rng(K + L)
    rows = rng.permutation(np.arange(1, 3 * K + 1, dtype=np.uint32)).reshape(K, 3) << 8      # pairwise distinct, non-zero
    rows[twin[1]] = rows[twin[0]]
    rows[near[1]] = rows[near[0]]
    rows[near[1], 2] ^= 0x80000001
    rows[L:] = 0
    st = {"cur": np.repeat(rows.view(np.int32)[None], W, 0), "cur_rank": np.full(W, L, np.int32)}
    st.update(best=st["cur"].copy(), best_rank=st["cur_rank"].copy(), best_step=np.zeros(W, np.int64),
              flips=np.zeros(W, np.int64), state=np.zeros(W, np.int32), since=np.zeros(W, np.int32), pluses=np.zeros(W, np.int64))
    g = Guarded(W, K)
    for k in F2.STATE_NAMES:
        g.st[k].copy_(dev(st[k]))
    events = Counter()
    F2.advance(st, SEED, 0, 0, 3, events=events)
    assert min(events["null1"], events["null2"], events["cancel"], events["merge"]) >= 4, events
    assert_state(gpu_advance(g, 3, S, SEED), st, (K, L))
    # the sum over Z_2 of the hand-written list: the twins cancel, the near pair leaves its two XORed bits
    target = F2.xor_sum(F2.from_rows(rows.view(np.int32), L), S).astype(np.int8)
    for which in ("best", "cur"):
        res = ops.flip2_residual(dev(np.repeat(target[None], W, 0)), g.st[which].contiguous(), g.st[which + "_rank"].contiguous())
        assert not bool(res.any()), which


# ---- more walks than workgroups; what the registers held ---------------------------------------------------------------
def test_a_workgroup_loops_over_walks_of_mixed_length_and_state(golden):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    W = 2 * 32 * cus + 77
    assert W > 32 * cus                                           # the launch starts at most 32 workgroups per CU
    S, K, shift, n_steps = 4, 8, 1, 2
    std, L = FR.standard_matmul(2)
    tokens = np.zeros((7, K, 3 * S), dtype=np.int8)
    tokens[0] = std                                               # the standard list
    tokens[1, :7] = golden("strassen")["tokens"]                  # stuck at once
    tokens[3] = std                                               # 2: empty; 3: K/2 terms and rows behind them
    tokens[4] = std                                               # a bad length
    tokens[5] = std
    tokens[5, 6, 7] = 2 + shift                                   # an even value: the factor loses a bit, no range error
    tokens[6] = FR.pool_list(np.random.default_rng(5), S, K, K, 3, shift)[0]
    lengths = np.array([L, 7, 0, K // 2, K + 1, L, K], dtype=np.int64)
    src = np.arange(W, dtype=np.int64) % 7                        # 7 does not divide the grid: a workgroup meets them all
    one, wstatus = F2.begin(tokens, lengths, None, shift)         # once per list
    want = {k: v[src] for k, v in one.items()}
    assert wstatus == F2.BAD_LENGTH and list(one["state"]) == [0, 0, 0, 0, -1, 0, 0]
    g, status = gpu_begin(tokens, lengths, src, shift)
    assert status == wstatus
    assert_state(to_np(g.st), want, "begin")
    F2.advance(want, SEED, 0, 0, n_steps, plus_after=1, plus_slack=1)
    assert {int(s) for s in want["state"]} == {-1, 0, 1} and (want["state"][src == 2] == 1).all()
    assert (want["pluses"][src == 3] > 0).any() and (want["flips"][src == 0] > 0).all()
    got = gpu_advance(g, n_steps, S, SEED, plus_after=1, plus_slack=1)
    assert_state(got, want, "advance")
    assert_proven(tokens, lengths, src, shift, g.st)


def test_advance_does_not_depend_on_what_the_registers_held():
    """A wavefront's registers are not cleared between launches: a second, different walk set (shorter lists, K = 70
    after K = 128 with every slot live) must come out as the restatement gives it, whatever the first left behind."""
    tokens, L, S, W, n_steps, shift, _, want, _ = advanced_ref("pool70")
    g, _ = gpu_begin(tokens[None], [L], np.zeros(W, dtype=np.int64), shift)
    rng = np.random.default_rng(9)
    dense = FR.pool_list(rng, 32, 128, 128, 60, 1)[0]
    slots = 32 * torch.cuda.get_device_properties(DEV).multi_processor_count
    d = ops.flip2_begin(dev(dense[None]), dev(np.array([128])), src=torch.zeros(slots, dtype=torch.int64, device=DEV), shift=1)
    ops.flip2_advance(d, 3, 32, seed=5)
    assert int(d["cur_rank"].min()) > 64
    got = gpu_advance(g, n_steps, S, SEED)
    assert_state(got, want)
    assert_proven(tokens[None], [L], np.zeros(W, dtype=np.int64), shift, g.st)


# ---- the proof -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, K", [(4, 8), (1, 3), (9, 27), (32, 128), (25, 70)])
def test_residual_equals_numpy(S, K):
    rng = np.random.default_rng(S * K)
    M = 7
    lists = rng.integers(0, 2 ** S, size=(M, K, 3), dtype=np.uint64).astype(np.uint32).view(np.int32)
    ranks = np.array([K, K, K // 2, 0, -1, K + 1, 1], dtype=np.int32)
    if S == 32:
        assert (lists < 0).any()
    targets = np.stack([F2.xor_sum(F2.from_rows(lists[m], int(np.clip(ranks[m], 0, K))), S) for m in range(M)]).astype(np.int8)
    targets = targets + 2 * rng.integers(-60, 60, size=targets.shape).astype(np.int8)      # only the parity counts
    cells = [(0, 0, 0), (S - 1, S - 1, S - 1), (S // 2, S - 1, 0)]
    for i, j, k in cells[:1 if S == 1 else 3]:
        targets[1, i, j, k] ^= 1                                   # list 1: exactly these cells differ
    lists[2, K // 2:] = -1                                         # rows beyond the rank are poison, and ignored
    lists[3] = 0x5A5A5A5A
    want = F2.residual(targets, lists, ranks)
    assert list(want) == [0, 1 if S == 1 else 3, 0, 0, -1, -1, 0]
    _, tg = odd(dev(targets))
    _, ls = odd(dev(lists), 4)
    buf, res = guarded((M,), torch.int32)
    out = ops.flip2_residual(tg, ls, dev(ranks), residual=res)
    assert out is res
    check_flat(buf, "residual")
    assert np.array_equal(res.cpu().numpy(), want)
    # a single flipped bit of one m_2: the exact count is the number of (i, j) cells the term covers
    flipped = lists.copy()
    flipped.view(np.uint32)[0, 0, 2] ^= np.uint32(1 << (S - 1))
    count = bin(int(flipped.view(np.uint32)[0, 0, 0])).count("1") * bin(int(flipped.view(np.uint32)[0, 0, 1])).count("1")
    got = ops.flip2_residual(tg, dev(flipped), dev(ranks)).cpu().numpy()
    assert got[0] == count == F2.residual(targets, flipped, ranks)[0] and np.array_equal(got[1:], want[1:])


# ---- Mod2Walks, reduce_mod2, reduce_archive_mod2 ---------------------------------------------------------------------
def test_mod2walks_reach_rank_7_from_the_standard_2x2_algorithm():
    std, L = FR.standard_matmul(2)
    lists, lengths = dev(std[None]), dev(np.array([L]))
    walks = Mod2Walks.start(lists, lengths, walks_per_list=16, seed=SEED).advance(2000)
    want, _ = F2.begin(std[None], [L], np.zeros(16, dtype=np.int64), 1)
    F2.advance(want, SEED, 0, 0, 2000)
    assert_state(to_np(walks._st), want)
    assert int(walks.best_rank.min()) == 7 and walks.steps_done == 2000 and walks.W == 16 and walks.K == 8
    target = flips.term_sum(lists, lengths, 1)
    for which in ("best", "cur"):
        assert not bool(walks.residual(target.expand(16, 4, 4, 4).contiguous(), which).any())
    # the token form: {0,1} + shift, zero bytes beyond the rank, and the same sum mod 2
    tok = walks.tokens("best", shift=2)
    assert tok.dtype == torch.int8 and tuple(tok.shape) == (16, 8, 12)
    live = torch.arange(8, device=DEV)[None, :] < walks.best_rank[:, None]
    assert bool((tok[~live] == 0).all()) and bool(((tok[live] == 2) | (tok[live] == 3)).all())
    back = flips.term_sum(tok, walks.best_rank.to(torch.int64), 2)
    assert torch.equal(back & 1, (target & 1).expand(16, 4, 4, 4))
    with pytest.raises(TensorGameError, match="which"):
        walks.tokens("first")


@pytest.mark.parametrize("entry", ["archive", "lists"])
def test_reduce_archive_mod2_reports_rank_7_proven(entry):
    std, L = FR.standard_matmul(2, K=8)
    lists, lengths = dev(std[None]), dev(np.array([L]))
    if entry == "archive":
        arch = SolutionArchive(S=4, max_rank=8, capacity=64, device=DEV, shift=1)
        rep = arch.add(flips.term_sum(lists, lengths, 1), lists, lengths)
        assert bool(rep.proven[0]) and int(arch.count) == 1
        start = arch.entries()[0].cpu().numpy()
        res = reduce_archive_mod2(arch, 2000, walks_per_entry=8, seed=SEED)
        assert int(arch.count) == 1 and int(arch.lowest_rank) == 8          # Z_2 lists do not enter the archive
    else:
        start = std[None]
        res = reduce_mod2(lists, lengths, 2000, walks_per_list=8, seed=SEED)
    want, _ = F2.begin(start, [8], np.zeros(8, dtype=np.int64), 1)
    F2.advance(want, SEED, 0, 0, 2000)
    assert want["best_rank"].min() == 7
    assert_state(to_np(res.walks._st), want)
    assert bool(res.proven.all()) and not bool(res.residual.any()) and res.best_rank.tolist() == [7]
    # proven only through the residual: a walk whose best list is spoilt is not
    res.walks.best[3, 0, 0] ^= 1
    target = flips.term_sum(lists, lengths, 1).expand(8, 4, 4, 4).contiguous()
    assert (res.walks.residual(target) != 0).nonzero().flatten().tolist() == [3]
    if entry == "archive":
        empty = SolutionArchive(S=4, max_rank=8, capacity=4, device=DEV, shift=1)
        assert reduce_archive_mod2(empty, 10) is None


def test_mod2walks_state_dict_round_trip_continues_bit_for_bit():
    tokens, L = FR.standard_matmul(3, K=28)
    W, n, plus = 8, 200, dict(plus_after=20, plus_slack=1)
    lists, lengths = dev(tokens[None]), dev(np.array([L]))
    want, _ = F2.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), 1)
    F2.advance(want, SEED, 3, 0, n, **plus)
    assert want["pluses"].sum() > 0
    whole = Mod2Walks.start(lists, lengths, walks_per_list=W, seed=SEED, walk0=3, **plus).advance(n)
    assert_state(to_np(whole._st), want)
    part = Mod2Walks.start(lists, lengths, walks_per_list=W, seed=SEED, walk0=3, **plus).advance(77)
    f = io.BytesIO()
    torch.save({"mod2": part.state_dict()}, f)
    f.seek(0)
    back = Mod2Walks.from_state_dict(torch.load(f, weights_only=True)["mod2"], DEV)
    assert back.steps_done == 77 and (back.S, back.seed, back.walk0, back.plus_after, back.plus_slack) == (9, SEED, 3, 20, 1)
    back.advance(n - 77)
    assert_state(to_np(back._st), want)
    assert torch.equal(back.src, whole.src) and back.steps_done == n
    assert not bool(back.residual(flips.term_sum(lists, lengths, 1).expand(W, 9, 9, 9).contiguous()).any())


def test_mod2walks_advance_70000_takes_two_launches():
    std, L = FR.standard_matmul(2, K=9)                           # with plus transitions no walk is ever stuck
    lists, lengths = dev(std[None]), dev(np.array([L]))
    walks = Mod2Walks.start(lists, lengths, walks_per_list=1, seed=SEED, plus_after=40, plus_slack=2)
    with pytest.raises(TensorGameError, match="n_steps=70000"):
        ops.flip2_advance(walks._st, 70000, 4)
    walks.advance(70000)
    assert walks.steps_done == 70000
    want, _ = F2.begin(std[None], [L], np.zeros(1, dtype=np.int64), 1)
    F2.advance(want, SEED, 0, 0, 65536, 40, 2)
    F2.advance(want, SEED, 0, 65536, 70000 - 65536, 40, 2)
    assert want["flips"][0] + want["pluses"][0] == 70000 and want["state"][0] == 0     # every step of both launches acted
    assert_state(to_np(walks._st), want)
    assert not bool(walks.residual(flips.term_sum(lists, lengths, 1), "cur").any())


def test_captured_graph_of_begin_and_two_advances_equals_the_eager_calls():
    tokens, L, S, W, n_steps, shift, _, want, _ = advanced_ref("3x3")
    K = tokens.shape[0]
    _, tok = odd(dev(tokens[None]))
    lens, src = dev(np.array([L], dtype=np.int64)), torch.zeros(W, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    g = Guarded(W, K)

    def call():
        ops.flip2_begin(tok, lens, src=src, shift=shift, status=status, **g.st)
        ops.flip2_advance(g.st, 100, S, seed=SEED)
        ops.flip2_advance(g.st, n_steps - 100, S, seed=SEED, step0=100)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    eager = to_np(g.st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for name, _ in ops._FLIP2_STATE:
        g.st[name].fill_(0x33)                                    # the replay starts from rubbish, as begin may
    graph.replay()
    torch.cuda.synchronize()
    g.check()
    got = to_np(g.st)
    assert_state(got, eager, "eager")
    assert_state(got, want, "restatement")
    assert int(status.cpu().view(torch.int32).item()) == 0
    assert_proven(tokens[None], [L], np.zeros(W, dtype=np.int64), shift, g.st)
