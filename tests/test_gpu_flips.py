"""GPU checks of the flip-graph walks (include/tensor_game_flips.h): ``ops.flip_begin`` and ``ops.flip_advance`` bit for
bit against the host restatement (flips_ref.py) on unaligned, canary-guarded buffers; continuation, sharding, stuck and
bad walks; the exact proof of every walk's best list, which does not go through the restatement; ``FlipWalks`` and
``reduce_archive``."""
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


def assert_proven(tokens, lengths, src, shift, st):
    """Independent of the restatement: every walk's best list is a proven factorisation of what its start list sums to,
    of rank best_rank."""
    targets = flips.term_sum(dev(tokens), dev(np.asarray(lengths, np.int64)), shift)
    idx = torch.arange(len(lengths), device=DEV) if src is None else dev(np.asarray(src, np.int64))
    good = st["state"] >= 0
    _, rank, _, res = ops.solution_canon(targets[idx].contiguous(), st["best"].contiguous(), st["best_rank"].to(torch.int64),
                                         shift=shift)
    assert bool((res[good] == 0).all()) and torch.equal(rank[good], st["best_rank"][good])
    _, rank, _, res = ops.solution_canon(targets[idx].contiguous(), st["cur"].contiguous(), st["cur_rank"].to(torch.int64),
                                         shift=shift)
    assert bool((res[good] == 0).all()) and torch.equal(rank[good], st["cur_rank"][good])


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
