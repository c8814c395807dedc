"""GPU checks of the solution archive: ``tg_solution_canon`` bit for bit against the host restatement
(tests/solutions_ref.py) over the sizes at which the kernel takes another path, its invariance, the int8 wrap case,
addressing, bad rows, graph capture, and ``SolutionArchive`` against the restatement's ``Archive`` and end to end."""
import functools
import io

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import SolutionArchive, SyntheticDemos, TensorGameEnv, _lib, ops, rollout

import solutions_ref as SR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy()


def ukey(key):
    """The uint64 keys an int64 device tensor holds."""
    return host(key).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(S, K, shift, M=None):
    """(tokens, lengths, targets, the restatement's outputs) of one seeded batch, computed once."""
    M = M or (37 if S <= 5 else 5)
    rng = np.random.default_rng(100000 * S + 100 * K + shift)
    tokens, lengths = SR.random_lists(rng, M, K, S, shift)
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    return tokens, lengths, targets, SR.canon(targets, tokens, lengths, shift)


def run(targets, tokens, lengths, shift, **kw):
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.solution_canon(None if targets is None else dev(targets), dev(tokens), dev(lengths), shift=shift,
                             status=status, **kw)
    return out, int(status.cpu().view(torch.int32).item())


def assert_equal_to_ref(out, status, want, what=""):
    canon, rank, key, res = out
    assert np.array_equal(host(rank), want[1]), what
    assert np.array_equal(host(canon), want[0]), what
    assert np.array_equal(ukey(key), want[2]), what
    if want[3] is None:
        assert res is None
    else:
        assert np.array_equal(host(res), want[3]), what
    assert status == want[4], what


@pytest.mark.parametrize("shift", [1, 2])
@pytest.mark.parametrize("K", [1, 7, 64, 65, 256])
@pytest.mark.parametrize("S", [1, 2, 4, 5, 9, 16, 25, 32])
def test_bit_exact_against_the_restatement(S, K, shift):
    tokens, lengths, targets, want = case(S, K, shift)
    assert lengths.min() == 0 and lengths.max() == K
    out, status = run(targets, tokens, lengths, shift)
    assert_equal_to_ref(out, status, want, (S, K, shift))
    res = want[3]
    assert (res[0::3] == 0).all() and (res[1::3] == 1).all()   # the exact sums and the sums with one entry changed
    if S > 1:
        assert (res[2::3] > 0).any()


@pytest.mark.parametrize("K", [7, 64, 65, 256])
@pytest.mark.parametrize("S", [1, 4, 9, 25])
def test_invariant_under_rewriting(S, K):
    shift, M = 1, 12 if S <= 5 else 4
    rng = np.random.default_rng(977 * S + K)
    lengths = rng.integers(0, K - 2, size=M)
    lengths[0], lengths[-1] = 0, K - 3
    tokens, lengths = SR.random_lists(rng, M, K, S, shift, lengths)
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    tok2, len2 = np.zeros_like(tokens), np.zeros_like(lengths)
    for m in range(M):
        tok2[m], len2[m] = SR.variant(rng, tokens[m], int(lengths[m]), K, S, shift)
    assert (len2 == lengths + 3).all()
    (c1, r1, k1, n1), s1 = run(targets, tokens, lengths, shift)
    (c2, r2, k2, n2), s2 = run(targets, tok2, len2, shift)
    assert s1 == s2 == 0
    assert torch.equal(c1, c2) and torch.equal(r1, r2) and torch.equal(k1, k2) and torch.equal(n1, n2)
    assert int(r1.max()) > 0 and len(set(ukey(k1)[host(r1) > 0])) > 1


def test_int8_wrap_is_reported_solved_and_not_proven():
    S, K = 4, 256
    unit = np.ones(3 * S, dtype=np.int8)
    unit[[0, S, 2 * S]] = 2                                    # e0 (x) e0 (x) e0 at shift 1
    env = TensorGameEnv(1, S, device=DEV)
    env.reset(torch.zeros((S, S, S), dtype=torch.int8))
    action = dev(unit[None])
    for _ in range(K):
        env.step(action)
    assert int(env.done[0]) == 1 and int(env.overflow[0]) == 1 and not env.state.any()
    targets = torch.zeros((1, S, S, S), dtype=torch.int8, device=DEV)
    tokens, lengths = dev(np.broadcast_to(unit, (1, K, 3 * S))), dev(np.array([K], dtype=np.int64))
    canon, rank, key, res = ops.solution_canon(targets, tokens, lengths)
    assert int(res[0]) == 1 and int(rank[0]) == K and torch.equal(canon, tokens)
    arch = SolutionArchive(S=S, max_rank=K, capacity=8, device=DEV)
    rep = arch.add(targets, tokens, lengths)
    assert not bool(rep.proven[0]) and not bool(rep.fresh[0]) and int(arch.count) == 0
    assert int(arch.lowest_rank) == K + 1 and arch.entries()[0].shape[0] == 0


def odd(x):
    """A copy of int8 ``x`` one byte behind an aligned allocation (with canaries around it): (buffer, view)."""
    n = x.numel()
    buf = torch.full((GUARD + 1 + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + 1:GUARD + 1 + n].view(torch.int8).view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 1
    return buf, view


@pytest.mark.parametrize("S", [4, 9, 25])
def test_any_alignment_and_no_write_outside_the_outputs(S):
    K, shift = 7, 1
    tokens, lengths, targets, want = case(S, K, shift, 6)
    M = len(lengths)
    _, tgt = odd(dev(targets))
    _, tok = odd(dev(tokens))
    cbuf, canon = odd(torch.zeros((M, K, 3 * S), dtype=torch.int8, device=DEV))
    rbuf, rank = guarded((M,), torch.int32)
    kbuf, key = guarded((M,), torch.int64)
    nbuf, res = guarded((M,), torch.int32)
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.solution_canon(tgt, tok, dev(lengths), shift=shift, canon=canon, rank=rank, key=key, residual_nnz=res,
                             status=status)
    assert out[0] is canon and out[1] is rank and out[2] is key and out[3] is res
    assert_equal_to_ref(out, int(status.cpu().view(torch.int32).item()), want)
    n = canon.numel()
    assert bool((cbuf[:GUARD + 1] == CANARY).all()) and bool((cbuf[GUARD + 1 + n:] == CANARY).all())
    for buf, what in ((rbuf, "rank"), (kbuf, "key"), (nbuf, "residual_nnz")):
        check_flat(buf, what)
    # without targets: the same form, no verification
    c2, r2, k2, n2 = ops.solution_canon(None, tok, dev(lengths), shift=shift)
    assert n2 is None and torch.equal(c2, canon) and torch.equal(r2, rank) and torch.equal(k2, key)


def test_bad_rows_are_zeroed_and_flagged_alone():
    S, K, shift = 2, 5, 0
    rng = np.random.default_rng(7)
    tokens, lengths = SR.random_lists(rng, 6, K, S, shift, [3, 0, 4, 0, 2, 5])
    lengths[[1, 3]] = -1, K + 1
    targets = SR.targets_for(rng, tokens, np.clip(lengths, 0, K), S, shift)
    want = SR.canon(targets, tokens, lengths, shift)
    assert want[4] == SR.BAD_LENGTH
    assert_equal_to_ref(*run(targets, tokens, lengths, shift), want)
    tokens[2, 0] = [-128, 1, 1, 0, 1, 0]                        # -u holds 128
    tokens[5, 1] = [-1, 0, 1, 0, 1, -128]                       # sigma = -1 alone in its run: -w holds 128
    tokens[5, 2] = [-128, 1, 0, 0, 1, 0]                        # a null term: dropped before any negation
    want = SR.canon(targets, tokens, lengths, shift)
    assert want[4] == SR.BAD_LENGTH | SR.BAD_NEGATION and want[3][2] == -1
    (canon, rank, key, res), status = run(targets, tokens, lengths, shift)
    assert_equal_to_ref((canon, rank, key, res), status, want)
    for m in (1, 2, 3):
        assert not canon[m].any() and (int(rank[m]), int(key[m]), int(res[m])) == (0, 0, -1)
    only_null = tokens[5:6].copy()
    only_null[0, 1] = only_null[0, 2]
    assert run(None, only_null, lengths[5:6], shift)[1] == 0
    assert run(None, tokens[5:6], lengths[5:6], shift)[1] == SR.BAD_NEGATION
    with pytest.raises(_lib.TensorGameError, match="lengths"):
        ops.solution_canon(None, dev(tokens), dev(lengths[:3]))
    with pytest.raises(_lib.TensorGameError, match="targets"):
        ops.solution_canon(dev(targets[:, :1]), dev(tokens), dev(lengths))
    with pytest.raises(_lib.TensorGameError, match="K=257"):
        ops.solution_canon(None, torch.zeros((1, 257, 6), dtype=torch.int8, device=DEV), dev(lengths[:1]))


@pytest.mark.parametrize("K", [7, 65])
def test_captured_graph_equals_the_eager_call(K):
    S, shift = 4, 1
    a, b = case(S, K, shift), case(S, K, 2)                    # two batches of the same shape (tokens of shift 2 as shift 1)
    tgt, tok, lens = dev(a[2]), dev(a[0]), dev(a[1])
    M = len(a[1])
    canon = torch.zeros((M, K, 3 * S), dtype=torch.int8, device=DEV)
    rank = torch.zeros(M, dtype=torch.int32, device=DEV)
    key = torch.zeros(M, dtype=torch.int64, device=DEV)
    res = torch.zeros(M, dtype=torch.int32, device=DEV)
    call = lambda: ops.solution_canon(tgt, tok, lens, shift=shift, canon=canon, rank=rank, key=key, residual_nnz=res)  # noqa: E731
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    tgt.copy_(dev(b[2])), tok.copy_(dev(b[0])), lens.copy_(dev(b[1]))
    g.replay()
    torch.cuda.synchronize()
    eager = ops.solution_canon(tgt, tok, lens, shift=shift)
    for got, want in zip((canon, rank, key, res), eager):
        assert torch.equal(got, want)
    assert int(rank.max()) > 0


# ---- the archive -----------------------------------------------------------------------------------------------------
def pool(S=4, K=8, shift=1, M=36):
    """Lists of which a third are proven, with rewritten copies of earlier rows among them."""
    rng = np.random.default_rng(4242)
    tokens, lengths = SR.random_lists(rng, M, K, S, shift, rng.integers(0, K - 2, size=M))
    for m in range(24, M):                                     # row m := row m - 24 written differently
        tokens[m], lengths[m] = SR.variant(rng, tokens[m - 24], int(lengths[m - 24]), K, S, shift)
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    targets[24:] = targets[:M - 24]
    return targets, tokens, lengths


def assert_same_archive(arch, ref):
    tokens, rank, key, target_key = arch.entries()
    assert int(arch.count) == ref.count == tokens.shape[0] and int(arch.status) == ref.status
    assert int(arch.lowest_rank) == ref.lowest_rank
    if ref.count:
        assert np.array_equal(host(tokens), np.stack(ref.tokens))
        assert host(rank).tolist() == ref.rank and ukey(key).tolist() == ref.key
        assert ukey(target_key).tolist() == ref.target_key


def assert_same_report(rep, want):
    proven, rank, key, fresh = want
    assert np.array_equal(host(rep.proven), proven) and np.array_equal(host(rep.rank), rank)
    assert np.array_equal(ukey(rep.key), key) and np.array_equal(host(rep.fresh), fresh)


def test_archive_equals_the_restatement_over_overlapping_adds():
    S, K, shift = 4, 8, 1
    targets, tokens, lengths = pool(S, K, shift)
    arch = SolutionArchive(S=S, max_rank=6, capacity=64, device=DEV, shift=shift)
    ref = SR.Archive(S, 6, 64, shift)
    stored = 0
    for sl in (slice(0, 20), slice(10, 30), slice(5, 36)):
        rep = arch.add(dev(targets[sl]), dev(tokens[sl]), dev(lengths[sl]))
        want = ref.add(targets[sl], tokens[sl], lengths[sl])
        assert_same_report(rep, want)
        assert_same_archive(arch, ref)
        stored += int(want[3].sum())
    assert ref.count == stored >= 6 and int(arch.table_status) == 0
    assert (host(arch.table) != 0).sum() == ref.count == len(ref.offered)
    # rank above max_rank: proven, not stored
    small = SolutionArchive(S=S, max_rank=1, capacity=64, device=DEV, shift=shift)
    rep = small.add(dev(targets), dev(tokens), dev(lengths))
    assert_same_report(rep, SR.Archive(S, 1, 64, shift).add(targets, tokens, lengths))
    assert bool((rep.proven & (rep.rank > 1)).any()) and int(small.entries()[1].max()) <= 1


def test_archive_capacity_cut_and_state_dict_round_trip():
    S, K, shift = 4, 8, 1
    targets, tokens, lengths = pool(S, K, shift)
    args = (dev(targets), dev(tokens), dev(lengths))
    arch, ref = SolutionArchive(S=S, max_rank=K, capacity=3, device=DEV, shift=shift), SR.Archive(S, K, 3, shift)
    assert_same_report(arch.add(*args), ref.add(targets, tokens, lengths))
    assert_same_archive(arch, ref)
    assert int(arch.count) == 3 and int(arch.status) == 1
    blob = io.BytesIO()
    torch.save({"solutions": arch.state_dict()}, blob)
    blob.seek(0)
    sd = torch.load(blob, weights_only=True)["solutions"]
    back = SolutionArchive.from_state_dict(sd, DEV)
    for x, y in zip(arch.entries(), back.entries()):
        assert torch.equal(x, y)
    assert (int(back.count), int(back.status), int(back.lowest_rank)) == (3, 1, int(arch.lowest_rank))
    for a in (arch, back):                                      # the reloaded archive answers as the original
        rep = a.add(*args)
        assert not bool(rep.fresh.any()) and int(a.count) == 3
    # with room to spare: a reloaded archive goes on exactly where the original does
    big, ref = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV, shift=shift), SR.Archive(S, K, 64, shift)
    big.add(*(x[:18] for x in args)), ref.add(targets[:18], tokens[:18], lengths[:18])
    back = SolutionArchive.from_state_dict(big.state_dict(), DEV)
    want = ref.add(targets[9:], tokens[9:], lengths[9:])
    for a in (big, back):
        assert_same_report(a.add(*(x[9:] for x in args)), want)
        assert_same_archive(a, ref)
    assert int(want[3].sum()) > 0
    empty = SolutionArchive.from_state_dict(SolutionArchive(S=S, max_rank=K, capacity=4, device=DEV).state_dict(), DEV)
    assert int(empty.count) == 0 and int(empty.lowest_rank) == K + 1


def test_end_to_end_reversed_demonstrations_at_s4():
    S, R, G, n = 4, 5, 64, 2
    demos = SyntheticDemos(R, G, 1, S, device=DEV, seed=31)
    states = demos.target_tensor[:, None].contiguous()
    scalars = torch.zeros((G, 1), device=DEV)

    def policy(frames, scal, rows, step):                      # every sample un-does its demonstration, last action first
        return demos.action_seq[rows // n, R - 1 - step].contiguous()

    res = rollout.sample_rollouts(policy, states, scalars, n, R)
    assert int(res.num_solved) == G
    arch = SolutionArchive(S=S, max_rank=16, capacity=256, device=DEV)
    rep = arch.add_result(res, states)
    assert rep.proven.shape == (G,) and bool(rep.proven.all())
    groups, tokens, lengths = (host(x) for x in res.solutions())
    targets = host(states[:, 0])
    want = SR.canon(targets[groups], tokens, lengths, 1)
    assert (want[3] == 0).all() and np.array_equal(ukey(rep.key), want[2])
    distinct = len(set(want[2].tolist()))
    assert int(arch.count) == distinct == int(rep.fresh.sum()) and int(arch.lowest_rank) == want[1].min()
    by_key = {SR.state_key(t): t for t in targets}
    etok, erank, ekey, etarget = (host(x) for x in arch.entries())
    for tok, r, tk in zip(etok, erank, etarget.view(np.uint64)):
        assert np.array_equal(SR.term_sum(tok, int(r), S, 1), by_key[int(tk)])
    # the same search through solve_states: a SolveResult, nothing new
    sres = rollout.solve_states(policy, states, scalars, n, R, chunk_groups=24)
    rep2 = arch.add_result(sres, states)
    assert bool(rep2.proven.all()) and not bool(rep2.fresh.any()) and int(arch.count) == distinct
    with pytest.raises(mat_mul_amd.TensorGameError, match="shift"):
        SolutionArchive(S=S, max_rank=16, capacity=8, device=DEV, shift=2).add_result(res, states)
