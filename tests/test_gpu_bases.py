"""GPU checks of the way back from a changed basis: ``tg_basis_inverse_i32`` and ``tg_solution_rebase`` equal to the host
restatement (tests/bases_ref.py) over the sizes and edges of include/tensor_game_bases.h, the round trip with exact
verification, ``BasisSet.expand`` and its fallback, graph capture, and ``solve_in_bases`` into a ``SolutionArchive`` end
to end."""
import functools
import io

import numpy as np
import pytest
import torch

from mat_mul_amd import BasisSet, SolutionArchive, SyntheticDemos, _lib, ops, solve_in_bases
from oracle import tensor_game as O

import bases_ref as BR
import solutions_ref as SR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy()


def new_status():
    return torch.zeros(1, dtype=torch.uint32, device=DEV)


def word(status):
    return int(status.cpu().view(torch.int32).item())


def odd(x):
    """A copy of int8 ``x`` one byte behind an aligned allocation (with canaries around it): (buffer, view)."""
    n = x.numel()
    buf = torch.full((GUARD + 1 + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + 1:GUARD + 1 + n].view(torch.int8).view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 1
    return buf, view


def check_odd(buf, n, what):
    assert bool((buf[:GUARD + 1] == CANARY).all()) and bool((buf[GUARD + 1 + n:] == CANARY).all()), what


# ---- the inverse -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 4, 9, 16, 25, 32])
def test_inverse_equals_the_restatement(S):
    N = 5
    rng = np.random.default_rng(700 + S)
    lower, upper = BR.random_factors(rng, N, S, (0.2, 0.6, 0.2) if S <= 9 else None)
    clean = BR.basis_inverse(lower, upper)
    assert clean[2] == 0
    lower[0, 1][np.triu_indices(S, 1)] = 99                     # junk in the triangles that must not be read
    upper[0, 2][np.tril_indices(S, -1)] = -77
    lower[1, 2, S - 1, S - 1] = 0                                # a diagonal entry 0
    upper[3, 0, 0, 0] = 2                                        # and one 2
    if S == 32:
        lower[2, 0][np.tril_indices(S, -1)] = 127               # the entries of L^-1 pass 2^28
    if S == 9:                                                   # the bound itself: L^-1 holds 128^3 (triple 2) / 128^4 (triple 4)
        for n, rows in ((2, 3), (4, 4)):
            lower[n, 1] = np.eye(S)
            lower[n, 1][np.arange(1, rows + 1), np.arange(rows)] = -128
    want_inv, want_bad, want_status = BR.basis_inverse(lower, upper)
    assert want_bad.tolist() == [0, 1, int(S == 32), 1, int(S == 9)]
    assert want_status == BR.BASIS_BAD_DIAGONAL | (BR.BASIS_BAD_RANGE if S in (9, 32) else 0)
    assert np.array_equal(want_inv[0], clean[0][0])             # the junk changed nothing
    if S == 9:
        assert np.abs(want_inv[2, 1].astype(np.int64)).max() >= 128 ** 3
    ibuf, inv = guarded((N, 3, S, S), torch.int32)
    bbuf, bad = guarded((N,), torch.uint8)
    status = new_status()
    out = ops.basis_inverse(dev(lower), dev(upper), inv=inv, bad=bad, status=status)
    assert out[0] is inv and out[1] is bad
    assert np.array_equal(host(bad), want_bad) and word(status) == want_status
    assert np.array_equal(host(inv), want_inv)
    check_flat(ibuf, "inv"), check_flat(bbuf, "bad")
    for n in np.flatnonzero(want_bad):
        assert not inv[n].any()
    inv2, none = ops.basis_inverse(dev(lower), dev(upper), bad=False)       # bad and status as NULL
    assert none is None and torch.equal(inv2, inv)
    status.fill_(8)                                                         # sticky: the call only ORs
    ops.basis_inverse(dev(lower), dev(upper), status=status)
    assert word(status) == 8 | want_status


def test_sampled_bases_are_inverted_exactly():
    for S in (4, 25):
        P, L, U = ops.sample_basis(64, S, DEV, seed=3, want_factors=True)
        inv, bad = ops.basis_inverse(L, U)
        assert not bool(bad.any())
        assert np.array_equal(host(inv), O.unimodular_inverse(host(L), host(U)))
        prod = host(P).astype(np.int64) @ host(inv).astype(np.int64)
        assert np.array_equal(prod, np.broadcast_to(np.eye(S, dtype=np.int64), prod.shape))
    assert ops.basis_inverse(L[:0], U[:0])[0].shape == (0, 3, S, S)


# ---- the rebase --------------------------------------------------------------------------------------------------------
SPECIAL = ("neg_len", "long_len", "range", "beyond", "wide", "neg_idx", "big_idx")


@functools.lru_cache(maxsize=None)
def rebase_case(S, K, M, shift, indexed):
    """(tokens, lengths, mats, index or None, {kind: row} of the constructed rows, the restatement's outputs) of one
    seeded batch, computed once.  Constructed rows exist where M >= 9 or so allows them (rows 1..7)."""
    rng = np.random.default_rng(1000 * S + 10 * K + shift + 5 * indexed)
    G = max(1, M // 2) if indexed else M
    special = dict(zip(SPECIAL, range(1, 8))) if M >= 7 + 2 * indexed else {}
    if special and not indexed:
        del special["neg_idx"], special["big_idx"]
    lengths = rng.integers(0, K + 1, size=M)
    lengths[0], lengths[-1] = 0, K
    for kind, L in (("neg_len", -1), ("long_len", K + 1), ("range", 2), ("beyond", 1), ("wide", 2), ("neg_idx", 1),
                    ("big_idx", 1)):
        if kind in special:
            lengths[special[kind]] = L
    tokens, lengths = BR.random_lists(rng, M, K, S, shift, lengths)
    lower, upper = BR.random_factors(rng, G, S)
    mats = (lower.astype(np.int64) @ upper.astype(np.int64)).astype(np.int32)
    index = rng.integers(0, max(1, G - 1), size=M) if indexed else None      # repeats; triple G-1 is for the constructed rows
    for kind in ("range", "beyond", "wide"):
        if kind not in special:
            continue
        m = special[kind]
        g = G - 1 if indexed else m
        if indexed:
            index[m] = g
        mats[g, 0, 0, 1], mats[g, 1, 0, 1] = 100, -2 ** 31      # u'[0] += 100 u[1], v'[0] -= 2^31 v[1]
        tokens[m, :K, 1] = tokens[m, :K, S + 1] = shift          # u[1] = v[1] = 0 ...
        if kind == "range":
            tokens[m, 0, 1] = 2 + shift                          # ... but for a factor 2 that meets the 100
        elif kind == "beyond":
            tokens[m, 1, 1] = tokens[m, 1, S + 1] = 2 + shift    # ... or only behind the list's end: not read, not bad
        else:
            tokens[m, 1, S + 1] = 2 + shift                      # ... or -2^32, which is 0 in 32 bits
    if "neg_idx" in special:
        index[special["neg_idx"]], index[special["big_idx"]] = -1, G
    want = BR.solution_rebase(tokens, lengths, mats, index, shift)
    return tokens, lengths, mats, index, special, want


# (S, K, M) and the shifts of the two calls (index NULL, index given)
REBASE_CASES = [(2, 1, 3, 0, 1), (4, 7, 130, 2, 64), (9, 64, 9, 1, 0), (9, 65, 5, 64, 2), (16, 20, 7, 1, 2),
                (25, 75, 4, 0, 64), (32, 256, 2, 1, 1)]


@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("S, K, M, shift_null, shift_indexed", REBASE_CASES)
def test_rebase_equals_the_restatement(S, K, M, shift_null, shift_indexed, indexed):
    shift = shift_indexed if indexed else shift_null
    tokens, lengths, mats, index, special, want = rebase_case(S, K, M, shift, indexed)
    want_tok, want_len, want_bad, want_status = want
    assert lengths[0] == 0 and lengths[-1] == K
    if indexed:
        assert mats.shape[0] < M or M == 1
    # what the constructed rows are there for
    bits = 0
    for kind, bit in (("neg_len", 1), ("long_len", 1), ("neg_idx", 2), ("big_idx", 2), ("range", 4), ("wide", 4)):
        if kind in special:
            assert want_bad[special[kind]] == 1 and want_len[special[kind]] == 0, kind
            bits |= bit
    if "beyond" in special:
        assert want_bad[special["beyond"]] == 0 and want_len[special["beyond"]] == 1
    assert want_status == bits and int(want_bad.sum()) == len(special) - ("beyond" in special)
    assert bool(special) == (M >= (9 if indexed else 7)) and bits == ((7 if indexed else 5) if special else 0)
    _, tok = odd(dev(tokens))
    obuf, out = odd(torch.full((M, K, 3 * S), 33, dtype=torch.int8, device=DEV))
    lbuf, lens_out = guarded((M,), torch.int64)
    bbuf, bad = guarded((M,), torch.uint8)
    status = new_status()
    d_len, d_mats, d_index = dev(lengths), dev(mats), None if index is None else dev(index)
    res = ops.solution_rebase(tok, d_len, d_mats, index=d_index, shift=shift, tokens_out=out, lengths_out=lens_out,
                              bad=bad, status=status)
    assert res[0] is out and res[1] is lens_out and res[2] is bad
    assert np.array_equal(host(bad), want_bad) and word(status) == want_status
    assert np.array_equal(host(lens_out), want_len)
    assert np.array_equal(host(out), want_tok)
    check_odd(obuf, out.numel(), "tokens_out"), check_flat(lbuf, "lengths_out"), check_flat(bbuf, "bad")
    for m in range(M):                                          # zero padding; bad rows all zero
        assert not out[m, want_len[m]:].any()
    # the rows behind a list's end are not read: other junk there, the same answer (aligned buffers, no flags)
    keep = np.arange(K)[None, :, None] < np.clip(lengths, 0, K)[:, None, None]
    out2, len2, none = ops.solution_rebase(dev(np.where(keep, tokens, np.int8(-128))), d_len, d_mats, index=d_index,
                                           shift=shift, bad=False)
    assert none is None and torch.equal(out2, out) and torch.equal(len2, lens_out)
    with pytest.raises(_lib.TensorGameError, match="in-place"):
        ops.solution_rebase(tok, d_len, d_mats, index=d_index, shift=shift, tokens_out=tok)


def test_rebase_refusals_and_empty_batch():
    tok = torch.zeros((3, 4, 12), dtype=torch.int8, device=DEV)
    lens = torch.zeros(3, dtype=torch.int64, device=DEV)
    mats = torch.zeros((2, 3, 4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.TensorGameError, match="index must be given"):
        ops.solution_rebase(tok, lens, mats)
    with pytest.raises(_lib.TensorGameError, match="K=257"):
        ops.solution_rebase(torch.zeros((1, 257, 12), dtype=torch.int8, device=DEV), lens[:1], mats[:1])
    with pytest.raises(_lib.TensorGameError, match="shift=65"):
        ops.solution_rebase(tok, lens, mats, index=lens, shift=65)
    with pytest.raises(_lib.TensorGameError, match="lengths is on cpu"):
        ops.solution_rebase(tok, lens.cpu(), mats, index=lens)
    out, lens_out, bad = ops.solution_rebase(tok[:0], lens[:0], mats[:0])
    assert out.shape == (0, 4, 12) and lens_out.shape == (0,) and bad.shape == (0,)


def test_identity_gives_the_input_with_zeroed_padding():
    S, K, M, shift = 9, 65, 5, 2
    rng = np.random.default_rng(99)
    tokens, lengths = BR.random_lists(rng, M, K, S, shift)
    eye = torch.eye(S, dtype=torch.int32, device=DEV).expand(1, 3, S, S).contiguous()
    out, lens, bad = ops.solution_rebase(dev(tokens), dev(lengths), eye, index=torch.zeros(M, dtype=torch.int64, device=DEV),
                                         shift=shift)
    keep = np.arange(K)[None, :, None] < lengths[:, None, None]
    assert np.array_equal(host(out), np.where(keep, tokens, np.int8(0)))
    assert np.array_equal(host(lens), lengths) and not bool(bad.any())


@pytest.mark.parametrize("S", [4, 9])
def test_round_trip_commutes_with_verification(S):
    R, G, n = 5, 32, 4
    demos = SyntheticDemos(R, G, 1, S, device=DEV, seed=17)
    F, T = demos.action_seq.contiguous(), demos.target_tensor
    lengths = torch.full((G,), R, dtype=torch.int64, device=DEV)
    bases = BasisSet.sample(n, S, DEV, seed=3)
    assert not bool(bases.bad.any())
    fwd, inv = host(bases.forward).astype(np.int64), host(bases.inverse).astype(np.int64)
    assert np.array_equal(fwd @ inv, np.broadcast_to(np.eye(S, dtype=np.int64), fwd.shape))
    assert np.array_equal(fwd[0], np.broadcast_to(np.eye(S), (3, S, S))) and (fwd[1:] != fwd[0]).any()
    index = torch.arange(G, device=DEV) % n
    overflow = torch.zeros(G, dtype=torch.uint8, device=DEV)
    T2 = ops.change_basis(T, bases.forward[index], overflow=overflow)
    assert not bool(overflow.any())
    status = new_status()
    F2, len2, bad = ops.solution_rebase(F, lengths, bases.forward, index=index, status=status)
    assert not bool(bad.any()) and torch.equal(len2, lengths)
    assert np.array_equal(host(F2), BR.solution_rebase(host(F), host(lengths), host(bases.forward), host(index), 1)[0])
    res = ops.solution_canon(T2.contiguous(), F2, len2)[3]      # the moved list is a factorisation of the moved target
    assert not bool(res.any())
    moved = (T2 != T).flatten(1).any(dim=1)
    assert int(moved.sum()) >= G // 4 and not bool(moved[index == 0].any())
    res0 = ops.solution_canon(T.contiguous(), F2, len2)[3]      # ... and of the original target only where nothing moved
    assert bool((res0[moved] > 0).all())
    back, len3, bad = ops.solution_rebase(F2, len2, bases.inverse, index=index, status=status)
    assert torch.equal(back, F) and torch.equal(len3, lengths) and not bool(bad.any()) and word(status) == 0


# ---- BasisSet ----------------------------------------------------------------------------------------------------------
def test_expand_layout_frames_and_fallback():
    S, T, G, n = 4, 2, 3, 3
    rng = np.random.default_rng(8)
    states = rng.integers(-2, 3, size=(G, T, S, S, S)).astype(np.int8)
    states[1, 1, 0, 0, 0] = states[1, 1, 1, 0, 0] = 127         # frame 1 of state 1 overflows under a row (1, 1, 0, 0)
    eye = np.broadcast_to(np.eye(S, dtype=np.int32), (3, S, S))
    forward = np.stack([eye, eye, eye]).copy()
    forward[1, 0, 0, 1] = 1                                      # basis 1: A = I + E01, B = C = I
    forward[2, 2] = np.eye(S, dtype=np.int32)[::-1] * -1         # basis 2: C reverses and negates
    inverse = forward.copy()
    inverse[1, 0, 0, 1] = -1
    assert np.array_equal(forward.astype(np.int64) @ inverse, np.stack([eye] * 3))
    want = np.zeros((G * n, T, S, S, S), dtype=np.int8)
    for g in range(G):
        for j in range(n):
            want[g * n + j], ovf = O.change_basis_i8(states[g], np.broadcast_to(forward[j], (T, 3, S, S)))
            assert ovf.any() == ((g, j) == (1, 1))
    want[1 * n + 1] = states[1]                                  # that row stays untransformed, under basis 0
    want_basis = np.tile(np.arange(n), G)
    want_basis[1 * n + 1] = 0
    zero_bad = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bases = BasisSet(dev(forward), dev(inverse), zero_bad, identity_first=True)
    moved, basis_of_row = bases.expand(dev(states))
    assert moved.shape == (G * n, T, S, S, S) and basis_of_row.dtype == torch.int64
    assert np.array_equal(host(moved), want) and np.array_equal(host(basis_of_row), want_basis)
    assert (want[2] != states[0]).any() and (want[2, 1] != states[0, 1]).any()   # both frames are moved
    # a bad basis in the set falls back the same way
    bad = zero_bad.clone()
    bad[2] = 1
    moved, basis_of_row = BasisSet(dev(forward), dev(inverse), bad, identity_first=True).expand(dev(states))
    for g in range(G):
        want[g * n + 2], want_basis[g * n + 2] = states[g], 0
    assert np.array_equal(host(moved), want) and np.array_equal(host(basis_of_row), want_basis)
    with pytest.raises(_lib.TensorGameError, match="identity_first"):
        BasisSet(dev(forward), dev(inverse), zero_bad, identity_first=False).expand(dev(states))
    with pytest.raises(_lib.TensorGameError, match="states must be int8"):
        bases.expand(dev(states[:, :, :3]))


def test_basis_set_state_dict_round_trip():
    bases = BasisSet.sample(5, 9, DEV, seed=3)
    blob = io.BytesIO()
    torch.save({"bases": bases.state_dict()}, blob)
    blob.seek(0)
    back = BasisSet.from_state_dict(torch.load(blob, weights_only=True)["bases"], DEV)
    assert torch.equal(back.forward, bases.forward) and torch.equal(back.inverse, bases.inverse)
    assert torch.equal(back.bad, bases.bad) and (back.n, back.S, back.identity_first) == (5, 9, True)
    assert back.forward.is_cuda and bool((bases.forward[0] == torch.eye(9, dtype=torch.int32, device=DEV)).all())
    free = BasisSet.sample(5, 9, DEV, seed=3, identity_first=False)           # the same draws, basis 0 as drawn
    assert torch.equal(free.forward[1:], bases.forward[1:]) and not torch.equal(free.forward[0], bases.forward[0])
    again = BasisSet.sample(5, 9, DEV, seed=4)
    assert not torch.equal(again.forward, bases.forward)


def test_captured_graph_equals_the_eager_calls():
    S, K, M, N, shift = 9, 12, 21, 6, 1
    rng = np.random.default_rng(31)
    fa, fb = BR.random_factors(rng, N, S), BR.random_factors(rng, N, S)
    (ta, la), (tb, lb) = BR.random_lists(rng, M, K, S, shift), BR.random_lists(rng, M, K, S, shift)
    ia, ib = rng.integers(0, N, size=M), rng.integers(0, N, size=M)
    lower, upper, tok, lens, index = dev(fa[0]), dev(fa[1]), dev(ta), dev(la), dev(ia)
    inv = torch.zeros((N, 3, S, S), dtype=torch.int32, device=DEV)
    ibad = torch.zeros(N, dtype=torch.uint8, device=DEV)
    out = torch.zeros((M, K, 3 * S), dtype=torch.int8, device=DEV)
    lens_out = torch.zeros(M, dtype=torch.int64, device=DEV)
    bad = torch.zeros(M, dtype=torch.uint8, device=DEV)

    def call():                                                  # a linear chain: the rebase reads the inverse
        ops.basis_inverse(lower, upper, inv=inv, bad=ibad)
        ops.solution_rebase(tok, lens, inv, index=index, shift=shift, tokens_out=out, lengths_out=lens_out, bad=bad)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    lower.copy_(dev(fb[0])), upper.copy_(dev(fb[1])), tok.copy_(dev(tb)), lens.copy_(dev(lb)), index.copy_(dev(ib))
    g.replay()
    torch.cuda.synchronize()
    e_inv, e_ibad = ops.basis_inverse(lower, upper)
    e_out, e_len, e_bad = ops.solution_rebase(tok, lens, e_inv, index=index, shift=shift)
    for got, want in ((inv, e_inv), (ibad, e_ibad), (out, e_out), (lens_out, e_len), (bad, e_bad)):
        assert torch.equal(got, want)
    assert np.array_equal(host(inv), BR.basis_inverse(*fb)[0]) and bool(out.any())


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_end_to_end_solve_in_bases_at_s4():
    S, R, G, n, n_samples = 4, 5, 16, 4, 2
    demos = SyntheticDemos(R, G, 1, S, device=DEV, seed=31)
    states = demos.target_tensor[:, None].contiguous()
    scalars = torch.zeros((G, 1), device=DEV)
    bases = BasisSet.sample(n, S, DEV, seed=3)
    assert not bool(bases.bad.any())
    moved, basis_of_row = bases.expand(states)
    rows_basis = np.tile(np.arange(n), G)
    assert np.array_equal(host(basis_of_row), rows_basis)       # no fallback
    # expanded row e plays the demonstration of g = e // n moved into its basis: the restatement's tokens
    F = host(demos.action_seq)
    table, _, tbad, _ = BR.solution_rebase(np.repeat(F, n, axis=0), np.full(G * n, R), host(bases.forward), rows_basis, 1)
    assert not tbad.any()
    d_table = dev(table)

    def policy(frames, scal, rows, step):                        # last action first; `step` is a number or the rows' own steps
        e = torch.div(rows.clamp(min=0), n_samples, rounding_mode="floor")
        if torch.is_tensor(step):
            return d_table[e, R - 1 - step.to(torch.int64).clamp(max=R - 1)].contiguous()
        return d_table[e, R - 1 - step].contiguous()

    targets = host(states[:, 0])
    want = SR.canon(targets, F, np.full(G, R), 1)
    assert (want[3] == 0).all()
    distinct = len(set(want[2].tolist()))
    for kw in (dict(chunk_groups=24), dict(slots=24)):
        reb = solve_in_bases(policy, states, scalars, bases, n_samples, R, **kw)
        assert reb.groups.shape == (G * n,) and int(reb.bad.sum()) == 0 and reb.shift == 1   # every expanded group solved
        assert np.array_equal(host(reb.groups), np.arange(G * n) // n) and np.array_equal(host(reb.basis), rows_basis)
        assert np.array_equal(host(reb.found.groups), np.arange(G * n))
        arch = SolutionArchive(S=S, max_rank=16, capacity=256, device=DEV)
        rep = arch.add_result(reb, states)                       # proven against the ORIGINAL targets
        assert rep.proven.shape == (G * n,) and bool(rep.proven.all())
        keys = host(rep.key).view(np.uint64).reshape(G, n)
        assert (keys == keys[:, :1]).all() and np.array_equal(keys[:, 0], want[2])   # one key for the n copies of a group
        assert int(arch.count) == distinct == int(rep.fresh.sum()) and distinct <= G < G * n
        # the contrast: the lists as they were found, against the original targets
        plain = SolutionArchive(S=S, max_rank=16, capacity=256, device=DEV)
        rep2 = plain.add(states[reb.groups, 0].contiguous(), reb.found.tokens, reb.found.lengths)
        target_moved = host((moved[:, 0] != states[reb.groups, 0]).flatten(1).any(dim=1))
        assert not target_moved[rows_basis == 0].any() and target_moved.sum() >= G
        assert not host(rep2.proven)[target_moved].any() and host(rep2.proven)[~target_moved].all()
    with pytest.raises(_lib.TensorGameError, match="exactly one"):
        solve_in_bases(policy, states, scalars, bases, n_samples, R)
    with pytest.raises(_lib.TensorGameError, match="exactly one"):
        solve_in_bases(policy, states, scalars, bases, n_samples, R, chunk_groups=8, slots=8)
