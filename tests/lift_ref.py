"""Host restatement of include/tensor_game_lift.h, straight from its text: dense uint8 elimination with the columns in
ascending order, the oracle's Philox, exact int64 sums.  No shortcuts: every column is a dense tensor, every try is
solved and summed in full, and all ``tries`` are run even after an exact one.  Nothing here calls the library."""
import numpy as np

from oracle import tensor_game as O

DOMAIN, MAX_TRIES, MAX_K = 0x4C320000, 1024, 128
OK, NOT_MOD2, INCONSISTENT, NOT_EXACT, BAD_RANK = 0, 1, 2, 3, -1
OUT_NAMES = ("status", "try_used", "unknowns", "sys_rank", "miss")


def x0_of(rows, R, S):
    """int64 (R,3,S): X0[r][d][e] = bit e of m_d(r)."""
    m = np.asarray(rows[:R]).view(np.uint32).astype(np.uint64).reshape(R, 3)
    return ((m[:, :, None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)


def term_sum(X):
    """int64 (S,S,S): sum_r X[r][0] (x) X[r][1] (x) X[r][2]."""
    return np.einsum("ri,rj,rk->ijk", X[:, 0], X[:, 1], X[:, 2])


def system(X0):
    """(support positions [(r,d,e)] in ascending order, A uint8 (S^3, N)): column c is term r with its mode-d factor
    replaced by the unit vector e, mod 2."""
    R, _, S = X0.shape
    support = [(r, d, e) for r in range(R) for d in range(3) for e in range(S) if X0[r, d, e]]
    A = np.zeros((S ** 3, len(support)), dtype=np.uint8)
    for c, (r, d, e) in enumerate(support):
        f = [X0[r, 0], X0[r, 1], X0[r, 2]]
        f[d] = np.eye(S, dtype=np.int64)[e]
        A[:, c] = (np.einsum("i,j,k->ijk", *f).reshape(-1) & 1).astype(np.uint8)
    return support, A


def eliminate(A, b):
    """Gauss-Jordan on [A | b], the columns in ascending order.  Returns (M reduced, pivot columns, free columns): row i
    of M is the pivot row of pivot column i; the rows from len(pivots) on are zero in every column of A."""
    M = np.concatenate([A, b.reshape(-1, 1)], axis=1).astype(np.uint8)
    rows, N = A.shape
    pivots, free, P = [], [], 0
    for c in range(N):
        hit = np.flatnonzero(M[P:, c]) + P
        if len(hit) == 0:          # in the span of the columns below c
            free.append(c)
            continue
        p = hit[0]
        if p != P:
            M[[P, p]] = M[[p, P]]
        other = np.flatnonzero(M[:, c])
        other = other[other != P]
        M[other] ^= M[P]
        pivots.append(c)
        P += 1
    return M, pivots, free


def free_bits(seed, g, t, n_free):
    """uint8 (n_free,): free variable f at try t of the list with the global id g."""
    if t == 0 or n_free == 0:
        return np.zeros(n_free, dtype=np.uint8)
    blocks = (n_free + 127) // 128
    ctr = np.zeros((blocks, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, t
    ctr[:, 3] = (DOMAIN + np.arange(blocks)).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    o = O.philox4x32_10(ctr, np.broadcast_to(key, (blocks, 2))).astype(np.uint64)    # (blocks, 4)
    f = np.arange(n_free)
    return ((o[f >> 7, (f >> 5) & 3] >> (f & 31).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def lift_one(target, rows, R, S, shift, seed, g, tries, detail=None):
    """(tokens int8 (K,3S), status, try_used, unknowns, sys_rank, miss) of one list.  ``detail`` (a dict) receives the
    pivot columns, the matrix and the miss of every try."""
    K = rows.shape[0]
    zero = np.zeros((K, 3 * S), dtype=np.int8)
    if R < 0 or R > K:
        return zero, BAD_RANK, -1, 0, 0, -1
    target = np.asarray(target).astype(np.int64)
    X0 = x0_of(rows, R, S)
    D = target - term_sum(X0)
    if (D & 1).any():
        return zero, NOT_MOD2, -1, 0, 0, int((D & 1).sum())
    support, A = system(X0)
    N = len(support)
    b = ((D >> 1) & 1).astype(np.uint8).reshape(-1)
    M, pivots, free = eliminate(A, b)
    P = len(pivots)
    if detail is not None:
        detail.update(A=A, b=b, pivots=pivots, free=free, support=support, misses=[])
    if M[P:, N].any():
        return zero, INCONSISTENT, -1, N, P, -1
    best, used, tokens = None, -1, zero
    for t in range(tries):
        x = np.zeros(N, dtype=np.uint8)
        xf = free_bits(seed, g, t, len(free))
        x[free] = xf
        if P:
            x[pivots] = M[:P, N] ^ ((M[:P][:, free].astype(np.int64) @ xf.astype(np.int64)) & 1).astype(np.uint8)
        if t < 2:                  # x solves the system (a check of this restatement itself; dense, so not every try)
            assert np.array_equal((A.astype(np.int64) @ x.astype(np.int64)) & 1, b)
        X = X0.copy()
        for c, (r, d, e) in enumerate(support):
            if x[c]:
                X[r, d, e] = -1
        miss = int(np.count_nonzero(target - term_sum(X)))
        if detail is not None:
            detail["misses"].append(miss)
        best = miss if best is None else min(best, miss)
        if miss == 0 and used < 0:
            used = t
            tokens = zero.copy()
            tokens[:R] = (X.reshape(R, 3 * S) + shift).astype(np.int8)
    if used >= 0:
        return tokens, OK, used, N, P, 0
    return zero, NOT_EXACT, -1, N, P, best


def lift(targets, lists, ranks, S, shift=1, seed=0, list0=0, tries=32):
    """``tg_lift2_signs`` of W lists: dict of tokens int8 (W,K,3S) and status, try_used, unknowns, sys_rank, miss int32
    (W,)."""
    W, K = lists.shape[0], lists.shape[1]
    out = {"tokens": np.zeros((W, K, 3 * S), dtype=np.int8), **{k: np.zeros(W, dtype=np.int32) for k in OUT_NAMES}}
    for w in range(W):
        res = lift_one(targets[w], lists[w], int(ranks[w]), S, shift, seed, (list0 + w) & (2 ** 64 - 1), tries)
        out["tokens"][w] = res[0]
        for k, v in zip(OUT_NAMES, res[1:]):
            out[k][w] = v
    return out


def masks_of_tokens(tokens, L, S, shift):
    """int32 (K,3): the mask rows of a token list taken mod 2 (no term is dropped, nothing is reduced)."""
    K = tokens.shape[0]
    f = (np.asarray(tokens[:L], dtype=np.int64) - shift) & 1
    m = (f.reshape(L, 3, S).astype(np.uint64) << np.arange(S, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    out = np.zeros((K, 3), dtype=np.uint32)
    out[:L] = m
    return out.view(np.int32)


def tokens_sum(tokens, L, S, shift):
    """int64 (S,S,S): the exact sum of a token list."""
    f = np.asarray(tokens[:L], dtype=np.int64) - shift
    return term_sum(f.reshape(L, 3, S))


def kron_lists(ta, La, na, tb, Lb, nb, shift):
    """The tensor product of two matrix-multiplication lists (<na,na,na> and <nb,nb,nb>, token rows + shift) as a
    <na nb, na nb, na nb> list: int8 (La Lb, 3 (na nb)^2).  Entry (i, j) of a factor matrix of the product is
    a[i // nb, j // nb] * b[i % nb, j % nb]."""
    Sa, Sb, n = na * na, nb * nb, na * nb
    fa = (np.asarray(ta[:La], dtype=np.int64) - shift).reshape(La, 3, na, na)
    fb = (np.asarray(tb[:Lb], dtype=np.int64) - shift).reshape(Lb, 3, nb, nb)
    out = np.einsum("adij,bdkl->abdikjl", fa, fb).reshape(La * Lb, 3 * n * n)
    assert Sa * Sb == n * n
    return (out + shift).astype(np.int8)
