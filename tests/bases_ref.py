"""Host restatement of include/tensor_game_bases.h, straight from its text: ``tg_basis_inverse_i32`` in Python integers
(object arrays: the arithmetic is unbounded, as the header states its rules) and ``tg_solution_rebase`` in Python
integers too, bad rules included.  Nothing here calls the library."""
import numpy as np

BASIS_BAD_DIAGONAL, BASIS_BAD_RANGE = 1, 2
REBASE_BAD_LENGTH, REBASE_BAD_INDEX, REBASE_BAD_RANGE = 1, 2, 4
LIMIT = 1 << 28


def _units(d):
    return all(int(v) in (1, -1) for v in d)


def inv_lower(L):
    """X = L^-1 by forward substitution, column by column; reads the diagonal and the strictly lower triangle only."""
    S = L.shape[0]
    X = np.zeros((S, S), dtype=object)
    for c in range(S):
        for r in range(c, S):
            acc = int(r == c) - sum(int(L[r, k]) * X[k, c] for k in range(c, r))
            X[r, c] = int(L[r, r]) * acc
    return X


def inv_upper(U):
    """Y = U^-1 by back substitution, column by column; reads the diagonal and the strictly upper triangle only."""
    S = U.shape[0]
    Y = np.zeros((S, S), dtype=object)
    for c in range(S):
        for r in range(c, -1, -1):
            acc = int(r == c) - sum(int(U[r, k]) * Y[k, c] for k in range(r + 1, c + 1))
            Y[r, c] = int(U[r, r]) * acc
    return Y


def inverse_triple(L3, U3):
    """(inv (3,S,S) int32, status bits) of one triple; all zero when a bit is set."""
    S = L3.shape[-1]
    zero = np.zeros((3, S, S), dtype=np.int32)
    if not all(_units(np.diagonal(M)) for M in (*L3, *U3)):
        return zero, BASIS_BAD_DIAGONAL
    out = []
    for L, U in zip(L3, U3):
        X, Y = inv_lower(L), inv_upper(U)
        if any(abs(v) >= LIMIT for M in (X, Y) for v in M.flat):
            return zero, BASIS_BAD_RANGE
        P = Y.dot(X)
        if any(not -2 ** 31 <= v < 2 ** 31 for v in P.flat):
            return zero, BASIS_BAD_RANGE
        out.append(P.astype(np.int64))
    return np.stack(out).astype(np.int32), 0


def basis_inverse(lower, upper):
    """(inv int32 (N,3,S,S), bad uint8 (N), status) of ``tg_basis_inverse_i32``."""
    lower, upper = np.asarray(lower), np.asarray(upper)
    N, _, S, _ = lower.shape
    inv = np.zeros((N, 3, S, S), dtype=np.int32)
    bad = np.zeros(N, dtype=np.uint8)
    status = 0
    for n in range(N):
        inv[n], bits = inverse_triple(lower[n], upper[n])
        bad[n] = bits != 0
        status |= bits
    return inv, bad, status


def rebase_row(tokens, length, mats, g, shift):
    """(tokens_out (K,3S) int8, length_out, status bits) of one row; mats (G,3,S,S)."""
    K, A3 = tokens.shape
    S = A3 // 3
    zero = np.zeros((K, A3), dtype=np.int8)
    bits = (REBASE_BAD_LENGTH if length < 0 or length > K else 0) | (REBASE_BAD_INDEX if g < 0 or g >= len(mats) else 0)
    if bits:
        return zero, 0, bits
    out = zero.copy()
    f = tokens[:length].astype(object) - shift                       # Python integers from here on
    for x in range(3):
        moved = f[:, x * S:(x + 1) * S].dot(np.asarray(mats[g][x]).astype(object).T) + shift   # (length, S)
        if any(not -128 <= v <= 127 for v in moved.flat):
            return zero, 0, REBASE_BAD_RANGE
        out[:length, x * S:(x + 1) * S] = moved.astype(np.int64)
    return out, length, 0


def solution_rebase(tokens, lengths, mats, index, shift):
    """(tokens_out int8 (M,K,3S), lengths_out int64 (M), bad uint8 (M), status) of ``tg_solution_rebase``; ``index``
    None: row m uses triple m."""
    tokens = np.asarray(tokens, dtype=np.int8)
    M = tokens.shape[0]
    out = np.zeros_like(tokens)
    lengths_out = np.zeros(M, dtype=np.int64)
    bad = np.zeros(M, dtype=np.uint8)
    status = 0
    for m in range(M):
        g = m if index is None else int(index[m])
        out[m], lengths_out[m], bits = rebase_row(tokens[m], int(lengths[m]), mats, g, shift)
        bad[m] = bits != 0
        status |= bits
    return out, lengths_out, bad, status


# ---- seeded inputs -----------------------------------------------------------------------------------------------------
def random_factors(rng, N, S, probs=None):
    """(lower, upper) int8 (N,3,S,S): unit(+-1)-diagonal triangular factors with off-diagonal values from {-1,0,1}
    (``probs``: their weights; default min(0.15, 0.4/S) for each of -1 and +1), zeros in the other triangle."""
    if probs is None:
        p = min(0.15, 0.4 / S)
        probs = (p, 1 - 2 * p, p)
    off = rng.choice((-1, 0, 1), size=(2, N, 3, S, S), p=probs)
    diag = rng.choice((-1, 1), size=(2, N, 3, S))
    lower, upper = np.tril(off[0], -1), np.triu(off[1], 1)
    idx = np.arange(S)
    lower[..., idx, idx], upper[..., idx, idx] = diag[0], diag[1]
    return lower.astype(np.int8), upper.astype(np.int8)


def random_lists(rng, M, K, S, shift, lengths=None):
    """(tokens int8 (M,K,3S), lengths int64 (M)): factor values from {-2..2}; lengths (unless given) from 0 to K, both
    ends present when M >= 2.  The rows beyond a list's length hold arbitrary tokens, which nothing may read."""
    tokens = rng.integers(-128, 128, size=(M, K, 3 * S)).astype(np.int8)
    if lengths is None:
        lengths = rng.integers(0, K + 1, size=M)
        if M >= 2:
            lengths[0], lengths[-1] = 0, K
    lengths = np.asarray(lengths, dtype=np.int64)
    for m in range(M):
        L = int(np.clip(lengths[m], 0, K))                       # (a given length may be a bad one)
        tokens[m, :L] = (rng.choice((-2, -1, 0, 1, 2), size=(L, 3 * S), p=(0.05, 0.2, 0.5, 0.2, 0.05)) + shift).astype(np.int8)
    return tokens, lengths
