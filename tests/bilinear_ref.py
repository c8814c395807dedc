"""A numpy restatement of include/tensor_game_bilinear.h (of the header's words, not of the kernels), and the lists the
bilinear tests use.  A list is its coefficients ``f``: int64 (R,3S), row r = cat(u_r, v_r, w_r) = tokens[r] - shift.

``encode`` and ``decode`` work in the dtype of their operand, one rounding per operation: float32 and float64 arrays give
what the header defines bit for bit, int64 arrays the exact value."""
import numpy as np


def coefficients(tokens, R, shift):
    """f of the first R rows of a token table, taken in a wide type."""
    return np.asarray(tokens)[:R].astype(np.int64) - shift


def as_tokens(f, shift=1, K=None):
    """int8 (K,3S): the rows of f as tokens, zero bytes behind them."""
    f = np.asarray(f)
    out = np.zeros((len(f) if K is None else K, f.shape[1]), dtype=np.int8)
    out[:len(f)] = f + shift
    return out


def _block(X, a, n, h, w):
    return X[:, (a // n) * h:(a // n + 1) * h, (a % n) * w:(a % n + 1) * w]


def encode(f, n, mode, X):
    """Y (batch,R,h,w) of X (batch,rows,cols): the accumulator starts at +0, the terms come in ascending a, a zero
    coefficient is skipped, a non-zero one adds round(c * x) with one more rounding."""
    S = n * n
    batch, rows, cols = X.shape
    h, w = rows // n, cols // n
    Y = np.zeros((batch, len(f), h, w), dtype=X.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(f)):
            acc = Y[:, r]
            for a in range(S):
                c = int(f[r, mode * S + a])
                if c:
                    acc = acc + X.dtype.type(c) * _block(X, a, n, h, w)
            Y[:, r] = acc
    return Y


def decode(f, n, M):
    """C (batch,n*h,n*w) of M (batch,R,h,w): block c = sum_r w_r[c] * M[:, r], ascending r, by the same rule."""
    S = n * n
    batch, R, h, w = M.shape
    assert R == len(f)
    C = np.zeros((batch, n * h, n * w), dtype=M.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(S):
            acc = _block(C, c, n, h, w).copy()
            for r in range(R):
                k = int(f[r, 2 * S + c])
                if k:
                    acc = acc + M.dtype.type(k) * M[:, r]
            _block(C, c, n, h, w)[...] = acc
    return C


def multiply(f, n, A, B, levels=1):
    """A (batch,P,Q) times B (batch,Q,T) by the algorithm f, ``levels`` deep, the block products by numpy in the
    operands' dtype."""
    a, b = A, B
    for _ in range(levels):
        a = encode(f, n, 0, a)
        b = encode(f, n, 1, b)
        a, b = a.reshape(-1, *a.shape[2:]), b.reshape(-1, *b.shape[2:])
    m = np.matmul(a, b)
    for _ in range(levels):
        m = decode(f, n, m.reshape(-1, len(f), *m.shape[1:]))
    return m


def matmul_tensor(n):
    """<n,n,n> as build_matmul_tensor writes it: entry (i*n+j, j*n+k, i*n+k) is 1."""
    S = n * n
    T = np.zeros((S, S, S), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                T[i * n + j, j * n + k, i * n + k] = 1
    return T


def term_sum(f, n):
    S = n * n
    return np.einsum("ra,rb,rc->abc", f[:, :S], f[:, S:2 * S], f[:, 2 * S:])


def standard(n):
    """The n^3 terms a_ij (x) b_jk (x) c_ik."""
    S = n * n
    f = np.zeros((n ** 3, 3 * S), dtype=np.int64)
    t = 0
    for i in range(n):
        for j in range(n):
            for k in range(n):
                f[t, i * n + j] = f[t, S + j * n + k] = f[t, 2 * S + i * n + k] = 1
                t += 1
    return f


def kron(f1, n1, f2, n2):
    """The Kronecker product of two algorithms, an algorithm for n = n1*n2: term r1*R2 + r2 has
    u[(i1*n2+i2)*n + (j1*n2+j2)] = u1[i1*n1+j1] * u2[i2*n2+j2], and likewise v and w."""
    n, S1, S2 = n1 * n2, n1 * n1, n2 * n2
    S = n * n
    f = np.zeros((len(f1) * len(f2), 3 * S), dtype=np.int64)
    for r1 in range(len(f1)):
        for r2 in range(len(f2)):
            row = f[r1 * len(f2) + r2]
            for m in range(3):
                x1 = f1[r1, m * S1:(m + 1) * S1].reshape(n1, n1)
                x2 = f2[r2, m * S2:(m + 1) * S2].reshape(n2, n2)
                # entry [i1, i2, j1, j2] -> row i1*n2+i2, column j1*n2+j2
                row[m * S:(m + 1) * S] = np.einsum("ij,kl->ikjl", x1, x2).reshape(S)
    return f


def exact_bound(f, n, levels, q, inner):
    """The largest magnitude an intermediate (a partial sum included) can reach for integer inputs in [-q, q] and a leaf
    whose inner dimension is ``inner``: each encode multiplies a bound by the largest row sum of |u| (|v|), the leaf gives
    inner * bound_a * bound_b, each decode multiplies by the largest column sum of |w|.  Below 2^24 (2^53) every float32
    (float64) operation of the run is exact."""
    S = n * n
    alpha = int(np.abs(f[:, :S]).sum(axis=1).max())
    beta = int(np.abs(f[:, S:2 * S]).sum(axis=1).max())
    gamma = int(np.abs(f[:, 2 * S:]).sum(axis=0).max())
    a = b = q
    worst = q
    for _ in range(levels):
        a, b = a * alpha, b * beta
        worst = max(worst, a, b)
    m = inner * a * b
    worst = max(worst, m)
    for _ in range(levels):
        m *= gamma
        worst = max(worst, m)
    return worst
