"""A numpy restatement of include/tensor_game_rect.h (of the header's words, not of the kernels): the target <n,m,p> in a
cube of size S, the schoolbook list, and the two linear halves on a gr x gc grid.  A list is its coefficients ``f``: int64
(R,3S), row r = cat(u_r, v_r, w_r) = tokens[r] - shift; part d uses f[r, d*S : d*S + gr*gc] and nothing behind it.

``encode`` and ``decode`` work in the dtype of their operand, one rounding per operation: float32 and float64 arrays give
what the header defines bit for bit, int64 arrays the exact value."""
import numpy as np


def cube_size(n, m, p):
    return max(n * m, m * p, n * p)


def matmul_target(n, m, p, S=None):
    """T[i*m+j, j*p+k, i*p+k] = 1 for A n x m, B m x p, C n x p; 0 elsewhere, the padding included."""
    S = cube_size(n, m, p) if S is None else S
    assert S >= cube_size(n, m, p)
    T = np.zeros((S, S, S), dtype=np.int64)
    for i in range(n):
        for j in range(m):
            for k in range(p):
                T[i * m + j, j * p + k, i * p + k] = 1
    return T


def standard_rect(n, m, p, S=None):
    """The n*m*p terms a_ij (x) b_jk (x) c_ik in ascending (i, j, k), as coefficients."""
    S = cube_size(n, m, p) if S is None else S
    f = np.zeros((n * m * p, 3 * S), dtype=np.int64)
    t = 0
    for i in range(n):
        for j in range(m):
            for k in range(p):
                f[t, i * m + j] = f[t, S + j * p + k] = f[t, 2 * S + i * p + k] = 1
                t += 1
    return f


def term_sum(f):
    S = f.shape[1] // 3
    return np.einsum("ra,rb,rc->abc", f[:, :S], f[:, S:2 * S], f[:, 2 * S:])


def _block(X, e, gc, h, w):
    return X[:, (e // gc) * h:(e // gc + 1) * h, (e % gc) * w:(e % gc + 1) * w]


def encode(f, gr, gc, part, X):
    """Y (batch,R,h,w) of X (batch,rows,cols) on the grid gr x gc: the accumulator starts at +0, the terms come in
    ascending e < gr*gc, a zero coefficient is skipped, a non-zero one adds round(c * x) with one more rounding."""
    S = f.shape[1] // 3
    batch, rows, cols = X.shape
    assert rows % gr == 0 and cols % gc == 0 and gr * gc <= S
    h, w = rows // gr, cols // gc
    Y = np.zeros((batch, len(f), h, w), dtype=X.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(f)):
            acc = Y[:, r]
            for e in range(gr * gc):
                c = int(f[r, part * S + e])
                if c:
                    acc = acc + X.dtype.type(c) * _block(X, e, gc, h, w)
            Y[:, r] = acc
    return Y


def decode(f, gr, gc, M):
    """C (batch,gr*h,gc*w) of M (batch,R,h,w): block e = sum_r w_r[e] * M[:, r], ascending r, by the same rule."""
    S = f.shape[1] // 3
    batch, R, h, w = M.shape
    assert R == len(f) and gr * gc <= S
    C = np.zeros((batch, gr * h, gc * w), dtype=M.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(gr * gc):
            acc = _block(C, e, gc, h, w).copy()
            for r in range(R):
                k = int(f[r, 2 * S + e])
                if k:
                    acc = acc + M.dtype.type(k) * M[:, r]
            _block(C, e, gc, h, w)[...] = acc
    return C


def multiply(f, n, m, p, A, B, levels=1):
    """A (batch,P,Q) times B (batch,Q,T) by the algorithm f for <n,m,p>, ``levels`` deep: A on the grid n x m with part
    0, B on m x p with part 1, the block products by numpy in the operands' dtype, C on n x p."""
    a, b = A, B
    for _ in range(levels):
        a = encode(f, n, m, 0, a)
        b = encode(f, m, p, 1, b)
        a, b = a.reshape(-1, *a.shape[2:]), b.reshape(-1, *b.shape[2:])
    mm = np.matmul(a, b)
    for _ in range(levels):
        mm = decode(f, n, p, mm.reshape(-1, len(f), *mm.shape[1:]))
    return mm


def exact_bound(f, levels, q, inner):
    """As bilinear_ref.exact_bound: the largest magnitude an intermediate can reach for integer inputs in [-q, q] and a
    leaf whose inner dimension is ``inner``.  Below 2^24 (2^53) every float32 (float64) operation of the run is exact."""
    S = f.shape[1] // 3
    alpha = int(np.abs(f[:, :S]).sum(axis=1).max())
    beta = int(np.abs(f[:, S:2 * S]).sum(axis=1).max())
    gamma = int(np.abs(f[:, 2 * S:]).sum(axis=0).max())
    a = b = worst = q
    for _ in range(levels):
        a, b = a * alpha, b * beta
        worst = max(worst, a, b)
    mm = inner * a * b
    worst = max(worst, mm)
    for _ in range(levels):
        mm *= gamma
        worst = max(worst, mm)
    return worst


def apply_symmetry(row, f):
    """The rows f (R,3S) under one element (uint8 (3S+1), include/tensor_game_symmetry.h): f^g[d*S + a] = s * f[rho[d]*S +
    pi_d[a]], with rho from the mode code and (pi, s) from the low seven bits and the top bit of each byte."""
    rho = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)][int(row[0])]
    S = (len(row) - 1) // 3
    idx = (row[1:] & 0x7F).astype(np.int64)
    sign = np.where(row[1:] & 0x80, -1, 1)
    src = np.repeat(np.array(rho), S) * S + idx
    return sign[None] * f[:, src]
