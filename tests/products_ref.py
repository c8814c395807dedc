"""A numpy restatement of include/tensor_game_products.h (of the header's words, not of the kernel).  H is "bf16" or "f16";
a value of H is carried as the float32 it converts to exactly (rule 1), so every array here is float32 unless it says
otherwise.  A list is its coefficients ``f`` as in bilinear_rect_ref.py: int64 (R,3S), row r = tokens[r] - shift."""
import numpy as np

import bilinear_rect_ref as RR

TYPES = ("bf16", "f16")
# the largest n such that every integer of magnitude <= n is a value of H (8 and 11 significant bits)
EXACT_INTEGERS = {"bf16": 2 ** 8, "f16": 2 ** 11}


def rn_bf16(x):
    """IEEE round-to-nearest-even from float32 to bfloat16, overflow to infinity, by integer arithmetic on the float32
    bits: half an ulp of the kept 16 bits less one, plus the lowest kept bit, carries into them exactly when the value
    rounds up.  Returns the float32 of the result."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    r = np.where(np.isnan(x), (b | 0x00400000) & 0xFFFF0000, r)          # a NaN stays one (its payload is not defined)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def rn_f16(x):
    """The same to IEEE binary16, through numpy's float16."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


RN = {"bf16": rn_bf16, "f16": rn_f16}


def encoded(f, gr, gc, part, X, H):
    """Ahat (part 0, grid n x m) or Bhat (part 1, grid m x p) of rule 2, every bit defined: the float32 block combination
    of bilinear_rect_ref.encode, then one rounding to H.  X float32 (batch,rows,cols) holding values of H."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and np.array_equal(RN[H](X), X, equal_nan=True), "X must hold values of H"
    return RN[H](RR.encode(f, gr, gc, part, X))


def products64(Ah, Bh):
    """s of rule 3 in float64: (batch,R,h,q) @ (batch,R,q,w).  Every product of two values of H is exact in float64, and
    the float64 sum's error is 2^-29 of the bound's unit."""
    return np.matmul(Ah.astype(np.float64), Bh.astype(np.float64))


def bound(Ah, Bh):
    """q * 2^-23 * sum_k |Ahat * Bhat| of rule 3, in float64."""
    return Ah.shape[-1] * 2.0 ** -23 * np.matmul(np.abs(Ah).astype(np.float64), np.abs(Bh).astype(np.float64))


def exact_ok(f, n, m, p, qmax, inner, H):
    """True when integer inputs in [-qmax, qmax] keep every encoded value an integer that is a value of H (so that no
    rounding of rule 2 happens, the float32 sums before it included) and every sum of rule 3 and of the float32 decode on
    n x p below 2^24, for an inner block size q = ``inner``: the whole run is then exact."""
    S = f.shape[1] // 3
    alpha = int(np.abs(f[:, :n * m]).sum(axis=1).max())
    beta = int(np.abs(f[:, S:S + m * p]).sum(axis=1).max())
    gamma = int(np.abs(f[:, 2 * S:2 * S + n * p]).sum(axis=0).max())
    a, b = alpha * qmax, beta * qmax
    return max(a, b) <= EXACT_INTEGERS[H] and gamma * inner * a * b < 2 ** 24


def multiply(f, n, m, p, A, B, H):
    """The whole algorithm as the restatement runs it: ``encoded``, a float32 numpy matmul, the float32 decode."""
    Ah, Bh = encoded(f, n, m, 0, A, H), encoded(f, m, p, 1, B, H)
    return RR.decode(f, n, p, np.matmul(Ah, Bh))
