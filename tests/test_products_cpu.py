"""CPU checks of the half-precision block products (include/tensor_game_products.h): the header, the exported symbols,
every refusal of the host side of the library and of the bindings, and the restatement's own checks -- its two roundings
on ties and overflow, and integer matrices multiplied exactly through ``encoded`` and an int64 product, which is what
test_gpu_products.py relies on."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import _lib, build, ops

import bilinear_rect_ref as RR
import bilinear_ref as BR
import products_ref as PR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_products.h"
ENTRIES = ["tg_bilinear_products_bf16", "tg_bilinear_products_check", "tg_bilinear_products_f16"]


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_products_header_is_plain_c_and_states_the_rule():
    text = " ".join(re.sub(r"\n \*", "\n", HDR.read_text()).split())      # the comment's line breaks do not matter
    for words in ("that of tensor_game_rect.h, word for word", "on the grid n x m with part 0", "m x p with part 1",
                  "tokens[r][d*S + e] - shift", "converts to float32 exactly", "rn_H(acc)", "starts at +0", "ascending e",
                  "a zero coefficient contributes nothing", "round(c * x)", "round(acc + t)", "no fused multiply-add",
                  "ties to even", "overflow to infinity", "Each product is exact in float32", "are not fixed",
                  "q * 2^-23 * sum_k |Ahat_r[y][k] * Bhat_r[k][x]|", "derived, not", "integer below 2^24",
                  "no atomics and no split-K", "changes no bit", "sign of a zero result", "payload of a NaN", "Denormals",
                  "must not overlap", "64-bit", "multiples of 8 elements", "before any launch and names the argument",
                  "no allocation", "no host sync", "capturable"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_products_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ENTRIES == sorted(_lib.PRODUCTS_SIGNATURES)
    assert HDR in build.HEADERS and (build.CSRC / "tg_products.hip") in build.SOURCES
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    for name in ("bilinear_products_check", "bilinear_products"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    assert "FusedBilinearMatmul" in mat_mul_amd.__all__ and "FusedBilinearMatmul" in mat_mul_amd.bilinear.__all__
    assert mat_mul_amd.FusedBilinearMatmul is mat_mul_amd.bilinear.FusedBilinearMatmul


# ---- tg_bilinear_products_check and the entries --------------------------------------------------------------------------
OK_SIZES = dict(batch=2, P=4, Q=6, T=9, lda=8, stride_a=32, ldb=10, stride_b=60, R=11, S=7, n=2, m=2, p=3, shift=1)
REFUSALS = [(dict(n=0), "n=0 < 1"), (dict(m=0), "m=0 < 1"), (dict(p=-1), "p=-1 < 1"), (dict(S=0), "S=0"), (dict(S=33), "S=33"),
            (dict(n=4, P=4), "n*m=8 above S=7"), (dict(S=5), "m*p=6 above S=5"),
            (dict(n=3, m=1, p=3, P=3, S=8), "n*p=9 above S=8"), (dict(n=2 ** 16, m=2 ** 16), "n*m="),
            (dict(R=0), "R=0"), (dict(R=257), "R=257"), (dict(shift=-1), "shift=-1"), (dict(shift=65), "shift=65"),
            (dict(batch=-1), "batch=-1"), (dict(P=0), "P=0"), (dict(P=5), "P=5 is no positive multiple of n=2"),
            (dict(Q=0), "Q=0"), (dict(Q=7), "Q=7 is no positive multiple of m=2"), (dict(T=0), "T=0"),
            (dict(T=10), "T=10 is no positive multiple of p=3"), (dict(lda=5), "lda=5 < Q=6"), (dict(ldb=8), "ldb=8 < T=9"),
            (dict(stride_a=31), "stride_a=31 < P*lda=32"), (dict(stride_b=59), "stride_b=59 < Q*ldb=60"),
            (dict(batch=2 ** 61), "byte offset"), (dict(P=2 ** 40, lda=2 ** 40, batch=1), "byte offset"),
            (dict(Q=2 ** 40, ldb=2 ** 40, batch=1, lda=2 ** 40), "byte offset"),
            (dict(batch=1, P=2 ** 31, T=3 * 2 ** 30, ldb=3 * 2 ** 30, R=256), "byte offset of M")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_bilinear_products_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)) as info:
        ops.bilinear_products_check(**{**OK_SIZES, **over})
    assert str(info.value).count("tg_bilinear_products_check: ") == 1


def test_bilinear_products_check_takes_the_limits():
    ops.bilinear_products_check(**OK_SIZES)
    ops.bilinear_products_check(0, 32, 1, 1, R=256, S=32, n=32, m=1, p=1, shift=64)
    ops.bilinear_products_check(1, 1, 1, 1, 1, 0, 1, 0, R=1, S=1, n=1, m=1, p=1, shift=0)   # strides count from batch 2 on
    ops.bilinear_products_check(1 << 40, 4, 4, 4, R=256, S=32, n=4, m=4, p=4)
    ops.bilinear_products_check(3, 10, 10, 18, S=30, n=5, m=5, p=6)                        # ld and strides default to dense
    ops.bilinear_products_check(3, 1, 32, 1, S=32, n=1, m=32, p=1)
    ops.bilinear_products_check(**{**OK_SIZES, "S": 6})                                     # S = max(n*m, m*p, n*p)


def test_products_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    order = ("A", "B", "batch", "P", "Q", "T", "lda", "stride_a", "ldb", "stride_b", "tokens", "R", "S", "n", "m", "p",
             "shift", "M")
    sizes = dict(batch=2, P=4, Q=6, T=9, lda=6, stride_a=24, ldb=9, stride_b=54, R=11, S=6, n=2, m=2, p=3, shift=1)
    # A spans 24 + 3*6 + 6 = 48 elements (96 bytes), B 54 + 5*9 + 9 = 108 (216 bytes), M 2*11*2*3 = 132 floats (528
    # bytes), the list 11 * 18 = 198 bytes
    ok = dict(A=p(1 << 16), B=p(1 << 18), tokens=p(1 << 12), M=p(1 << 20), **sizes)
    cases = [(dict(S=33), b"S=33"), (dict(n=0), b"n=0"), (dict(S=5), b"m*p=6 above S=5"), (dict(R=257), b"R=257"),
             (dict(shift=65), b"shift=65"), (dict(P=5), b"P=5"), (dict(Q=5), b"Q=5"), (dict(T=8), b"T=8"),
             (dict(lda=5), b"lda=5"), (dict(ldb=8), b"ldb=8"), (dict(stride_a=23), b"stride_a=23"),
             (dict(stride_b=53), b"stride_b=53"), (dict(batch=-1), b"batch=-1"),
             (dict(A=None), b"null A"), (dict(B=None), b"null B"), (dict(tokens=None), b"null tokens"),
             (dict(M=None), b"null M"),
             (dict(A=p((1 << 16) + 1)), b"A not 2-byte aligned"), (dict(B=p((1 << 18) + 1)), b"B not 2-byte aligned"),
             (dict(M=p((1 << 20) + 2)), b"M not 4-byte aligned"),
             (dict(M=p((1 << 16) + 96 - 4)), b"A and M overlap"),         # A's last element
             (dict(A=p((1 << 20) + 528 - 2)), b"A and M overlap"),        # M's last element
             (dict(M=p((1 << 16) - 528 + 4)), b"A and M overlap"),
             (dict(M=p((1 << 18) + 216 - 4)), b"B and M overlap"),
             (dict(B=p((1 << 20) + 528 - 2)), b"B and M overlap"),
             (dict(M=p((1 << 18) - 528 + 4)), b"B and M overlap"),
             (dict(tokens=p((1 << 20) + 8)), b"tokens and M overlap"),
             (dict(tokens=p((1 << 20) - 198 + 1)), b"tokens and M overlap")]
    for sfx in ("bf16", "f16"):
        fn = getattr(_lib.lib, f"tg_bilinear_products_{sfx}")
        for over, words in cases:
            kw = {**ok, **over}
            assert fn(*[kw[k] for k in order], None) == -1, (sfx, over)
            err = _lib.lib.tg_last_error()
            assert err.startswith(f"tg_bilinear_products_{sfx}: ".encode()) and words in err, (sfx, over, err)
        assert fn(None, None, 0, 4, 6, 9, 6, 24, 9, 54, None, 11, 6, 2, 2, 3, 1, None, None) == 0    # batch = 0 returns at once
        assert fn(None, None, 0, 4, 6, 9, 6, 24, 9, 54, None, 11, 5, 2, 2, 3, 1, None, None) == -1   # ... after the size checks


def test_products_bindings_refuse_cpu_tensors():
    A, B = torch.zeros((2, 4, 4), dtype=torch.bfloat16), torch.zeros((2, 4, 6), dtype=torch.bfloat16)
    tok = mat_mul_amd.standard_rect(2, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.bilinear_products(A, B, tok, 12, 2, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FusedBilinearMatmul(tok, 12, 2, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FusedBilinearMatmul.__call__(object.__new__(mat_mul_amd.FusedBilinearMatmul), A, B)


# ---- the restatement on its own ----------------------------------------------------------------------------------------
def test_both_roundings_send_ties_to_even_and_overflow_to_infinity():
    f32 = lambda *v: np.array(v, dtype=np.float32)
    # bfloat16 keeps 8 significant bits: the spacing in [1, 2) is 2^-7
    x = f32(1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, -(1 + 2.0 ** -8),
            -(1 + 2.0 ** -7 + 2.0 ** -8), 0.0, 3.0, 256.0, 257.0, 259.0)
    want = f32(1, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1, -1, -(1 + 2.0 ** -6), 0, 3, 256, 256, 260)
    assert np.array_equal(PR.rn_bf16(x), want)
    big = f32(np.finfo(np.float32).max, -np.finfo(np.float32).max, 2.0 ** 127 * (2 - 2.0 ** -8), 2.0 ** 127 * (2 - 2.0 ** -7),
              np.inf, -np.inf)
    assert np.array_equal(PR.rn_bf16(big), f32(np.inf, -np.inf, np.inf, 2.0 ** 127 * (2 - 2.0 ** -7), np.inf, -np.inf))
    assert np.isnan(PR.rn_bf16(f32(np.nan)))[0] and PR.rn_bf16(np.zeros((2, 3), dtype=np.float32)).shape == (2, 3)
    # binary16 keeps 11: the spacing in [1, 2) is 2^-10, the largest value 65 504, and 65 520 is the tie that overflows
    x = f32(1 + 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, -(1 + 2.0 ** -11), 2049, 2051, 65504,
            65519, 65520, -65520, 1e9)
    want = f32(1, 1 + 2.0 ** -9, 1 + 2.0 ** -10, -1, 2048, 2052, 65504, 65504, np.inf, -np.inf, np.inf)
    assert np.array_equal(PR.rn_f16(x), want)
    for H in PR.TYPES:                                              # every value of H is a fixed point
        v = PR.RN[H](np.random.default_rng(0).standard_normal(1000).astype(np.float32))
        assert np.array_equal(PR.RN[H](v), v)
        ints = np.arange(-PR.EXACT_INTEGERS[H], PR.EXACT_INTEGERS[H] + 1, dtype=np.float32)
        assert np.array_equal(PR.RN[H](ints), ints) and PR.RN[H](f32(PR.EXACT_INTEGERS[H] + 1))[0] != PR.EXACT_INTEGERS[H] + 1


def _strassen(golden):
    return BR.coefficients(golden("strassen")["tokens"], 7, 1)


@pytest.mark.parametrize("H", PR.TYPES)
@pytest.mark.parametrize("name", ["strassen", "kron", "223"])
def test_integer_matrices_multiply_exactly_through_encoded_and_int64(golden, name, H):
    f, (n, m, p) = {"strassen": (_strassen(golden), (2, 2, 2)),
                    "kron": (BR.kron(_strassen(golden), 2, _strassen(golden), 2), (4, 4, 4)),
                    "223": (RR.standard_rect(2, 2, 3), (2, 2, 3))}[name]
    rng = np.random.default_rng(len(f))
    q = 5
    assert PR.exact_ok(f, n, m, p, 3, q, H) and not PR.exact_ok(f, n, m, p, 3, 2 ** 24, H)
    assert not PR.exact_ok(f, n, m, p, PR.EXACT_INTEGERS[H] + 1, 1, H)
    A = rng.integers(-3, 4, size=(2, 3 * n, q * m)).astype(np.float32)
    B = rng.integers(-3, 4, size=(2, q * m, 2 * p)).astype(np.float32)
    Ah, Bh = PR.encoded(f, n, m, 0, A, H), PR.encoded(f, m, p, 1, B, H)
    assert np.array_equal(Ah, RR.encode(f, n, m, 0, A.astype(np.int64))) and Ah.shape == (2, len(f), 3, q)
    M = np.matmul(Ah.astype(np.int64), Bh.astype(np.int64))
    assert np.array_equal(PR.products64(Ah, Bh), M) and (PR.bound(Ah, Bh) >= 0).all()
    assert np.array_equal(RR.decode(f, n, p, M), A.astype(np.int64) @ B.astype(np.int64))
    assert np.array_equal(PR.multiply(f, n, m, p, A, B, H), (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32))


def test_encoded_rounds_once_after_the_float32_sum():
    # u = (1, 1): 1 + 2^-9 is exact in float32 and a tie in bfloat16 (to even: 1); a restatement that rounded the operands'
    # sum in H step by step, or truncated, gives the same here, so the second case adds a term: (1 + 2^-8) + 2^-16 is above
    # the tie in float32 and rounds up, while rounding after each term loses the 2^-16
    f = np.zeros((1, 9), dtype=np.int64)
    f[0, :3] = 1
    X = np.array([[[1.0, 2.0 ** -9, 0.0]]], dtype=np.float32)
    assert PR.encoded(f, 1, 3, 0, X, "bf16")[0, 0, 0, 0] == 1.0
    X = np.array([[[1.0, 2.0 ** -8, 2.0 ** -16]]], dtype=np.float32)
    assert PR.encoded(f, 1, 3, 0, X, "bf16")[0, 0, 0, 0] == np.float32(1 + 2.0 ** -7)
    with pytest.raises(AssertionError, match="values of H"):
        PR.encoded(f, 1, 3, 0, np.array([[[1 + 2.0 ** -9, 0, 0]]], dtype=np.float32), "bf16")
