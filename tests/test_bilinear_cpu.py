"""CPU checks of the bilinear entries (include/tensor_game_bilinear.h): the header, the exported symbols, the size checks
and the refusals of the host side of the library, and the host restatement's own checks of the index convention -- the
standard lists, Strassen's and its Kronecker square multiply matrices exactly, on rectangular blocks, which is what
test_gpu_bilinear.py relies on."""
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

import bilinear_ref as BR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_bilinear.h"
ENTRIES = ["tg_bilinear_check", "tg_bilinear_decode_f32", "tg_bilinear_decode_f64", "tg_bilinear_encode_f32",
           "tg_bilinear_encode_f64"]


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_bilinear_header_is_plain_c_and_states_the_rule():
    text = HDR.read_text()
    for words in ("a = i*n + j, b = j*n + k, c = i*n + k", "The accumulator starts at +0", "ascending a (encode)",
                  "ascending r (decode)", "A zero coefficient contributes nothing", "round(c * x)", "round(acc + t)",
                  "no fused multiply-add", "it gets +0", "must not overlap", "Denormal", "64-bit"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_bilinear_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ENTRIES == sorted(_lib.BILINEAR_SIGNATURES)
    assert HDR in build.HEADERS and _lib.TG_ABI_VERSION == 4 == _lib.lib.tg_abi_version()
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert (_lib.TG_BILINEAR_MIN_N, _lib.TG_BILINEAR_MAX_N) == (2, 5)
    for name in ("bilinear_check", "bilinear_encode", "bilinear_decode"):
        assert name in ops.__all__
    assert "BilinearMatmul" in mat_mul_amd.__all__ and mat_mul_amd.bilinear.BilinearMatmul is mat_mul_amd.BilinearMatmul


OK_SIZES = dict(batch=2, rows=4, cols=6, ld=8, batch_stride=32, R=7, n=2, mode=0, shift=1, elem_bytes=4)
REFUSALS = [(dict(n=1), "n=1"), (dict(n=6), "n=6"), (dict(R=0), "R=0"), (dict(R=257), "R=257"), (dict(shift=-1), "shift=-1"),
            (dict(shift=65), "shift=65"), (dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"), (dict(batch=-1), "batch=-1"),
            (dict(rows=0), "rows=0"), (dict(rows=5), "rows=5"), (dict(cols=0), "cols=0"), (dict(cols=7, ld=7), "cols=7"),
            (dict(ld=5), "ld=5"), (dict(batch_stride=31), "batch_stride=31"), (dict(elem_bytes=2), "elem_bytes=2"),
            (dict(elem_bytes=16), "elem_bytes=16"), (dict(batch=2 ** 61), "byte offset"),
            (dict(rows=2 ** 40, ld=2 ** 40, batch=1), "byte offset")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_bilinear_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.bilinear_check(**{**OK_SIZES, **over})


def test_bilinear_check_takes_the_limits():
    ops.bilinear_check(**OK_SIZES)
    ops.bilinear_check(0, 5, 5, 5, 0, R=256, n=5, mode=1, shift=64, elem_bytes=8)
    ops.bilinear_check(1, 2, 2, 2, 0, R=1, n=2, mode=0, shift=0, elem_bytes=4)   # batch_stride counts from batch 2 on
    ops.bilinear_check(2, 2, 2, 2, 4, R=1, n=2)
    ops.bilinear_check(1 << 40, 4, 4, R=256, n=2)                                # a recursive call's batch
    ops.bilinear_check(3, 6, 9, n=3)                                             # ld and batch_stride default to dense


def test_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    order_e = ("X", "batch", "rows", "cols", "ld", "batch_stride", "tokens", "R", "n", "mode", "shift", "Y")
    order_d = ("M", "batch", "rows", "cols", "ld", "batch_stride", "tokens", "R", "n", "shift", "C")
    sizes = dict(batch=2, rows=4, cols=4, ld=4, batch_stride=16, R=7, n=2, shift=1)
    # X spans ((2-1)*16 + 3*4 + 4) * 4 = 128 bytes (256 as f64); Y 2*7*2*2*4 = 224 (448)
    ok_e = dict(X=p(1 << 16), tokens=p(1 << 12), Y=p(1 << 20), mode=0, **sizes)
    ok_d = dict(M=p(1 << 20), tokens=p(1 << 12), C=p(1 << 16), **sizes)
    both = [(dict(n=6), b"n=6"), (dict(R=257), b"R=257"), (dict(shift=65), b"shift=65"), (dict(rows=5), b"rows=5"),
            (dict(rows=6, cols=2, n=3), b"cols=2"), (dict(ld=3), b"ld=3"), (dict(batch_stride=15), b"batch_stride=15"),
            (dict(batch=-1), b"batch=-1"), (dict(tokens=None), b"null tokens")]
    for eb, sfx in ((4, "f32"), (8, "f64")):
        enc, dec = getattr(_lib.lib, f"tg_bilinear_encode_{sfx}"), getattr(_lib.lib, f"tg_bilinear_decode_{sfx}")
        aligned = f"not {eb}-byte aligned".encode()
        for over, words in both + [(dict(mode=2), b"mode=2"), (dict(X=None), b"null X"), (dict(Y=None), b"null Y"),
                                   (dict(X=p((1 << 16) + eb // 2)), b"X " + aligned),
                                   (dict(Y=p((1 << 20) + eb // 2)), b"Y " + aligned),
                                   (dict(Y=p((1 << 16) + 32 * eb - eb)), b"X and Y overlap"),    # X's last element
                                   (dict(X=p((1 << 20) + 56 * eb - eb)), b"X and Y overlap"),    # Y's last element
                                   (dict(Y=p((1 << 16) - 56 * eb + eb)), b"X and Y overlap"),
                                   (dict(tokens=p((1 << 20) + 8)), b"tokens and Y overlap"),
                                   (dict(tokens=p((1 << 20) - 7 * 12 + 1)), b"tokens and Y overlap")]:
            kw = {**ok_e, **over}
            assert enc(*[kw[k] for k in order_e], None) == -1 and words in _lib.lib.tg_last_error(), (sfx, over)
        for over, words in both + [(dict(M=None), b"null M"), (dict(C=None), b"null C"),
                                   (dict(M=p((1 << 20) + eb // 2)), b"M " + aligned),
                                   (dict(C=p((1 << 16) + eb // 2)), b"C " + aligned),
                                   (dict(C=p((1 << 20) + 56 * eb - eb)), b"M and C overlap"),
                                   (dict(M=p((1 << 16) + 32 * eb - eb)), b"M and C overlap"),
                                   (dict(tokens=p((1 << 16) + 8)), b"tokens and C overlap")]:
            kw = {**ok_d, **over}
            assert dec(*[kw[k] for k in order_d], None) == -1 and words in _lib.lib.tg_last_error(), (sfx, over)
        assert enc(None, 0, 4, 4, 4, 16, None, 7, 2, 0, 1, None, None) == 0      # batch = 0 returns at once
        assert dec(None, 0, 4, 4, 4, 16, None, 7, 2, 1, None, None) == 0
        assert enc(None, 0, 4, 4, 4, 16, None, 7, 6, 0, 1, None, None) == -1     # ... after the size checks


def test_bindings_refuse_cpu_tensors_and_wrong_layouts(golden):
    X = torch.zeros((2, 4, 4))
    tok = torch.from_numpy(golden("strassen")["tokens"])
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.bilinear_encode(X, tok, 7, 2, 0)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.bilinear_decode(torch.zeros((2, 7, 2, 2)), tok, 7, 2)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.BilinearMatmul(tok, 7, n=2)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.BilinearMatmul.__call__(object.__new__(mat_mul_amd.BilinearMatmul), X, X)


# ---- the restatement's own checks: the index convention, in exact arithmetic -------------------------------------------
def _integers(rng, *shape):
    return rng.integers(-9, 10, size=shape)


def _strassen(golden):
    return BR.coefficients(golden("strassen")["tokens"], 7, 1)


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_the_standard_list_multiplies_rectangular_blocks(n):
    f = BR.standard(n)
    assert np.array_equal(BR.term_sum(f, n), BR.matmul_tensor(n))
    rng = np.random.default_rng(n)
    A, B = _integers(rng, 2, 2 * n, 3 * n), _integers(rng, 2, 3 * n, 1 * n)
    assert np.array_equal(BR.multiply(f, n, A, B), A @ B)


def test_the_golden_strassen_list_multiplies(golden):
    f = _strassen(golden)
    assert f.shape == (7, 12) and np.array_equal(BR.term_sum(f, 2), BR.matmul_tensor(2))
    assert np.array_equal(golden("strassen")["tensor"], BR.matmul_tensor(2))
    rng = np.random.default_rng(0)
    A, B = _integers(rng, 3, 6, 2), _integers(rng, 3, 2, 10)
    assert np.array_equal(BR.multiply(f, 2, A, B), A @ B)


def test_the_kronecker_square_of_strassen_proves_and_multiplies(golden):
    f = _strassen(golden)
    k = BR.kron(f, 2, f, 2)
    assert k.shape == (49, 48) and set(np.unique(k)) == {-1, 0, 1}
    assert np.array_equal(BR.term_sum(k, 4), BR.matmul_tensor(4))
    rng = np.random.default_rng(1)
    A, B = _integers(rng, 2, 8, 4), _integers(rng, 2, 4, 12)
    want = A @ B
    assert np.array_equal(BR.multiply(k, 4, A, B), want)
    assert np.array_equal(BR.multiply(f, 2, A, B, levels=2), want)           # two levels of Strassen: the same matrix
    s3 = BR.standard(3)
    mixed = BR.kron(f, 2, s3, 3)                                             # and a product of different sizes
    assert np.array_equal(BR.term_sum(mixed, 6), BR.matmul_tensor(6))


def test_encode_and_decode_keep_the_stated_order_and_skip_zero_coefficients():
    # one term u = (1, 1, -1, 0): ((x0 + x1) - x2) in float32, in that order, and x3 = NaN does not enter
    f = np.zeros((1, 12), dtype=np.int64)
    f[0, :4] = (1, 1, -1, 0)
    X = np.zeros((1, 2, 2), dtype=np.float32)
    X[0] = [[1.0, 2.0 ** -24], [1.0, np.nan]]
    Y = BR.encode(f, 2, 0, X)
    assert Y.dtype == np.float32 and Y.shape == (1, 1, 1, 1) and Y[0, 0, 0, 0] == 0.0     # 1 + 2^-24 rounds to 1
    X[0] = [[2.0 ** -24, -1.0], [-1.0, np.nan]]
    assert BR.encode(f, 2, 0, X)[0, 0, 0, 0] == np.float32(2.0 ** -24)                    # (2^-24 - 1) + 1, not 0
    f[0, 8:] = (0, 3, 0, 0)
    C = BR.decode(f, 2, np.full((1, 1, 1, 1), 0.1, dtype=np.float32))
    assert np.array_equal(C[0], np.array([[0, np.float32(3) * np.float32(0.1)], [0, 0]], dtype=np.float32))
    assert not np.signbit(C).any()                                                         # untouched blocks are +0


def test_exact_bound_is_reached_and_bounds(golden):
    f = _strassen(golden)
    assert BR.exact_bound(f, 2, 1, 3, 5) == 5 * (3 * 2) * (3 * 2) * 4        # rows of |u|, |v| sum to 2, a column of |w| to 4
    assert BR.exact_bound(BR.standard(5), 5, 1, 3, 2) == 2 * 3 * 3 * 5
    rng = np.random.default_rng(2)
    for levels in (1, 2):
        A, B = _integers(rng, 1, 4, 8) % 4, _integers(rng, 1, 8, 4) % 4      # inputs in [0, 3]
        assert np.abs(BR.multiply(f, 2, A, B, levels)).max() <= BR.exact_bound(f, 2, levels, 3, 8 // 2 ** levels)
