"""CPU checks of the rectangular entries (include/tensor_game_rect.h): the header, the exported symbols, every refusal of
the host side of the library, and the restatement's own checks of the <n,m,p> convention in exact arithmetic -- the
schoolbook lists sum to the target and multiply integer matrices, which is what test_gpu_rect.py relies on; and
``SymmetryGroup.matmul_rect`` on host arrays: closed, of the stated orders, every element fixing the target."""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import SymmetryGroup, _lib, build, functional, ops

import bilinear_rect_ref as RR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_rect.h"
ENTRIES = ["tg_bilinear_rect_check", "tg_bilinear_rect_decode_f32", "tg_bilinear_rect_decode_f64",
           "tg_bilinear_rect_encode_f32", "tg_bilinear_rect_encode_f64", "tg_reset_matmul_rect_i8"]
SHAPES = [(2, 2, 3), (2, 3, 4), (3, 4, 5), (4, 4, 8), (5, 5, 6), (1, 3, 2)]


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_rect_header_is_plain_c_and_states_the_convention_and_the_rule():
    text = HDR.read_text()
    for words in ("a = i*m + j,   b = j*p + k,   c = i*p + k", "The accumulator starts at +0", "ascending e (encode)",
                  "ascending r (decode)", "A zero coefficient contributes nothing", "round(c * x)", "round(acc + t)",
                  "no fused multiply-add", "it gets +0", "must not overlap", "Denormal", "64-bit",
                  "P = 16 where gr*gc <= 25 and P = 8 where gr*gc > 25"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_rect_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ENTRIES == sorted(_lib.RECT_SIGNATURES)
    assert HDR in build.HEADERS and (build.CSRC / "tg_rect.hip") in build.SOURCES
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    for name in ("reset_matmul_rect", "bilinear_rect_check", "bilinear_rect_encode", "bilinear_rect_decode"):
        assert name in ops.__all__
    for name in ("RectBilinearMatmul", "standard_rect"):
        assert name in mat_mul_amd.__all__ and getattr(mat_mul_amd, name) is getattr(mat_mul_amd.bilinear, name)
    assert callable(functional.matmul_target) and callable(SymmetryGroup.matmul_rect)


# ---- tg_reset_matmul_rect_i8 -------------------------------------------------------------------------------------------
RESET_OK = dict(state_out=C.c_void_p(1 << 16), B=2, n=2, m=3, p=4, S=12, game_stride_bytes=1728)
RESET_ORDER = ("state_out", "B", "n", "m", "p", "S", "game_stride_bytes")
RESET_REFUSALS = [(dict(n=0), b"n=0"), (dict(m=0), b"m=0"), (dict(p=-1), b"p=-1"), (dict(S=0), b"S=0"), (dict(S=33), b"S=33"),
                  (dict(n=5, S=14), b"n*m=15 above S=14"), (dict(S=11), b"m*p=12 above S=11"),
                  (dict(n=4, m=1, p=4, S=15), b"n*p=16 above S=15"), (dict(n=2 ** 16, m=2 ** 16), b"n*m="),
                  (dict(B=-1), b"B=-1"), (dict(game_stride_bytes=1727), b"game_stride_bytes=1727"),
                  (dict(B=2 ** 62), b"B="), (dict(state_out=None), b"null state_out")]


@pytest.mark.parametrize("over, words", RESET_REFUSALS)
def test_reset_matmul_rect_refuses_each_limit_by_name(over, words):
    kw = {**RESET_OK, **over}
    assert _lib.lib.tg_reset_matmul_rect_i8(*[kw[k] for k in RESET_ORDER], None) == -1, over
    err = _lib.lib.tg_last_error()
    assert err.startswith(b"tg_reset_matmul_rect_i8: ") and words in err, err


def test_reset_matmul_rect_takes_an_empty_batch_after_the_size_checks():
    lib = _lib.lib
    assert lib.tg_reset_matmul_rect_i8(None, 0, 2, 3, 4, 12, 1728, None) == 0
    assert lib.tg_reset_matmul_rect_i8(None, 0, 5, 5, 6, 30, 27000, None) == 0
    assert lib.tg_reset_matmul_rect_i8(None, 0, 1, 1, 1, 1, 1, None) == 0
    assert lib.tg_reset_matmul_rect_i8(None, 0, 2, 3, 4, 11, 1728, None) == -1


# ---- tg_bilinear_rect_check and the entries ----------------------------------------------------------------------------
OK_SIZES = dict(batch=2, rows=4, cols=6, ld=8, batch_stride=32, R=7, S=7, gr=2, gc=3, part=0, shift=1, elem_bytes=4)
REFUSALS = [(dict(S=0), "S=0"), (dict(S=33), "S=33"), (dict(gr=0), "gr=0"), (dict(gc=0), "gc=0"), (dict(gr=-2), "gr=-2"),
            (dict(S=5), "gr*gc=6 above S=5"), (dict(gr=4, gc=9, rows=4, cols=9, ld=9, S=32), "gr*gc=36 above S=32"),
            (dict(gr=2 ** 16, gc=2 ** 16), "above S=7"),
            (dict(R=0), "R=0"), (dict(R=257), "R=257"), (dict(shift=-1), "shift=-1"), (dict(shift=65), "shift=65"),
            (dict(part=3), "part=3"), (dict(part=-1), "part=-1"), (dict(batch=-1), "batch=-1"),
            (dict(rows=0), "rows=0"), (dict(rows=5), "rows=5 is no positive multiple of gr=2"), (dict(cols=0), "cols=0"),
            (dict(cols=7, ld=7), "cols=7 is no positive multiple of gc=3"), (dict(ld=5), "ld=5"),
            (dict(batch_stride=31), "batch_stride=31"), (dict(elem_bytes=2), "elem_bytes=2"),
            (dict(elem_bytes=16), "elem_bytes=16"), (dict(batch=2 ** 61), "byte offset"),
            (dict(rows=2 ** 40, ld=2 ** 40, batch=1), "byte offset")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_bilinear_rect_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.bilinear_rect_check(**{**OK_SIZES, **over})


def test_bilinear_rect_check_takes_the_limits():
    ops.bilinear_rect_check(**OK_SIZES)
    ops.bilinear_rect_check(0, 32, 1, 1, 0, R=256, S=32, gr=32, gc=1, part=2, shift=64, elem_bytes=8)
    ops.bilinear_rect_check(1, 1, 1, 1, 0, R=1, S=1, gr=1, gc=1, part=0, shift=0)     # batch_stride counts from batch 2 on
    ops.bilinear_rect_check(1 << 40, 4, 8, R=256, S=32, gr=4, gc=8)                   # a recursive call's batch
    ops.bilinear_rect_check(3, 10, 18, S=30, gr=5, gc=6, part=1)                      # ld, batch_stride default to dense
    ops.bilinear_rect_check(3, 1, 7, S=9, gr=1, gc=7)


def test_rect_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    order_e = ("X", "batch", "rows", "cols", "ld", "batch_stride", "tokens", "R", "S", "gr", "gc", "part", "shift", "Y")
    order_d = ("M", "batch", "rows", "cols", "ld", "batch_stride", "tokens", "R", "S", "gr", "gc", "shift", "C")
    sizes = dict(batch=2, rows=4, cols=6, ld=6, batch_stride=24, R=7, S=7, gr=2, gc=3, shift=1)
    # X spans ((2-1)*24 + 3*6 + 6) = 48 elements; Y 2*7*2*2 = 56; the list 7 * 21 = 147 bytes
    ok_e = dict(X=p(1 << 16), tokens=p(1 << 12), Y=p(1 << 20), part=0, **sizes)
    ok_d = dict(M=p(1 << 20), tokens=p(1 << 12), C=p(1 << 16), **sizes)
    both = [(dict(S=33), b"S=33"), (dict(gr=0), b"gr=0"), (dict(gc=0), b"gc=0"), (dict(S=5), b"gr*gc=6 above S=5"),
            (dict(R=257), b"R=257"), (dict(shift=65), b"shift=65"), (dict(rows=5), b"rows=5"), (dict(cols=4, ld=6), b"cols=4"),
            (dict(ld=5), b"ld=5"), (dict(batch_stride=23), b"batch_stride=23"), (dict(batch=-1), b"batch=-1"),
            (dict(tokens=None), b"null tokens")]
    for eb, sfx in ((4, "f32"), (8, "f64")):
        enc = getattr(_lib.lib, f"tg_bilinear_rect_encode_{sfx}")
        dec = getattr(_lib.lib, f"tg_bilinear_rect_decode_{sfx}")
        aligned = f"not {eb}-byte aligned".encode()
        for over, words in both + [(dict(part=2), b"part=2"), (dict(part=-1), b"part=-1"), (dict(X=None), b"null X"),
                                   (dict(Y=None), b"null Y"),
                                   (dict(X=p((1 << 16) + eb // 2)), b"X " + aligned),
                                   (dict(Y=p((1 << 20) + eb // 2)), b"Y " + aligned),
                                   (dict(Y=p((1 << 16) + 48 * eb - eb)), b"X and Y overlap"),    # X's last element
                                   (dict(X=p((1 << 20) + 56 * eb - eb)), b"X and Y overlap"),    # Y's last element
                                   (dict(Y=p((1 << 16) - 56 * eb + eb)), b"X and Y overlap"),
                                   (dict(tokens=p((1 << 20) + 8)), b"tokens and Y overlap"),
                                   (dict(tokens=p((1 << 20) - 147 + 1)), b"tokens and Y overlap")]:
            kw = {**ok_e, **over}
            assert enc(*[kw[k] for k in order_e], None) == -1 and words in _lib.lib.tg_last_error(), (sfx, over)
        for over, words in both + [(dict(M=None), b"null M"), (dict(C=None), b"null C"),
                                   (dict(M=p((1 << 20) + eb // 2)), b"M " + aligned),
                                   (dict(C=p((1 << 16) + eb // 2)), b"C " + aligned),
                                   (dict(C=p((1 << 20) + 56 * eb - eb)), b"M and C overlap"),
                                   (dict(M=p((1 << 16) + 48 * eb - eb)), b"M and C overlap"),
                                   (dict(tokens=p((1 << 16) + 8)), b"tokens and C overlap")]:
            kw = {**ok_d, **over}
            assert dec(*[kw[k] for k in order_d], None) == -1 and words in _lib.lib.tg_last_error(), (sfx, over)
        assert enc(None, 0, 4, 6, 6, 24, None, 7, 7, 2, 3, 0, 1, None, None) == 0     # batch = 0 returns at once
        assert dec(None, 0, 4, 6, 6, 24, None, 7, 7, 2, 3, 1, None, None) == 0
        assert enc(None, 0, 4, 6, 6, 24, None, 7, 5, 2, 3, 0, 1, None, None) == -1    # ... after the size checks


def test_rect_bindings_refuse_cpu_tensors():
    X = torch.zeros((2, 4, 6))
    tok = mat_mul_amd.standard_rect(2, 2, 3)
    assert tok.dtype == torch.int8 and tuple(tok.shape) == (12, 18) and not tok.is_cuda
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.reset_matmul_rect(torch.zeros((1, 6, 6, 6), dtype=torch.int8), 2, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        functional.matmul_target(1, 2, 2, 3, device="cpu")
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.bilinear_rect_encode(X, tok, 12, 2, 3, 1)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.bilinear_rect_decode(torch.zeros((2, 12, 2, 2)), tok, 12, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.RectBilinearMatmul(tok, 12, 2, 2, 3)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.RectBilinearMatmul.__call__(object.__new__(mat_mul_amd.RectBilinearMatmul), X, X)
    with pytest.raises(_lib.TensorGameError, match=r"S=5 outside \[max"):
        mat_mul_amd.standard_rect(2, 2, 3, S=5)
    with pytest.raises(_lib.TensorGameError, match="S=36"):
        functional.matmul_target(1, 6, 6, 6, device="cpu")
    with pytest.raises(_lib.TensorGameError, match="only square shapes"):             # untouched
        functional.build_matmul_tensor(1, 2, 2, 3, device="cpu")


# ---- the restatement's own checks: the convention, in exact arithmetic -------------------------------------------------
def _integers(rng, *shape):
    return rng.integers(-9, 10, size=shape)


@pytest.mark.parametrize("n, m, p", SHAPES)
def test_standard_rect_sums_to_the_target_and_the_package_list_is_the_same(n, m, p):
    need = RR.cube_size(n, m, p)
    for S in sorted({need, min(need + 1, 32), 32}):
        f = RR.standard_rect(n, m, p, S)
        T = RR.matmul_target(n, m, p, S)
        assert f.shape == (n * m * p, 3 * S) and T.sum() == n * m * p
        assert np.array_equal(RR.term_sum(f), T)
        assert not T[n * m:].any() and not T[:, m * p:].any() and not T[:, :, n * p:].any()   # the padding is zero
        for shift in (1, 2):
            tok = mat_mul_amd.standard_rect(n, m, p, S, shift=shift)
            assert np.array_equal(tok.numpy().astype(np.int64) - shift, f)
    assert np.array_equal(mat_mul_amd.standard_rect(n, m, p).numpy() - 1, RR.standard_rect(n, m, p))   # the default S
    if n == m == p:
        import bilinear_ref as BR
        assert np.array_equal(RR.matmul_target(n, n, n), BR.matmul_tensor(n))


def test_the_square_case_is_the_square_convention():
    import bilinear_ref as BR
    for n in (2, 3, 4, 5):
        assert np.array_equal(RR.matmul_target(n, n, n), BR.matmul_tensor(n))
        assert np.array_equal(RR.standard_rect(n, n, n), BR.standard(n))
        rng = np.random.default_rng(n)
        f = rng.integers(-2, 3, size=(5, 3 * n * n))
        X = _integers(rng, 2, 2 * n, 3 * n)
        assert np.array_equal(RR.encode(f, n, n, 1, X), BR.encode(f, n, 1, X))
        M = _integers(rng, 2, 5, 2, 3)
        assert np.array_equal(RR.decode(f, n, n, M), BR.decode(f, n, M))


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("n, m, p", SHAPES)
def test_standard_rect_multiplies_integer_matrices_exactly(n, m, p, levels):
    rng = np.random.default_rng(100 * n + 10 * m + p)
    need = RR.cube_size(n, m, p)
    for S in sorted({need, min(need + 2, 32)}):
        f = RR.standard_rect(n, m, p, S)
        f[:, n * m:S] = 7                                       # what the padding entries hold does not matter
        f[:, S + m * p:2 * S] = -5
        f[:, 2 * S + n * p:] = 3
        P, Q, T = 2 * n ** levels, m ** levels, 3 * p ** levels
        A, B = _integers(rng, 2, P, Q), _integers(rng, 2, Q, T)
        assert np.array_equal(RR.multiply(f, n, m, p, A, B, levels), A @ B)


def test_rect_encode_and_decode_keep_the_stated_order_and_skip_zero_coefficients():
    # one term on the grid 1 x 4, u = (1, 1, -1, 0): ((x0 + x1) - x2) in float32, in that order; x3 = NaN does not enter
    S = 5
    f = np.zeros((1, 3 * S), dtype=np.int64)
    f[0, :5] = (1, 1, -1, 0, 9)                                 # entry 4 is beyond the grid
    X = np.array([[[1.0, 2.0 ** -24, 1.0, np.nan]]], dtype=np.float32)
    Y = RR.encode(f, 1, 4, 0, X)
    assert Y.dtype == np.float32 and Y.shape == (1, 1, 1, 1) and Y[0, 0, 0, 0] == 0.0      # 1 + 2^-24 rounds to 1
    X[0, 0] = [2.0 ** -24, -1.0, -1.0, np.nan]
    assert RR.encode(f, 1, 4, 0, X)[0, 0, 0, 0] == np.float32(2.0 ** -24)                  # (2^-24 - 1) + 1, not 0
    f[0, 2 * S:] = (0, 3, 0, 0, 9)
    Cm = RR.decode(f, 2, 2, np.full((1, 1, 1, 1), 0.1, dtype=np.float32))
    assert np.array_equal(Cm[0], np.array([[0, np.float32(3) * np.float32(0.1)], [0, 0]], dtype=np.float32))
    assert not np.signbit(Cm).any()                                                         # untouched blocks are +0


# ---- SymmetryGroup.matmul_rect, on host arrays -------------------------------------------------------------------------
def _stabiliser_of_the_triple(n, m, p):
    """How many permutations of (n, m, p) leave the triple unchanged."""
    import itertools
    return sum(1 for q in itertools.permutations((n, m, p)) if q == (n, m, p))


ORDERS = [((3, 3, 3), 1296), ((2, 2, 3), 48), ((2, 3, 1), 12), ((2, 3, 2), 48), ((1, 3, 2), 12), ((2, 3, 4), 288)]


@pytest.mark.parametrize("dims, order", ORDERS)
def test_matmul_rect_is_a_group_of_the_stated_order_that_fixes_the_target(dims, order):
    n, m, p = dims
    assert order == math.factorial(n) * math.factorial(m) * math.factorial(p) * _stabiliser_of_the_triple(n, m, p)
    need = RR.cube_size(n, m, p)
    for S in (None, need + 1):
        grp = SymmetryGroup.matmul_rect(n, m, p, S=S, signs=False)
        S = need if S is None else S
        assert grp.S == S and grp.order == order and grp.closed() and grp.device is None
        assert len({bytes(r) for r in grp.rows}) == order
        f, T = RR.standard_rect(n, m, p, S), RR.matmul_target(n, m, p, S)
        pad = np.concatenate([np.arange(d * S + size, (d + 1) * S) for d, size in enumerate((n * m, m * p, n * p))])
        for row in grp.rows:                                     # every element maps the target to itself
            assert np.array_equal(RR.term_sum(RR.apply_symmetry(row, f)), T)
            assert np.array_equal(row[1:][pad], pad % S)         # the padding maps to itself, sign +1


def test_matmul_rect_with_signs():
    grp = SymmetryGroup.matmul_rect(2, 3, 1)                     # 12 * 2^(2+3+1) / 2: (a, b, c) = -(1, 1, 1) acts as +1
    assert grp.order == 384 and grp.closed()
    f, T = RR.standard_rect(2, 3, 1), RR.matmul_target(2, 3, 1)
    assert (grp.rows[:, 1:] & 0x80).any()
    for row in grp.rows:
        assert np.array_equal(RR.term_sum(RR.apply_symmetry(row, f)), T)
    # <2,2,3> with signs: 48 * 2^7 / 2 = 3 072 elements, above TG_ORBIT_MAX_G = 2 048: generate refuses the closure
    assert 48 * 2 ** 7 // 2 == 3072 > _lib.TG_ORBIT_MAX_G
    with pytest.raises(_lib.TensorGameError, match=rf"more than max_order={_lib.TG_ORBIT_MAX_G}"):
        SymmetryGroup.matmul_rect(2, 2, 3)


def test_matmul_rect_at_333_is_matmul_3_as_a_set_of_rows():
    rect = SymmetryGroup.matmul_rect(3, 3, 3, signs=False)
    square = SymmetryGroup.matmul(3, signs=False)
    assert rect.order == square.order == 1296
    assert {bytes(r) for r in rect.rows} == {bytes(r) for r in square.rows}


def test_matmul_rect_refuses_bad_sizes():
    with pytest.raises(_lib.TensorGameError, match="at least 1"):
        SymmetryGroup.matmul_rect(0, 2, 3)
    with pytest.raises(_lib.TensorGameError, match=r"S=5 outside \[max"):
        SymmetryGroup.matmul_rect(2, 2, 3, S=5)
    with pytest.raises(_lib.TensorGameError, match="S=36"):
        SymmetryGroup.matmul_rect(6, 6, 6)
