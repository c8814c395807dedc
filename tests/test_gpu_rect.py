"""GPU checks of the rectangular entries (include/tensor_game_rect.h): ``ops.reset_matmul_rect`` against the restatement
(bilinear_rect_ref.py) in canary-guarded games; ``ops.bilinear_rect_encode`` and ``ops.bilinear_rect_decode`` bit for bit
against it on strided, misaligned, canary-guarded buffers, for grids in every bucket of the block count and on both of
its edges, lists of a cube size at and above the grid with rubbish in the entries that are not read, both pack widths;
bit for bit against the square entries on the grid n x n; ``RectBilinearMatmul`` exactly equal to the integer product;
and <2,2,3> end to end: archive modulo its symmetry group, walks over Z_2, sign lift, and the rank-11 list run as a
matrix multiplication."""
import numpy as np
import pytest
import torch

from mat_mul_amd import (RectBilinearMatmul, SolutionArchive, SymmetryGroup, TensorGameError, functional, ops,
                         reduce_archive_lifted, standard_rect)

import bilinear_rect_ref as RR
from guarded_buffers import check_flat, check_states, guarded, guarded_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 777.0  # what every element of a buffer holds that no launch may write
DTYPES = {"f32": (np.float32, torch.float32, np.uint32), "f64": (np.float64, torch.float64, np.uint64)}


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def bits(x, dt):
    return np.ascontiguousarray(x).view(DTYPES[dt][2])


# ---- reset ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m, p, S", [(2, 2, 3, 6), (2, 3, 4, 12), (2, 3, 4, 13), (5, 5, 6, 30), (4, 4, 8, 32), (1, 3, 2, 6)])
def test_reset_matmul_rect_equals_the_restatement(n, m, p, S):
    want = RR.matmul_target(n, m, p, S).astype(np.int8)
    for B, stride in ((1, S ** 3), (3, S ** 3 + 11), (3, (S ** 3 + 15) // 16 * 16)):
        buf, view = guarded_states(B, S, stride)
        assert ops.reset_matmul_rect(view, n, m, p) is view
        torch.cuda.synchronize()
        check_states(buf, B, S, stride, (n, m, p, S, B, stride))
        assert np.array_equal(view.cpu().numpy(), np.repeat(want[None], B, 0))
    T = functional.matmul_target(3, n, m, p, S, device=DEV)
    assert T.dtype == torch.int8 and tuple(T.shape) == (3, S, S, S) and not bool(T[1:].any())
    assert np.array_equal(T[0].cpu().numpy(), want)
    if S == RR.cube_size(n, m, p):
        assert torch.equal(functional.matmul_target(1, n, m, p, device=DEV), T[:1])      # the default S


def test_reset_matmul_rect_at_222_equals_reset_matmul_bit_for_bit():
    for n in (2, 3, 5):
        S = n * n
        a, b = ops.alloc_states(3, S, DEV), ops.alloc_states(3, S, DEV)
        ops.reset_matmul(a, n)
        ops.reset_matmul_rect(b, n, n, n)
        assert torch.equal(a, b)
        assert torch.equal(functional.build_matmul_tensor(2, n, n, n, device=DEV),
                           functional.matmul_target(2, n, n, n, device=DEV))
    with pytest.raises(TensorGameError, match=r"m\*p=12 above S=11"):
        ops.reset_matmul_rect(torch.zeros((1, 11, 11, 11), dtype=torch.int8, device=DEV), 2, 3, 4)


# ---- encode and decode ---------------------------------------------------------------------------------------------------
def odd_tokens(f, shift, extra=2):
    """The list as device tokens at an odd address, with ``extra`` rows of rubbish behind the R that are used."""
    tok = np.full((len(f) + extra, f.shape[1]), 99, dtype=np.int8)
    tok[:len(f)] = f + shift
    flat = torch.zeros(tok.size + 1, dtype=torch.int8, device=DEV)
    flat[1:] = dev(tok.reshape(-1))
    return flat[1:].view(tok.shape)


class Strided:
    """A canary-guarded flat buffer full of FILL and a (batch,rows,cols) view of it with row stride ``ld``, batch stride
    ``bs``, starting ``off`` elements in (the guarded tensor itself starts on a 16-byte boundary)."""

    def __init__(self, batch, rows, cols, ld, bs, off, dt):
        self.dt, self.geom = dt, (batch, rows, cols, ld, bs, off)
        self.span = off + (batch - 1) * bs + (rows - 1) * ld + cols + 3
        self.buf, self.flat = guarded((self.span,), DTYPES[dt][1])
        assert self.flat.data_ptr() % 16 == 0
        self.flat.fill_(FILL)
        self.view = self.flat.as_strided((batch, rows, cols), (bs, ld, 1), self.flat.storage_offset() + off)
        assert self.view.data_ptr() == self.flat.data_ptr() + off * self.flat.element_size()

    def expect(self, want):
        """The whole flat buffer bit for bit: ``want`` in the view, FILL everywhere else; and the canaries."""
        batch, rows, cols, ld, bs, off = self.geom
        flat = np.full(self.span, FILL, dtype=DTYPES[self.dt][0])
        item = flat.itemsize
        np.lib.stride_tricks.as_strided(flat[off:], (batch, rows, cols), (bs * item, ld * item, item))[...] = want
        torch.cuda.synchronize()
        check_flat(self.buf, self.geom)
        got = self.flat.cpu().numpy()
        assert np.array_equal(bits(got, self.dt), bits(flat, self.dt)), self.geom


def dense(shape, off, dt):
    """A Strided whose view is contiguous: (batch, rows, cols) = (shape[0], prod(shape[1:-1]), shape[-1])."""
    rows = int(np.prod(shape[1:-1]))
    return Strided(shape[0], rows, shape[-1], shape[-1], rows * shape[-1], off, dt)


# (h, w, batch, ld - cols, batch_stride - rows*ld, offset of the strided operand, offset of the dense one), elements.
# Packs are 16 bytes up to 25 blocks and 8 bytes above (float32: 4 or 2 elements, float64: 2 or 1): a path needs w, ld,
# batch_stride and both offsets to allow it.
LAYOUTS = [
    (1, 1, 1, 0, 0, 0, 0),      # the smallest call: h = w = 1; single elements
    (3, 5, 3, 3, 5, 0, 0),      # odd h and w, ld > cols, a batch stride larger than needed; single elements
    (3, 4, 3, 0, 0, 0, 0),      # dense and aligned: packs, a partial wavefront
    (2, 5, 1, 0, 0, 1, 1),      # both base pointers one element off
    (3, 8, 3, 4, 8, 0, 0),      # packs with ld > cols and a larger batch stride
    (1, 68, 3, 0, 0, 0, 0),     # packs: 17 or 34 per row
    (3, 68, 2, 0, 0, 1, 0),     # the strided base alone is off: single elements, 408 items = a workgroup and a tail
    (2, 6, 3, 2, 2, 2, 2),      # everything a multiple of 8 bytes only (float32): packs of 8 bytes above 25 blocks alone
    (2, 8, 1, 0, 0, 0, 1),      # the dense base alone is off
    (2, 8, 3, 1, 0, 0, 0),      # ld alone forbids packs
    (2, 4, 3, 0, 1, 0, 0),      # the batch stride alone forbids packs
]
# every bucket of the block count (<= 4, 9, 16, 25, 32) and both edges of each: 1, 6 | 6, 7 | 20 | 30, 32
GRIDS = [(1, 1), (2, 3), (3, 2), (1, 7), (4, 5), (5, 6), (4, 8), (32, 1)]


def random_list(rng, R, S, live, zero_row, zero_col):
    """Random coefficients in [-3, 3] (no factorisation of anything), about a quarter of them zero; an all-zero term and
    an all-zero column (index 1 of every part, or 0 on a grid of one block) where asked; and rubbish in [-9, 9] without
    zeros in the entries at and beyond ``live``, which no entry may read."""
    f = rng.integers(-3, 4, size=(R, 3, S))
    f[rng.random(f.shape) < 0.25] = 0
    if zero_row and R > 1:
        f[R // 2] = 0
    if zero_col:
        f[:, :, min(1, live - 1)] = 0
    junk = rng.integers(1, 10, size=(R, 3, S)) * rng.choice([-1, 1], size=(R, 3, S))
    f[:, :, live:] = junk[:, :, live:]
    return f.reshape(R, 3 * S)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("R", [1, 7, 60, 256])
@pytest.mark.parametrize("gr, gc", GRIDS)
def test_rect_encode_and_decode_equal_the_restatement_bit_for_bit(gr, gc, R, dt):
    rng = np.random.default_rng(10000 * gr + 100 * gc + R)
    npdt = DTYPES[dt][0]
    live = gr * gc
    for i, (h, w, batch, dld, dbs, off, doff) in enumerate(LAYOUTS):
        shift = 1 + i % 2
        S = live if i % 2 == 0 else min(32, live + 1 + i % 3)                       # at and above the grid
        f = random_list(rng, R, S, live, zero_row=i % 3 == 0, zero_col=i % 3 == 1)
        tok = odd_tokens(f, shift)
        rows, cols = gr * h, gc * w
        ld = cols + dld
        bs = rows * ld + dbs
        # encode: strided X -> dense Y, parts 0 and 1
        part = i % 2
        X = Strided(batch, rows, cols, ld, bs, off, dt)
        Xn = rng.standard_normal((batch, rows, cols)).astype(npdt)
        X.view.copy_(dev(Xn))
        Y = dense((batch, R, h, w), doff, dt)
        got = ops.bilinear_rect_encode(X.view, tok, R, gr, gc, part, shift, out=Y.view.view(batch, R, h, w))
        assert got.data_ptr() == Y.view.data_ptr()
        Y.expect(RR.encode(f, gr, gc, part, Xn).reshape(batch, R * h, w))
        X.expect(Xn)                                                                   # the input is as it was
        # decode: dense M -> strided C, part 2
        Mn = rng.standard_normal((batch, R, h, w)).astype(npdt)
        M = dense((batch, R, h, w), doff, dt)
        M.view.copy_(dev(Mn.reshape(batch, R * h, w)))
        Cs = Strided(batch, rows, cols, ld, bs, off, dt)
        ops.bilinear_rect_decode(M.view.view(batch, R, h, w), tok, R, gr, gc, shift, out=Cs.view)
        Cs.expect(RR.decode(f, gr, gc, Mn))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_entries_beyond_the_grid_do_not_change_a_bit(dt):
    rng = np.random.default_rng(3)
    npdt = DTYPES[dt][0]
    gr, gc, R, S, h, w = 2, 3, 7, 9, 2, 4
    f = random_list(rng, R, S, gr * gc, False, False)
    g = f.copy().reshape(R, 3, S)
    g[:, :, gr * gc:] = 0                                              # the same list with a clean padding
    g = g.reshape(R, 3 * S)
    assert not np.array_equal(f, g)
    Xn = rng.standard_normal((2, gr * h, gc * w)).astype(npdt)
    Mn = rng.standard_normal((2, R, h, w)).astype(npdt)
    for part in (0, 1):
        a = ops.bilinear_rect_encode(dev(Xn), dev(f + 1).to(torch.int8), R, gr, gc, part)
        b = ops.bilinear_rect_encode(dev(Xn), dev(g + 1).to(torch.int8), R, gr, gc, part)
        assert np.array_equal(bits(a.cpu().numpy(), dt), bits(b.cpu().numpy(), dt))
    a = ops.bilinear_rect_decode(dev(Mn), dev(f + 1).to(torch.int8), R, gr, gc)
    b = ops.bilinear_rect_decode(dev(Mn), dev(g + 1).to(torch.int8), R, gr, gc)
    assert np.array_equal(bits(a.cpu().numpy(), dt), bits(b.cpu().numpy(), dt))
    assert np.array_equal(bits(a.cpu().numpy(), dt), bits(RR.decode(f, gr, gc, Mn), dt))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_the_grid_n_by_n_equals_the_square_entries_bit_for_bit(n, dt):
    rng = np.random.default_rng(n)
    npdt, S, R = DTYPES[dt][0], n * n, 23
    f = rng.integers(-3, 4, size=(R, 3 * S))
    tok = dev(f + 2).to(torch.int8)
    for h, w, off in ((3, 8, 0), (3, 5, 0), (2, 8, 1)):               # packs; single elements; a misaligned base
        flat = dev(rng.standard_normal(off + 3 * n * h * n * w).astype(npdt))
        X = flat[off:].view(3, n * h, n * w)
        for mode in (0, 1):
            sq = ops.bilinear_encode(X, tok, R, n, mode, 2)
            re = ops.bilinear_rect_encode(X, tok, R, n, n, mode, 2)
            assert np.array_equal(bits(sq.cpu().numpy(), dt), bits(re.cpu().numpy(), dt))
        M = dev(rng.standard_normal((3, R, h, w)).astype(npdt))
        sq, re = ops.bilinear_decode(M, tok, R, n, 2), ops.bilinear_rect_decode(M, tok, R, n, n, 2)
        assert np.array_equal(bits(sq.cpu().numpy(), dt), bits(re.cpu().numpy(), dt))


def test_rect_outputs_allocated_by_the_bindings_and_views_of_larger_tensors():
    rng = np.random.default_rng(5)
    gr, gc, R, S = 2, 3, 7, 8
    f = random_list(rng, R, S, gr * gc, False, False)
    tok = dev(f + 2).to(torch.int8)
    big = rng.standard_normal((4, 9, 24)).astype(np.float32)
    view = dev(big)[1:3, 3:9, 4:16]                                   # (2,6,12) inside (4,9,24): not copied
    Y = ops.bilinear_rect_encode(view, tok, R, gr, gc, 1, 2)
    assert Y.is_contiguous() and tuple(Y.shape) == (2, R, 3, 4)
    assert np.array_equal(bits(Y.cpu().numpy(), "f32"), bits(RR.encode(f, gr, gc, 1, big[1:3, 3:9, 4:16]), "f32"))
    C = ops.bilinear_rect_decode(Y, tok, R, gr, gc, 2)
    assert tuple(C.shape) == (2, 6, 12)
    assert np.array_equal(bits(C.cpu().numpy(), "f32"), bits(RR.decode(f, gr, gc, Y.cpu().numpy()), "f32"))
    with pytest.raises(TensorGameError, match="column stride"):
        ops.bilinear_rect_encode(dev(big).transpose(1, 2)[:, :12, :6], tok, R, gr, gc, 0, 2)
    with pytest.raises(TensorGameError, match="float32 or float64"):
        ops.bilinear_rect_encode(dev(big).to(torch.float16), tok, R, gr, gc, 0, 2)
    with pytest.raises(TensorGameError, match="R=9 above"):
        ops.bilinear_rect_encode(view, tok, 9, gr, gc, 0, 2)
    with pytest.raises(TensorGameError, match=r"gr\*gc=9 above S=8"):
        ops.bilinear_rect_encode(dev(big), tok, R, 3, 3, 0, 2)
    with pytest.raises(TensorGameError, match="part=2"):
        ops.bilinear_rect_encode(view, tok, R, gr, gc, 2, 2)
    with pytest.raises(TensorGameError, match="overlap"):
        flat = torch.zeros(320, dtype=torch.float32, device=DEV)
        ops.bilinear_rect_decode(flat[:168].view(2, 7, 3, 4), tok, R, gr, gc, 2, out=flat[8:152].view(2, 6, 12))


def test_a_rect_batch_of_70000_is_not_capped_by_a_grid_dimension():
    rng = np.random.default_rng(6)
    gr, gc, R = 2, 3, 7
    f = random_list(rng, R, 6, 6, False, False)
    tok = dev(f + 1).to(torch.int8)
    Xn = rng.standard_normal((70000, gr, gc)).astype(np.float32)      # the smallest block: h = w = 1
    Y = ops.bilinear_rect_encode(dev(Xn), tok, R, gr, gc, 0)
    want = RR.encode(f, gr, gc, 0, Xn)
    assert tuple(Y.shape) == (70000, R, 1, 1) and np.array_equal(bits(Y.cpu().numpy(), "f32"), bits(want, "f32"))
    C = ops.bilinear_rect_decode(Y, tok, R, gr, gc)
    assert np.array_equal(bits(C.cpu().numpy(), "f32"), bits(RR.decode(f, gr, gc, want), "f32"))


@pytest.mark.parametrize("w", [240004, 60001])                        # packs of 16 bytes; single elements
def test_more_rect_items_than_the_grid_holds_at_once(w):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    batch, h, gr, gc, R = 3, 3, 1, 2, 2
    items = batch * h * (w // 4 if w % 4 == 0 else w)
    assert items > 8 * cus * 256                                      # the launch starts at most 8 workgroups per CU
    rng = np.random.default_rng(w)
    f = random_list(rng, R, 3, 2, False, False)
    tok = dev(f + 1).to(torch.int8)
    Xn = rng.standard_normal((batch, gr * h, gc * w)).astype(np.float32)
    Y = ops.bilinear_rect_encode(dev(Xn), tok, R, gr, gc, 1)
    want = RR.encode(f, gr, gc, 1, Xn)
    assert np.array_equal(bits(Y.cpu().numpy(), "f32"), bits(want, "f32"))
    C = ops.bilinear_rect_decode(Y, tok, R, gr, gc)
    assert np.array_equal(bits(C.cpu().numpy(), "f32"), bits(RR.decode(f, gr, gc, want), "f32"))


@pytest.mark.parametrize("dt, w", [("f32", 4), ("f32", 3), ("f64", 2), ("f64", 5)])
@pytest.mark.parametrize("gr, gc", [(2, 3), (5, 6)])
def test_rect_zero_coefficients_do_not_spread_non_finite_values_and_give_plus_zero(gr, gc, dt, w):
    rng = np.random.default_rng(7)
    npdt = DTYPES[dt][0]
    S, R, h, batch = gr * gc + 1, 7, 2, 2
    f = random_list(rng, R, S, gr * gc, False, False)
    f[:3, 2] = 0                                                      # terms 0..2 do not use block 2 of X
    f[3:, 2] = (1, -2, 3, -1)
    f[:2, 2 * S + 1] = 0                                              # block 1 of C does not use products 0 and 1
    f[2:, 2 * S + 1] = (2, 1, -1, 3, -3)
    f[:, 2 * S + 4] = 0                                               # block 4 of C uses no product at all: +0
    f[5, :S] = 0                                                      # and Y[:, 5] no block
    tok = dev(f + 1).to(torch.int8)
    Xn = rng.standard_normal((batch, gr * h, gc * w)).astype(npdt)
    r2, c2 = (2 // gc) * h, (2 % gc) * w
    Xn[:, r2:r2 + h, c2:c2 + w] = np.nan                              # block 2
    Xn[0, r2, c2] = np.inf
    got = ops.bilinear_rect_encode(dev(Xn), tok, R, gr, gc, 0).cpu().numpy()
    want = RR.encode(f, gr, gc, 0, Xn)
    assert np.isfinite(got[:, :3]).all() and not np.isfinite(got[:, [3, 4, 6]]).any()
    assert np.array_equal(bits(got[:, :3], dt), bits(want[:, :3], dt)) and np.array_equal(got, want, equal_nan=True)
    assert not bits(got[:, 5], dt).any()                              # +0, every bit
    Mn = rng.standard_normal((batch, R, h, w)).astype(npdt)
    Mn[:, :2] = np.nan
    Mn[1, 0, 0, 0] = -np.inf
    got = ops.bilinear_rect_decode(dev(Mn), tok, R, gr, gc).cpu().numpy()
    want = RR.decode(f, gr, gc, Mn)
    blk = lambda e: (slice(None), slice((e // gc) * h, (e // gc + 1) * h), slice((e % gc) * w, (e % gc + 1) * w))
    assert np.isfinite(got[blk(1)]).all() and np.array_equal(bits(got[blk(1)], dt), bits(want[blk(1)], dt))
    assert not bits(got[blk(4)], dt).any()                            # the NaN products behind zero coefficients: +0
    assert np.array_equal(got, want, equal_nan=True)


# ---- RectBilinearMatmul --------------------------------------------------------------------------------------------------
def algorithm(f, n, m, p, levels, shift=1):
    return RectBilinearMatmul(dev(f + shift).to(torch.int8), len(f), n, m, p, shift=shift, levels=levels)


def small_integers(rng, *shape):
    return rng.integers(-3, 4, size=shape)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("n, m, p", [(2, 2, 3), (2, 3, 4), (3, 4, 5)])
def test_rect_bilinear_matmul_equals_the_integer_product(n, m, p, levels, dt):
    S = RR.cube_size(n, m, p) + (levels - 1)                          # at the smallest cube, and one above it
    f = RR.standard_rect(n, m, p, S)
    P, Q, T = 2 * n ** levels, 3 * m ** levels, p ** levels
    assert RR.exact_bound(f, levels, 3, Q // m ** levels) < (2 ** 24 if dt == "f32" else 2 ** 53)
    alg = algorithm(f, n, m, p, levels)
    assert (alg.n, alg.m, alg.p, alg.S) == (n, m, p, S)
    assert (alg.rank, alg.levels, alg.products) == (n * m * p, levels, (n * m * p) ** levels)
    rng = np.random.default_rng(levels)
    A, B = small_integers(rng, 2, P, Q), small_integers(rng, 2, Q, T)
    C = alg(dev(A).to(DTYPES[dt][1]), dev(B).to(DTYPES[dt][1]))
    assert C.dtype == DTYPES[dt][1] and tuple(C.shape) == (2, P, T)
    assert np.array_equal(C.cpu().numpy(), (A @ B).astype(DTYPES[dt][0]))
    want = RR.multiply(f, n, m, p, A.astype(DTYPES[dt][0]), B.astype(DTYPES[dt][0]), levels)
    assert np.array_equal(C.cpu().numpy(), want)                      # and the restatement run the same way


def test_rect_padding_and_out_into_a_strided_view():
    f = RR.standard_rect(2, 2, 3)
    alg = algorithm(f, 2, 2, 3, 2, shift=2)
    rng = np.random.default_rng(12)
    A, B = small_integers(rng, 5, 7), small_integers(rng, 7, 10)       # 5 -> 8, 7 -> 8, 10 -> 18
    a, b = dev(A).float(), dev(B).float()
    C = alg(a, b, pad=True)
    assert tuple(C.shape) == (5, 10) and np.array_equal(C.cpu().numpy(), (A @ B).astype(np.float32))
    out = torch.full((5, 10), FILL, device=DEV)
    assert alg(a, b, out=out, pad=True) is out and torch.equal(out, C)
    with pytest.raises(TensorGameError, match=r"P=5 is no multiple of n\^levels=4"):
        alg(a, b)
    with pytest.raises(TensorGameError, match=r"Q=6 is no multiple of m\^levels=4"):
        alg(torch.zeros((4, 6), device=DEV), torch.zeros((6, 9), device=DEV))
    with pytest.raises(TensorGameError, match=r"T=6 is no multiple of p\^levels=9"):
        alg(torch.zeros((4, 4), device=DEV), torch.zeros((4, 6), device=DEV))
    # out= as a strided view of a larger tensor: written in place by the last decode, nothing around it touched
    A, B = small_integers(rng, 2, 8, 4), small_integers(rng, 2, 4, 9)
    big = torch.full((2, 10, 16), FILL, device=DEV)
    view = big[:, 1:9, 4:13]
    assert alg(dev(A).float(), dev(B).float(), out=view) is view
    want = np.full((2, 10, 16), FILL, dtype=np.float32)
    want[:, 1:9, 4:13] = A @ B
    assert np.array_equal(big.cpu().numpy(), want)
    A1 = torch.zeros((4, 4), device=DEV)
    with pytest.raises(TensorGameError, match="out overlaps A"):
        alg(A1, torch.zeros((4, 9), device=DEV), out=A1.as_strided((4, 9), (1, 0)))
    with pytest.raises(TensorGameError, match="mixed dtypes"):
        alg(A1, torch.zeros((4, 9), device=DEV).double())
    with pytest.raises(TensorGameError, match="do not multiply"):
        alg(A1, torch.zeros((6, 9), device=DEV))


def test_rect_refuses_what_is_no_factorisation_of_its_dims():
    f = RR.standard_rect(2, 2, 3)
    bad = f.copy()
    bad[3, 7] += 1                                                    # one coefficient of v changed
    nnz = int(np.count_nonzero(RR.matmul_target(2, 2, 3) - RR.term_sum(bad)))
    assert nnz > 0
    with pytest.raises(TensorGameError, match=rf"no factorisation of <2,2,3> at S=6: residual_nnz={nnz}$"):
        algorithm(bad, 2, 2, 3, 1)
    # a square list given rectangular dims: the standard <2,2,2> list is no factorisation of <2,2,1> or <1,2,2> at S = 4
    sq = RR.standard_rect(2, 2, 2)
    assert algorithm(sq, 2, 2, 2, 1).rank == 8
    for dims in ((2, 2, 1), (1, 2, 2)):
        nnz = int(np.count_nonzero(RR.matmul_target(*dims, 4) - RR.term_sum(sq)))
        assert nnz == {(2, 2, 1): 10, (1, 2, 2): 4}[dims]             # one shared cell of 8 + 4; <1,2,2> lies inside
        with pytest.raises(TensorGameError, match=rf"no factorisation of <{dims[0]},{dims[1]},{dims[2]}> at S=4: "
                                                  rf"residual_nnz={nnz}$"):
            algorithm(sq, *dims, 1)
    with pytest.raises(TensorGameError, match=r"S=4 outside \[max\(n\*m, m\*p, n\*p\)=6,32\]"):
        algorithm(sq, 2, 2, 3, 1)                                     # and it does not fit <2,2,3> at all
    with pytest.raises(TensorGameError, match="bad row"):
        RectBilinearMatmul(dev(f + 1).to(torch.int8), 13, 2, 2, 3)    # a length beyond the table
    with pytest.raises(TensorGameError, match="levels=0"):
        RectBilinearMatmul(dev(f + 1).to(torch.int8), 12, 2, 2, 3, levels=0)


def test_a_rect_call_is_capturable_on_one_stream_and_replays_with_new_inputs():
    alg = algorithm(RR.standard_rect(2, 3, 2), 2, 3, 2, 2)
    rng = np.random.default_rng(14)
    A, B = dev(rng.standard_normal((2, 8, 18))).float(), dev(rng.standard_normal((2, 18, 4))).float()
    out = torch.zeros((2, 8, 4), device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        alg(A, B, out=out)                                            # the leaf's first call happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert alg(A, B, out=out) is out
    A.copy_(dev(rng.standard_normal((2, 8, 18))).float())
    B.copy_(dev(rng.standard_normal((2, 18, 4))).float())
    out.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, alg(A, B))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_223_end_to_end_archive_walks_lift_and_the_rank_11_list_multiplies():
    """<2,2,3> at S = 6: the schoolbook list enters an archive modulo the 48 unsigned symmetries, 8 walks over Z_2 run
    2 000 steps from it (seed 0) and are lifted.  flips_mod2_ref.advance and lift_ref.lift, run on the host from the
    stored form orbits_ref.orbit_canon gives, reach rank 11 on seven of the eight walks and lift six of them: rank 11,
    the known rank of <2,2,3>, is asserted."""
    n, m, p, S = 2, 2, 3, 6
    grp = SymmetryGroup.matmul_rect(n, m, p, device=DEV, signs=False)
    target = functional.matmul_target(1, n, m, p, device=DEV)
    assert grp.order == 48 and bool(grp.fixes(target).all())
    arch = SolutionArchive(S=S, max_rank=12, capacity=64, device=DEV, group=grp)
    lists = standard_rect(n, m, p).to(DEV)[None]
    rep = arch.add(target, lists, dev(np.array([12])))
    assert bool(rep.proven[0]) and int(arch.count) == 1 and int(arch.lowest_rank) == 12
    rep, mod2, res = reduce_archive_lifted(arch, 2_000, walks_per_entry=8, seed=0)
    assert bool(mod2.proven.all()) and torch.equal(rep.proven, res.lifted)
    assert int(arch.lowest_rank) <= 12 and int(arch.lowest_rank) == 11
    tokens, rank, _, _ = arch.entries()
    want = RR.matmul_target(n, m, p)
    for e in range(tokens.shape[0]):                                  # every entry is proven, on the host, exactly
        f = tokens[e, :int(rank[e])].cpu().numpy().astype(np.int64) - 1
        assert np.array_equal(RR.term_sum(f), want), e
    alg = RectBilinearMatmul.from_archive(arch, n, m, p)
    assert (alg.rank, alg.products, alg.S) == (11, 11, 6)
    f = alg.tokens.cpu().numpy().astype(np.int64) - 1
    assert RR.exact_bound(f, 1, 3, 3) < 2 ** 24
    rng = np.random.default_rng(0)
    A, B = small_integers(rng, 2, 4, 6), small_integers(rng, 2, 6, 6)
    assert np.array_equal(alg(dev(A).float(), dev(B).float()).cpu().numpy(), (A @ B).astype(np.float32))
    two = RectBilinearMatmul.from_archive(arch, n, m, p, levels=2)
    assert two.products == 121
    A, B = small_integers(rng, 4, 8), small_integers(rng, 8, 9)
    assert np.array_equal(two(dev(A).double(), dev(B).double()).cpu().numpy(), (A @ B).astype(np.float64))
    with pytest.raises(TensorGameError, match="no factorisation of <2,3,2>"):
        RectBilinearMatmul.from_archive(arch, 2, 3, 2)
    with pytest.raises(TensorGameError, match="empty"):
        RectBilinearMatmul.from_archive(SolutionArchive(S=6, max_rank=12, capacity=4, device=DEV), n, m, p)
