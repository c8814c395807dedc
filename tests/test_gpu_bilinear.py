"""GPU checks of the bilinear entries (include/tensor_game_bilinear.h) and of ``BilinearMatmul``: ``ops.bilinear_encode``
and ``ops.bilinear_decode`` bit for bit against the host restatement (bilinear_ref.py) on strided, misaligned,
canary-guarded buffers, with random lists that are no factorisations; batches beyond a grid dimension and items beyond
the grid; non-finite blocks behind zero coefficients; ``BilinearMatmul`` exactly equal to the integer product for
Strassen's list (1 to 3 levels), the standard lists and the 49-term Kronecker square, padding, refusals, archives, graph
capture, and the error on real inputs next to the same algorithm in float32 numpy."""
import numpy as np
import pytest
import torch

from mat_mul_amd import BilinearMatmul, SolutionArchive, TensorGameError, ops, reduce_archive

import bilinear_ref as BR
from guarded_buffers import check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0      # the seed test_flips_cpu.py chose: walks from the standard <2,2,2> list reach rank 7 with it
FILL = 777.0  # what every element of a buffer holds that no launch may write
DTYPES = {"f32": (np.float32, torch.float32, np.uint32), "f64": (np.float64, torch.float64, np.uint64)}


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def bits(x, dt):
    return np.ascontiguousarray(x).view(DTYPES[dt][2])


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
# With float32 packs of 4 and float64 packs of 2: the 16-byte path needs w, ld, batch_stride and both offsets to allow it.
LAYOUTS = [
    (1, 1, 1, 0, 0, 0, 0),      # the smallest call; scalar (w)
    (2, 3, 3, 3, 5, 0, 0),      # ld > cols, a batch stride larger than needed; scalar
    (3, 4, 3, 0, 0, 0, 0),      # dense and aligned: packs of 16 bytes, a partial wavefront
    (2, 5, 1, 0, 0, 1, 1),      # both base pointers one element off a 16-byte boundary
    (3, 8, 3, 4, 8, 0, 0),      # packs of 16 bytes with ld > cols and a larger batch stride
    (1, 68, 3, 0, 0, 0, 0),     # packs: 17 (34) per row
    (3, 68, 3, 0, 0, 1, 0),     # the strided base alone is off: scalar, 612 items = two full workgroups and a tail
    (2, 8, 1, 0, 0, 0, 1),      # the dense base alone is off: scalar
    (2, 8, 3, 1, 0, 0, 0),      # ld alone forbids packs
    (2, 4, 3, 0, 1, 0, 0),      # the batch stride alone forbids packs
    (3, 68, 3, 4, 0, 0, 0),     # packs, 153 (306) items: more than one workgroup in float64
]


def random_list(rng, R, n, zero_row, zero_col):
    """Random coefficients in [-3, 3] (no factorisation of anything), about a third of them zero; an all-zero term and an
    all-zero column (index 1 of every part) where asked."""
    S = n * n
    f = rng.integers(-3, 4, size=(R, 3 * S))
    f[rng.random(f.shape) < 0.25] = 0
    if zero_row and R > 1:
        f[R // 2] = 0
    if zero_col:
        f[:, 1::S] = 0
    return f


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("R", [1, 7, 23, 125, 256])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_encode_and_decode_equal_the_restatement_bit_for_bit(n, R, dt):
    rng = np.random.default_rng(1000 * n + R)
    npdt = DTYPES[dt][0]
    for i, (h, w, batch, dld, dbs, off, doff) in enumerate(LAYOUTS):
        shift = 1 + i % 2
        f = random_list(rng, R, n, zero_row=i % 3 == 0, zero_col=i % 3 == 1)
        tok = odd_tokens(f, shift)
        rows, cols = n * h, n * w
        ld = cols + dld
        bs = rows * ld + dbs
        # encode: strided X -> dense Y
        mode = i % 2
        X = Strided(batch, rows, cols, ld, bs, off, dt)
        Xn = rng.standard_normal((batch, rows, cols)).astype(npdt)
        X.view.copy_(dev(Xn))
        Y = dense((batch, R, h, w), doff, dt)
        got = ops.bilinear_encode(X.view, tok, R, n, mode, shift, out=Y.view.view(batch, R, h, w))
        assert got.data_ptr() == Y.view.data_ptr()
        Y.expect(BR.encode(f, n, mode, Xn).reshape(batch, R * h, w))
        X.expect(Xn)                                                                   # the input is as it was
        # decode: dense M -> strided C
        Mn = rng.standard_normal((batch, R, h, w)).astype(npdt)
        M = dense((batch, R, h, w), doff, dt)
        M.view.copy_(dev(Mn.reshape(batch, R * h, w)))
        Cs = Strided(batch, rows, cols, ld, bs, off, dt)
        ops.bilinear_decode(M.view.view(batch, R, h, w), tok, R, n, shift, out=Cs.view)
        Cs.expect(BR.decode(f, n, Mn))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_outputs_allocated_by_the_bindings_and_views_of_larger_tensors(dt):
    rng = np.random.default_rng(5)
    npdt = DTYPES[dt][0]
    f = random_list(rng, 7, 3, False, False)
    tok = dev(BR.as_tokens(f, 2))
    big = rng.standard_normal((4, 9, 24)).astype(npdt)
    view = dev(big)[1:3, 3:9, 4:16]                                   # (2,6,12) inside (4,9,24): not copied
    Y = ops.bilinear_encode(view, tok, 7, 3, 1, 2)
    assert Y.is_contiguous() and tuple(Y.shape) == (2, 7, 2, 4)
    assert np.array_equal(bits(Y.cpu().numpy(), dt), bits(BR.encode(f, 3, 1, big[1:3, 3:9, 4:16]), dt))
    C = ops.bilinear_decode(Y, tok, 7, 3, 2)
    assert tuple(C.shape) == (2, 6, 12)
    assert np.array_equal(bits(C.cpu().numpy(), dt), bits(BR.decode(f, 3, Y.cpu().numpy()), dt))
    with pytest.raises(TensorGameError, match="column stride"):
        ops.bilinear_encode(dev(big).transpose(1, 2)[:, :12, :6], tok, 7, 3, 0, 2)
    with pytest.raises(TensorGameError, match="float32 or float64"):
        ops.bilinear_encode(dev(big).to(torch.float16), tok, 7, 3, 0, 2)
    with pytest.raises(TensorGameError, match="R=9 above"):
        ops.bilinear_encode(dev(big), tok, 9, 3, 0, 2)
    with pytest.raises(TensorGameError, match="overlap"):
        flat = torch.zeros(160, dtype=DTYPES[dt][1], device=DEV)
        ops.bilinear_decode(flat[:112].view(2, 7, 2, 4), tok, 7, 3, 2, out=flat[8:152].view(2, 6, 12))


def test_a_batch_of_70000_is_not_capped_by_a_grid_dimension():
    rng = np.random.default_rng(6)
    f = random_list(rng, 7, 2, False, False)
    tok = dev(BR.as_tokens(f, 1))
    Xn = rng.standard_normal((70000, 2, 2)).astype(np.float32)
    Y = ops.bilinear_encode(dev(Xn), tok, 7, 2, 0, 1)
    want = BR.encode(f, 2, 0, Xn)
    assert tuple(Y.shape) == (70000, 7, 1, 1) and np.array_equal(bits(Y.cpu().numpy(), "f32"), bits(want, "f32"))
    C = ops.bilinear_decode(Y, tok, 7, 2, 1)
    assert np.array_equal(bits(C.cpu().numpy(), "f32"), bits(BR.decode(f, 2, want), "f32"))


@pytest.mark.parametrize("w", [240004, 60001])                        # packs of 16 bytes; scalar
def test_more_items_than_the_grid_holds_at_once(w):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    batch, h, n, R = 3, 3, 2, 2
    items = batch * h * (w // 4 if w % 4 == 0 else w)
    assert items > 8 * cus * 256                                      # the launch starts at most 8 workgroups per CU
    rng = np.random.default_rng(w)
    f = random_list(rng, R, n, False, False)
    tok = dev(BR.as_tokens(f, 1))
    Xn = rng.standard_normal((batch, n * h, n * w)).astype(np.float32)
    Y = ops.bilinear_encode(dev(Xn), tok, R, n, 1, 1)
    want = BR.encode(f, n, 1, Xn)
    assert np.array_equal(bits(Y.cpu().numpy(), "f32"), bits(want, "f32"))
    C = ops.bilinear_decode(Y, tok, R, n, 1)
    assert np.array_equal(bits(C.cpu().numpy(), "f32"), bits(BR.decode(f, n, want), "f32"))


@pytest.mark.parametrize("dt, w", [("f32", 4), ("f32", 3), ("f64", 2), ("f64", 5)])
def test_zero_coefficients_do_not_spread_non_finite_values(dt, w):
    rng = np.random.default_rng(7)
    npdt = DTYPES[dt][0]
    n, R, h, batch = 2, 7, 2, 2
    f = random_list(rng, R, n, False, False)
    f[:3, 2] = 0                                                      # terms 0..2 do not use block 2 of A
    f[3:, 2] = (1, -2, 3, -1)
    f[:2, 8 + 1] = 0                                                  # block 1 of C does not use products 0 and 1
    f[2:, 8 + 1] = (2, 1, -1, 3, -3)
    tok = dev(BR.as_tokens(f, 1))
    Xn = rng.standard_normal((batch, n * h, n * w)).astype(npdt)
    Xn[:, h:, :w] = np.nan                                            # block 2 = (1, 0)
    Xn[0, h, 0] = np.inf
    got = ops.bilinear_encode(dev(Xn), tok, R, n, 0, 1).cpu().numpy()
    want = BR.encode(f, n, 0, Xn)
    assert np.isfinite(got[:, :3]).all() and not np.isfinite(got[:, 3:]).any()
    assert np.array_equal(bits(got[:, :3], dt), bits(want[:, :3], dt)) and np.array_equal(got, want, equal_nan=True)
    Mn = rng.standard_normal((batch, R, h, w)).astype(npdt)
    Mn[:, :2] = np.nan
    Mn[1, 0, 0, 0] = -np.inf
    got = ops.bilinear_decode(dev(Mn), tok, R, n, 1).cpu().numpy()
    want = BR.decode(f, n, Mn)
    blk = (slice(None), slice(0, h), slice(w, 2 * w))                 # block 1 = (0, 1)
    assert np.isfinite(got[blk]).all() and np.array_equal(bits(got[blk], dt), bits(want[blk], dt))
    assert np.array_equal(got, want, equal_nan=True) and not np.isfinite(got[:, :h, :w]).any()


# ---- BilinearMatmul ----------------------------------------------------------------------------------------------------
def strassen(golden):
    return BR.coefficients(golden("strassen")["tokens"], 7, 1)


def the_list(name, golden):
    """(f, n) of the named list."""
    if name == "strassen":
        return strassen(golden), 2
    if name == "kron":
        return BR.kron(strassen(golden), 2, strassen(golden), 2), 4
    n = int(name[-1])
    return BR.standard(n), n


def algorithm(f, n, levels, shift=1):
    return BilinearMatmul(dev(BR.as_tokens(f, shift)), len(f), n=n, shift=shift, levels=levels)


def small_integers(rng, *shape):
    return rng.integers(-3, 4, size=shape)


EXACT = [("strassen", 1), ("strassen", 2), ("strassen", 3), ("standard3", 1), ("standard5", 1), ("kron", 1)]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name, levels", EXACT)
def test_bilinear_matmul_equals_the_integer_product(name, levels, dt, golden):
    f, n = the_list(name, golden)
    D = n ** levels
    P, Q, T = 2 * D, 3 * D, D
    assert BR.exact_bound(f, n, levels, 3, Q // D) < (2 ** 24 if dt == "f32" else 2 ** 53)
    alg = algorithm(f, n, levels)
    assert (alg.n, alg.rank, alg.levels, alg.products) == (n, len(f), levels, len(f) ** levels)
    rng = np.random.default_rng(levels)
    A, B = small_integers(rng, 2, P, Q), small_integers(rng, 2, Q, T)
    C = alg(dev(A).to(DTYPES[dt][1]), dev(B).to(DTYPES[dt][1]))
    assert C.dtype == DTYPES[dt][1] and tuple(C.shape) == (2, P, T)
    assert np.array_equal(C.cpu().numpy(), (A @ B).astype(DTYPES[dt][0]))


def test_two_levels_of_strassen_and_the_kronecker_list_give_the_same_matrix(golden):
    f = strassen(golden)
    rng = np.random.default_rng(11)
    A, B = dev(small_integers(rng, 3, 2, 8, 4)).float(), dev(small_integers(rng, 3, 2, 4, 12)).float()
    two = algorithm(f, 2, 2)(A, B)
    one = algorithm(BR.kron(f, 2, f, 2), 4, 1)(A, B)
    assert tuple(two.shape) == (3, 2, 8, 12) and torch.equal(two, one) and torch.equal(two, A @ B)


def test_padding_is_exact_and_its_absence_refuses_by_dimension_name(golden):
    alg = algorithm(strassen(golden), 2, 2)
    rng = np.random.default_rng(12)
    A, B = small_integers(rng, 5, 7), small_integers(rng, 7, 3)
    a, b = dev(A).float(), dev(B).float()
    C = alg(a, b, pad=True)
    assert tuple(C.shape) == (5, 3) and np.array_equal(C.cpu().numpy(), (A @ B).astype(np.float32))
    out = torch.full((5, 3), FILL, device=DEV)
    assert alg(a, b, out=out, pad=True) is out and torch.equal(out, C)
    with pytest.raises(TensorGameError, match=r"P=5 is no multiple of n\^levels=4"):
        alg(a, b)
    with pytest.raises(TensorGameError, match="Q=6"):
        alg(torch.zeros((4, 6), device=DEV), torch.zeros((6, 4), device=DEV))
    with pytest.raises(TensorGameError, match="T=2"):
        alg(torch.zeros((4, 4), device=DEV), torch.zeros((4, 2), device=DEV))


def test_refusals(golden):
    f = strassen(golden)
    alg = algorithm(f, 2, 1)
    A = torch.zeros((4, 4), device=DEV)
    with pytest.raises(TensorGameError, match="out overlaps A"):
        alg(A, torch.ones((4, 4), device=DEV), out=A)
    both = torch.zeros((2, 4, 4), device=DEV)
    with pytest.raises(TensorGameError, match="out overlaps B"):
        alg(both[0], both[1], out=both[1])
    with pytest.raises(TensorGameError, match="mixed dtypes"):
        alg(A, A.double())
    with pytest.raises(TensorGameError, match="float32 or float64"):
        alg(A.half(), A.half())
    with pytest.raises(TensorGameError, match="do not multiply"):
        alg(A, torch.zeros((6, 4), device=DEV))
    # one token changed: no factorisation any more, and the message counts the residual
    bad = f.copy()
    bad[3, 5] += 1
    nnz = int(np.count_nonzero(BR.matmul_tensor(2) - BR.term_sum(bad, 2)))
    assert nnz > 0
    with pytest.raises(TensorGameError, match=rf"no factorisation of <2,2,2>: residual_nnz={nnz}$"):
        algorithm(bad, 2, 1)
    # a list that is proven, of another target: twice the matmul tensor
    twice = np.concatenate([f, f])
    nnz2 = int(np.count_nonzero(BR.matmul_tensor(2) - BR.term_sum(twice, 2)))
    arch = SolutionArchive(S=4, max_rank=14, capacity=4, device=DEV)
    lists = dev(BR.as_tokens(twice, 1)[None])
    rep = arch.add(dev((2 * BR.matmul_tensor(2)).astype(np.int8)[None]), lists, dev(np.array([14])))
    assert bool(rep.proven[0]) and nnz2 == 8
    with pytest.raises(TensorGameError, match=r"no factorisation of <2,2,2>: residual_nnz=8$"):
        BilinearMatmul.from_archive(arch)
    with pytest.raises(TensorGameError, match="bad row"):
        BilinearMatmul(dev(BR.as_tokens(f, 1)), 8, n=2)               # a length beyond the table
    with pytest.raises(TensorGameError, match="n=6"):
        BilinearMatmul(torch.zeros((1, 108), dtype=torch.int8, device=DEV), 1, n=6)


def test_null_terms_and_cancelling_pairs_cost_no_products(golden):
    f = strassen(golden)
    null = np.zeros((1, 12), dtype=np.int64)
    null[0, :4] = 1                                                   # v and w all zero
    pair = np.array([[1, 0, -1, 0, 0, 1, 1, 0, 1, 1, 0, 0]])
    padded = np.concatenate([f[:3], null, pair, f[3:], pair * np.repeat([1, 1, -1], 4)])
    alg = algorithm(padded, 2, 1)
    assert alg.rank == 7 and alg.products == 7 and tuple(alg.tokens.shape) == (7, 12)
    rng = np.random.default_rng(13)
    A, B = small_integers(rng, 4, 2), small_integers(rng, 2, 6)
    assert np.array_equal(alg(dev(A).double(), dev(B).double()).cpu().numpy(), (A @ B).astype(np.float64))


def _multiplies_exactly(alg, f, seed):
    assert BR.exact_bound(f, alg.n, 1, 3, 3) < 2 ** 24
    rng = np.random.default_rng(seed)
    A, B = small_integers(rng, 2, 4, 6), small_integers(rng, 2, 6, 2)
    return np.array_equal(alg(dev(A).float(), dev(B).float()).cpu().numpy(), (A @ B).astype(np.float32))


def test_from_archive_picks_the_lowest_rank(golden):
    f = strassen(golden)
    lists = np.stack([BR.as_tokens(BR.standard(2), 1, K=8), BR.as_tokens(f, 1, K=8)])
    arch = SolutionArchive(S=4, max_rank=8, capacity=8, device=DEV)
    target = dev(np.repeat(BR.matmul_tensor(2).astype(np.int8)[None], 2, axis=0))
    rep = arch.add(target, dev(lists), dev(np.array([8, 7])))
    assert bool(rep.fresh.all()) and int(arch.count) == 2
    alg = BilinearMatmul.from_archive(arch)
    assert (alg.rank, alg.n, alg.levels) == (7, 2, 1) and _multiplies_exactly(alg, f, 0)
    first = BilinearMatmul.from_archive(arch, index=0, levels=2)
    assert (first.rank, first.products) == (8, 64)
    with pytest.raises(TensorGameError, match="index=2"):
        BilinearMatmul.from_archive(arch, index=2)
    with pytest.raises(TensorGameError, match="empty"):
        BilinearMatmul.from_archive(SolutionArchive(S=4, max_rank=8, capacity=8, device=DEV))


def test_every_entry_of_a_reduced_archive_multiplies_exactly():
    arch = SolutionArchive(S=4, max_rank=8, capacity=64, device=DEV)
    lists = dev(BR.as_tokens(BR.standard(2), 1)[None])
    arch.add(dev(BR.matmul_tensor(2).astype(np.int8)[None]), lists, dev(np.array([8])))
    reduce_archive(arch, 3000, walks_per_entry=8, seed=SEED)
    tokens, rank, _, _ = arch.entries()
    assert int(arch.lowest_rank) == 7 and len(rank) > 1
    assert BilinearMatmul.from_archive(arch).rank == 7
    for i, r in enumerate(rank.tolist()):
        alg = BilinearMatmul.from_archive(arch, index=i)
        f = BR.coefficients(tokens[i].cpu().numpy(), r, 1)
        assert alg.rank == r and _multiplies_exactly(alg, f, i), (i, r)


def test_a_call_is_capturable_on_one_stream_and_replays_with_new_inputs(golden):
    alg = algorithm(strassen(golden), 2, 2)
    rng = np.random.default_rng(14)
    A, B = dev(rng.standard_normal((2, 8, 12))).float(), dev(rng.standard_normal((2, 12, 4))).float()
    out = torch.zeros((2, 8, 4), device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        alg(A, B, out=out)                                            # the leaf's first call happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert alg(A, B, out=out) is out
    A.copy_(dev(rng.standard_normal((2, 8, 12))).float())
    B.copy_(dev(rng.standard_normal((2, 12, 4))).float())
    out.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, alg(A, B))


def test_real_inputs_err_like_the_same_algorithm_in_float32_numpy(golden):
    """e(X) = max|X - C64| / max|C64| for standard-normal float32 inputs, 64 x 64 blocks at two levels of Strassen.  The
    device result and bilinear_ref.multiply in float32 numpy evaluate the same algorithm in the same precision and
    differ only in the order of the leaf's inner sums; both obey the same a-priori bound, and a wrong coefficient or a
    misplaced block gives an error of order 1, about 10^6 times beyond it.  The margin is a factor of 4."""
    f = strassen(golden)
    rng = np.random.default_rng(15)
    A = rng.standard_normal((1, 256, 256)).astype(np.float32)
    B = rng.standard_normal((1, 256, 256)).astype(np.float32)
    C64 = A.astype(np.float64) @ B.astype(np.float64)

    def e(X):
        return float(np.abs(X.astype(np.float64) - C64).max() / np.abs(C64).max())

    e_ref = e(BR.multiply(f, 2, A, B, levels=2))
    e_gpu = e(algorithm(f, 2, 2)(dev(A), dev(B)).cpu().numpy())
    print(f"e(gpu) = {e_gpu:.3e}, e(float32 numpy) = {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
    assert 0 < e_ref < 1e-4 and e_gpu <= 4 * e_ref
