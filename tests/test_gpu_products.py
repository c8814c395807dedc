"""GPU tests of the half-precision block products (include/tensor_game_products.h) against products_ref.py: the encode half
bit for bit (the other operand's block 0 an identity), the exact regime equal to the int64 product on every tail, both
load paths and strided operands, the bound of rule 3 on real inputs, determinism, sizes beyond a grid and beyond the
resident workgroups, and ``FusedBilinearMatmul`` from lists and archives with padding, ``out``, refusals, graph capture and
its error on real inputs next to the restatement's.  Outputs go in canary-guarded buffers; zeros compare without sign."""
import numpy as np
import pytest
import torch

from mat_mul_amd import (FusedBilinearMatmul, SolutionArchive, SymmetryGroup, TensorGameError, functional, ops,
                         reduce_archive, reduce_archive_lifted, standard_rect)

import bilinear_rect_ref as RR
import bilinear_ref as BR
import products_ref as PR
from guarded_buffers import check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}
GRIDS = [(1, 1, 1, 1), (2, 2, 2, 4), (2, 2, 3, 6), (2, 2, 3, 8), (3, 3, 3, 9), (4, 4, 4, 16), (5, 5, 6, 30), (1, 32, 1, 32)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def place(x, H, off=0, ld=None, gap=0):
    """The values x (float32 (batch,rows,cols) holding values of H) as a view of a larger tensor of H: first element
    ``off`` elements in, rows ``ld`` apart, matrices rows*ld + gap apart; every element around the view is a NaN."""
    batch, rows, cols = x.shape
    ld = cols if ld is None else ld
    stride = rows * ld + gap
    flat = torch.full((off + batch * stride + 16,), float("nan"), dtype=TORCH[H], device=DEV)
    view = flat[off:off + batch * stride].view(batch, stride)[:, :rows * ld].view(batch, rows, ld)[:, :, :cols]
    view.copy_(dev(x))
    assert view.data_ptr() == flat.data_ptr() + 2 * off
    return view


def same_but_zero_signs(got, want):
    """Equal bits, except that +0 and -0 are one value."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    g[got == 0] = 0
    w[want == 0] = 0
    return np.array_equal(g, w)


def products(A, B, tokens, R, n, m, p, shift=1):
    """ops.bilinear_products into a guarded buffer."""
    shape = (A.shape[0], R, A.shape[1] // n, B.shape[2] // p)
    buf, out = guarded(shape, torch.float32)
    out.fill_(777.0)
    assert ops.bilinear_products(A, B, tokens, R, n, m, p, shift, out=out) is out
    torch.cuda.synchronize()
    check_flat(buf, "bilinear_products wrote outside M")
    return out.cpu().numpy()


def strassen(golden):
    return BR.coefficients(golden("strassen")["tokens"], 7, 1)


# ---- 1. the encode half, bit for bit ---------------------------------------------------------------------------------------
def grid_values(rng, H, *shape):
    """Values of H with few significant bits at mixed exponents: their small-integer combinations are exact in float32
    and need rounding to H, to ties among them."""
    v = rng.integers(-20, 21, size=shape) * 2.0 ** -rng.integers(0, 12 if H == "f16" else 9, size=shape)
    return PR.RN[H](v.astype(np.float32))


def one_sided_list(rng, R, S, n, m, p, free, shift, extra=3):
    """R + extra rows: part ``free`` random in [-3, 3] on its grid with some rows all zero and one block that no row
    uses (where the grid has two), the other operand's part the unit vector of block 0, rubbish everywhere else."""
    live = (n * m, m * p)
    f = rng.integers(-3, 4, size=(R + extra, 3 * S))
    lo = free * S
    if R > 2:
        f[rng.integers(0, R, size=max(1, R // 5)), lo:lo + live[free]] = 0
    dead = live[free] - 1 if live[free] > 1 else None
    if dead is not None:
        f[:, lo + dead] = 0
    other = (1 - free) * S
    f[:R, other:other + live[1 - free]] = 0
    f[:R, other] = 1
    return f, dead, (f + shift).astype(np.int8)


@pytest.mark.parametrize("H", PR.TYPES)
@pytest.mark.parametrize("R", [1, 7, 256])
@pytest.mark.parametrize("n, m, p, S", GRIDS)
def test_the_encode_half_equals_the_restatement_bit_for_bit(n, m, p, S, R, H):
    rng = np.random.default_rng(1000 * S + 10 * R + (H == "f16"))
    shift = 2 if R == 7 else 1
    batch = 1 if R == 256 else 2
    seen = {"ties": 0, "up": 0, "down": 0}
    for free, q, other in ((0, 16, 5), (0, 9, 34), (1, 16, 40), (1, 9, 3)):
        # free = 0: A (batch, n*other, m*q) is encoded, B's block 0 is the q x q identity (w = q);
        # free = 1: B (batch, m*q, p*other) is encoded, A's block 0 is the identity (h = q)
        f, dead, tokens = one_sided_list(rng, R, S, n, m, p, free, shift)
        gr, gc = ((n, m), (m, p))[free]
        rows, cols = ((other, q), (q, other))[free]
        X = grid_values(rng, H, batch, gr * rows, gc * cols)
        if dead is not None:                                          # a block no row uses holds NaN and infinities
            blk = X[:, (dead // gc) * rows:(dead // gc + 1) * rows, (dead % gc) * cols:(dead % gc + 1) * cols]
            blk[...] = np.nan
            blk[:, ::2, ::3] = np.inf
        ogr, ogc = ((m, p), (n, m))[free]
        Y = grid_values(rng, H, batch, ogr * q, ogc * q) * 1e3
        if ogr * ogc > 1:
            Y[:, -1, -1] = np.nan                                     # rubbish behind the other part's zero coefficients
        Y[:, :q, :q] = np.eye(q, dtype=np.float32)
        acc = RR.encode(f[:R], gr, gc, free, X)
        want = PR.RN[H](acc)
        assert np.isfinite(want).all()
        low = acc.view(np.uint32) & (0xFFFF if H == "bf16" else 0x1FFF)
        half = 0x8000 if H == "bf16" else 0x1000
        seen["ties"] += int((low == half).sum())
        seen["up"] += int((np.abs(want) > np.abs(acc)).sum())
        seen["down"] += int((np.abs(want) < np.abs(acc)).sum())
        for off, pad in ((0, 0), (1, 3)):                             # 16-byte loads where q allows them; single elements
            up = lambda c: c + pad + (-c % 8 if off == 0 else 0)
            Xd = place(X, H, off, up(X.shape[2]), 8 * (off == 0) + pad)
            Yd = place(Y, H, off, up(Y.shape[2]), 16 * (off == 0) + pad)
            A, B = (Xd, Yd) if free == 0 else (Yd, Xd)
            got = products(A, B, dev(tokens), R, n, m, p, shift)
            assert same_but_zero_signs(got, want), (free, q, off)
    if n * m > 1 and R > 1:
        assert min(seen.values()) > 0, seen                           # the inputs do reach ties and both directions


# ---- 2. the exact regime -----------------------------------------------------------------------------------------------
def the_list(name, golden):
    s = strassen(golden)
    return {"strassen": (s, 2, 2, 2), "kron": (BR.kron(s, 2, s, 2), 4, 4, 4), "223": (RR.standard_rect(2, 2, 3), 2, 2, 3),
            "556": (RR.standard_rect(5, 5, 6), 5, 5, 6)}[name]


_ALGORITHMS = {}


def algorithm(name, golden):
    if name not in _ALGORITHMS:
        f, n, m, p = the_list(name, golden)
        _ALGORITHMS[name] = FusedBilinearMatmul(dev(BR.as_tokens(f, 1)), len(f), n, m, p)
        assert (_ALGORITHMS[name].rank, _ALGORITHMS[name].products) == (len(f), len(f))
    return _ALGORITHMS[name]


# every h, w of {1, 31, 32, 33, 65, 129} and every q of {1, 7, 15, 16, 17, 33, 64, 257}: the tails of both tile sizes
BLOCKS = [(1, 1, 1), (31, 7, 33), (32, 16, 32), (33, 15, 31), (65, 17, 129), (129, 33, 65), (65, 64, 65), (32, 257, 1),
          (129, 16, 129), (1, 64, 32)]


@pytest.mark.parametrize("H", PR.TYPES)
@pytest.mark.parametrize("h, q, w", BLOCKS)
@pytest.mark.parametrize("name", ["strassen", "kron", "223", "556"])
def test_small_integers_give_the_bits_of_the_int64_product(golden, name, h, q, w, H):
    f, n, m, p = the_list(name, golden)
    qmax = 7 if PR.exact_ok(f, n, m, p, 7, q, H) else 3
    assert PR.exact_ok(f, n, m, p, qmax, q, H)
    rng = np.random.default_rng(h * 1000 + q)
    alg = algorithm(name, golden)
    fc = alg.tokens.cpu().numpy().astype(np.int64) - alg.shift        # the canonical form is what runs: its order of terms
    assert len(fc) == len(f) and PR.exact_ok(fc, n, m, p, qmax, q, H)
    for batch in (1, 3):
        A = rng.integers(-qmax, qmax + 1, size=(batch, n * h, m * q)).astype(np.float32)
        B = rng.integers(-qmax, qmax + 1, size=(batch, m * q, p * w)).astype(np.float32)
        Ah, Bh = PR.encoded(fc, n, m, 0, A, H), PR.encoded(fc, m, p, 1, B, H)
        M = np.matmul(Ah.astype(np.int64), Bh.astype(np.int64)).astype(np.float32)
        C = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32)
        results = []
        for off in (0, 1):                                            # a 16-byte aligned address and an odd element
            up = lambda c: c + (-c % 8 if off == 0 else 0)
            Ad = place(A, H, off, up(A.shape[2] + 8) + off * 3, 8 + off * 5)
            Bd = place(B, H, off, up(B.shape[2] + 8) + off * 3, 16 + off * 7)
            assert Ad.data_ptr() % 16 == (2 if off else 0) and (batch == 1 or Ad.stride(0) > Ad.shape[1] * Ad.stride(1))
            results.append(products(Ad, Bd, alg.tokens, alg.rank, n, m, p))
            assert same_but_zero_signs(results[-1], M), (batch, off)
            assert same_but_zero_signs(alg(Ad, Bd).cpu().numpy(), C), (batch, off)
        assert same_but_zero_signs(results[0], results[1])


# ---- 3. the bound, 4. determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", PR.TYPES)
@pytest.mark.parametrize("q", [16, 64, 512])
def test_real_inputs_stay_inside_the_bound_and_two_calls_give_the_same_bits(q, H):
    """Measured on the MI355X, max |M - s| / (2^-24 sum|Ahat Bhat|): see DESIGN section 3 (the bound allows 2 q)."""
    n, m, p, S, R, h, w = 2, 2, 3, 6, 5, 33, 40
    rng = np.random.default_rng(q)
    f = rng.integers(-3, 4, size=(R, 3 * S))
    A = PR.RN[H](rng.standard_normal((2, n * h, m * q)).astype(np.float32))
    B = PR.RN[H](rng.standard_normal((2, m * q, p * w)).astype(np.float32))
    Ah, Bh = PR.encoded(f, n, m, 0, A, H), PR.encoded(f, m, p, 1, B, H)
    s, bound = PR.products64(Ah, Bh), PR.bound(Ah, Bh)
    Ad, Bd, tokens = place(A, H), place(B, H), dev((f + 1).astype(np.int8))
    got = products(Ad, Bd, tokens, R, n, m, p)
    err = np.abs(got.astype(np.float64) - s)
    unit = bound / (2 * q)                                            # 2^-24 * sum |Ahat * Bhat|
    print(f"{H} q={q}: max |M - s| / (2^-24 sum|Ahat Bhat|) = {np.max(err[unit > 0] / unit[unit > 0]):.3f} (bound {2 * q})")
    assert (err <= bound).all(), float((err - bound).max())
    again = products(Ad, Bd, tokens, R, n, m, p)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    odd = products(place(A, H, 1, A.shape[2] + 1, 3), place(B, H, 3, B.shape[2] + 5, 1), tokens, R, n, m, p)
    assert np.array_equal(got.view(np.uint32), odd.view(np.uint32))  # the load path changes no bit


# ---- 5. sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch, h, q, w", [(70000, 1, 1, 1), (400, 33, 17, 33)])
def test_batches_beyond_a_grid_dimension_and_tiles_beyond_the_resident_workgroups(golden, batch, h, q, w):
    f = strassen(golden)
    assert PR.exact_ok(f, 2, 2, 2, 7, q, "bf16") and batch * 7 > 8 * 256
    rng = np.random.default_rng(batch)
    A = rng.integers(-7, 8, size=(batch, 2 * h, 2 * q)).astype(np.float32)
    B = rng.integers(-7, 8, size=(batch, 2 * q, 2 * w)).astype(np.float32)
    Ah, Bh = PR.encoded(f, 2, 2, 0, A, "bf16"), PR.encoded(f, 2, 2, 1, B, "bf16")
    M = np.matmul(Ah.astype(np.int64), Bh.astype(np.int64)).astype(np.float32)
    got = products(place(A, "bf16"), place(B, "bf16"), dev(BR.as_tokens(f, 1)), 7, 2, 2, 2)
    assert same_but_zero_signs(got, M)


# ---- 6. FusedBilinearMatmul ----------------------------------------------------------------------------------------------
def multiplies_exactly(alg, seed, H="bf16", lead=(2,)):
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(*lead, 3 * alg.n, 5 * alg.m)).astype(np.float32)
    B = rng.integers(-3, 4, size=(*lead, 5 * alg.m, 2 * alg.p)).astype(np.float32)
    f = alg.tokens.cpu().numpy().astype(np.int64) - alg.shift
    assert PR.exact_ok(f, alg.n, alg.m, alg.p, 3, 5, H)
    C = alg(dev(A).to(TORCH[H]), dev(B).to(TORCH[H]))
    assert C.dtype == torch.float32 and tuple(C.shape) == (*lead, 3 * alg.n, 2 * alg.p)
    return same_but_zero_signs(C.cpu().numpy(), (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32))


def test_from_an_archive_before_and_after_reduce_archive():
    arch = SolutionArchive(S=4, max_rank=8, capacity=64, device=DEV)
    arch.add(dev(BR.matmul_tensor(2).astype(np.int8)[None]), dev(BR.as_tokens(BR.standard(2), 1)[None]), dev(np.array([8])))
    alg = FusedBilinearMatmul.from_archive(arch, 2)
    assert (alg.n, alg.m, alg.p, alg.S, alg.rank, alg.products) == (2, 2, 2, 4, 8, 8) and not hasattr(alg, "levels")
    assert multiplies_exactly(alg, 0) and multiplies_exactly(alg, 1, "f16")
    reduce_archive(arch, 3000, walks_per_entry=8, seed=0)             # the seed and steps of test_gpu_bilinear.py
    alg = FusedBilinearMatmul.from_archive(arch, 2)
    assert (alg.rank, alg.products) == (7, 7) and multiplies_exactly(alg, 2) and multiplies_exactly(alg, 3, "f16")
    assert FusedBilinearMatmul.from_archive(arch, 2, index=0).products in (7, 8)
    with pytest.raises(TensorGameError, match=r"index=\d+ outside"):
        FusedBilinearMatmul.from_archive(arch, 2, index=int(arch.count))
    with pytest.raises(TensorGameError, match="empty"):
        FusedBilinearMatmul.from_archive(SolutionArchive(S=4, max_rank=8, capacity=8, device=DEV), 2)


def test_the_rank_11_list_of_223_from_its_archive():
    """The recipe of test_gpu_rect.py's end-to-end test, same seed and steps: the host restatements predict rank 11."""
    n, m, p, S = 2, 2, 3, 6
    grp = SymmetryGroup.matmul_rect(n, m, p, device=DEV, signs=False)
    target = functional.matmul_target(1, n, m, p, device=DEV)
    arch6 = SolutionArchive(S=S, max_rank=12, capacity=64, device=DEV, group=grp)
    arch6.add(target, standard_rect(n, m, p).to(DEV)[None], dev(np.array([12])))
    reduce_archive_lifted(arch6, 2_000, walks_per_entry=8, seed=0)
    alg = FusedBilinearMatmul.from_archive(arch6, 2, 2, 3)
    assert (alg.rank, alg.products, alg.S, alg.n, alg.m, alg.p) == (11, 11, 6, 2, 2, 3)
    assert multiplies_exactly(alg, 5) and multiplies_exactly(alg, 6, "f16", lead=(2, 1, 3))
    with pytest.raises(TensorGameError, match="no factorisation of <2,3,2>"):
        FusedBilinearMatmul.from_archive(arch6, 2, 3, 2)


@pytest.mark.parametrize("H", PR.TYPES)
def test_padding_out_and_leading_dimensions(golden, H):
    alg = algorithm("strassen", golden)
    rng = np.random.default_rng(7)
    A, B = rng.integers(-3, 4, size=(5, 7)).astype(np.float32), rng.integers(-3, 4, size=(7, 3)).astype(np.float32)
    Ad, Bd = dev(A).to(TORCH[H]), dev(B).to(TORCH[H])
    with pytest.raises(TensorGameError, match=r"P=5 is no multiple of n=2 \(pad=True pads with zeros\)"):
        alg(Ad, Bd)
    C = alg(Ad, Bd, pad=True)
    assert tuple(C.shape) == (5, 3) and same_but_zero_signs(C.cpu().numpy(), A @ B)
    out = torch.full((5, 3), 777.0, device=DEV)
    assert alg(Ad, Bd, out=out, pad=True) is out and same_but_zero_signs(out.cpu().numpy(), A @ B)
    # float32 out, a strided view: written by the decode itself, nothing around it touched
    A, B = rng.integers(-3, 4, size=(2, 3, 4, 6)).astype(np.float32), rng.integers(-3, 4, size=(2, 3, 6, 8)).astype(np.float32)
    Ad, Bd = dev(A).to(TORCH[H]), dev(B).to(TORCH[H])
    buf, big = guarded((2, 3, 4, 11), torch.float32)
    big.fill_(777.0)
    view = big[..., 2:10]
    assert alg(Ad, Bd, out=view) is view
    torch.cuda.synchronize()
    check_flat(buf, "out")
    assert same_but_zero_signs(view.cpu().numpy(), A @ B) and bool((big[..., :2] == 777.0).all() & (big[..., 10:] == 777.0).all())
    low = torch.zeros((2, 3, 4, 8), dtype=TORCH[H], device=DEV)      # out of the operands' type: one more rounding
    assert alg(Ad, Bd, out=low) is low and torch.equal(low.float().cpu(), torch.from_numpy(PR.RN[H]((A @ B).astype(np.float32))))
    assert same_but_zero_signs(alg(Ad.transpose(-1, -2).contiguous().transpose(-1, -2), Bd).cpu().numpy(), A @ B)


def test_every_refusal_by_its_words(golden):
    alg = algorithm("223", golden)
    bf = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    A, B = bf(2, 4, 6), bf(2, 6, 9)
    for args, words in [((A.cpu(), B), "A must live on a ROCm device"), ((A, B.cpu()), "B must live on a ROCm device"),
                        ((A, B.half()), "mixed dtypes: A is torch.bfloat16, B is torch.float16"),
                        ((A.float(), B.float()), "A and B must be bfloat16 or float16, got torch.float32"),
                        ((A[0, 0], B), "A must have at least two dimensions"),
                        ((A, bf(2, 8, 9)), "do not multiply"), ((A, bf(3, 6, 9)), "do not multiply"),
                        ((bf(2, 5, 6), B), "P=5 is no multiple of n=2"), ((bf(2, 4, 7), bf(2, 7, 9)), "Q=7 is no multiple of m=2"),
                        ((A, bf(2, 6, 10)), "T=10 is no multiple of p=3")]:
        with pytest.raises(TensorGameError, match=words):
            alg(*args)
    for out, words in [(torch.zeros((2, 4, 9), dtype=torch.float64, device=DEV), "out must be torch.float32 or torch.bfloat16"),
                       (torch.zeros((2, 4, 8), device=DEV), "out must be"), (torch.zeros((2, 4, 9)), "out must be")]:
        with pytest.raises(TensorGameError, match=words):
            alg(A, B, out=out)
    both = bf(2, 6, 9)
    with pytest.raises(TensorGameError, match="out overlaps B: in-place operation is not supported"):
        alg(A, both, out=both[:, :4])
    with pytest.raises(TensorGameError, match="out overlaps A"):
        alg(both[:, :4, :6], bf(2, 6, 9), out=both[:, :4])
    f, n, m, p = the_list("223", golden)
    tok = dev(BR.as_tokens(f, 1))
    for kw, words in [(dict(n=0), "at least 1"), (dict(S=5), r"S=5 outside \[max"), (dict(S=7), r"tokens must be int8 \(K,21\)"),
                      (dict(n=3), "S=6 outside"), (dict(m=3, p=2), "no factorisation of <2,3,2> at S=6: residual_nnz=")]:
        with pytest.raises(TensorGameError, match=words):
            FusedBilinearMatmul(tok, 12, **{**dict(n=2, m=2, p=3), **kw})
    with pytest.raises(TensorGameError, match="tokens must be int8"):
        FusedBilinearMatmul(tok.float(), 12, 2, 2, 3)
    with pytest.raises(TensorGameError, match="bad row"):
        FusedBilinearMatmul(tok, 13, 2, 2, 3)
    # the ops' own refusals
    with pytest.raises(TensorGameError, match=r"A must be bfloat16 or float16 \(batch,rows,cols\)"):
        ops.bilinear_products(A.float(), B, tok, 12, 2, 2, 3)
    with pytest.raises(TensorGameError, match="the column stride must be 1"):
        ops.bilinear_products(bf(2, 6, 4).transpose(1, 2), B, tok, 12, 2, 2, 3)
    with pytest.raises(TensorGameError, match="mixed dtypes"):
        ops.bilinear_products(A, B.half(), tok, 12, 2, 2, 3)
    with pytest.raises(TensorGameError, match="R=13 above the K=12 rows"):
        ops.bilinear_products(A, B, tok, 13, 2, 2, 3)
    with pytest.raises(TensorGameError, match="out must be contiguous torch.float32"):
        ops.bilinear_products(A, B, tok, 12, 2, 2, 3, out=torch.zeros((2, 12, 2, 4), device=DEV))
    with pytest.raises(TensorGameError, match="m\\*p=9 above S=6"):
        ops.bilinear_products(bf(2, 4, 6), bf(2, 6, 9), tok, 12, 2, 3, 3)


def test_a_list_with_one_token_changed_raises_with_the_residual_count(golden):
    f = strassen(golden).copy()
    f[3, 5] += 1
    nnz = int(np.count_nonzero(BR.matmul_tensor(2) - BR.term_sum(f, 2)))
    assert nnz > 0
    with pytest.raises(TensorGameError, match=rf"no factorisation of <2,2,2> at S=4: residual_nnz={nnz}$"):
        FusedBilinearMatmul(dev(BR.as_tokens(f, 1)), 7, 2)


def test_a_call_is_capturable_on_one_stream_and_replays_with_the_same_bits(golden):
    alg = algorithm("kron", golden)
    rng = np.random.default_rng(14)
    A = dev(rng.standard_normal((2, 64, 72)).astype(np.float32)).bfloat16()
    B = dev(rng.standard_normal((2, 72, 40)).astype(np.float32)).bfloat16()
    out = torch.zeros((2, 64, 40), device=DEV)
    want = alg(A, B).clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # one stream, no parallel branches
        assert alg(A, B, out=out) is out
    out.fill_(777.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ---- 7. the error on real inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["strassen", "kron"])
def test_the_error_on_real_inputs_is_that_of_the_restatement(golden, name):
    """256 x 256 standard-normal bfloat16: e = max|C - C64| / max|C64| of the device may be at most 4 times that of the
    restatement (``encoded``, a float32 numpy matmul, the float32 decode).  Measured: see DESIGN section 5."""
    f, n, m, p = the_list(name, golden)
    rng = np.random.default_rng(256)
    A = PR.rn_bf16(rng.standard_normal((1, 256, 256)).astype(np.float32))
    B = PR.rn_bf16(rng.standard_normal((1, 256, 256)).astype(np.float32))
    C64 = A.astype(np.float64) @ B.astype(np.float64)

    def e(X):
        return float(np.abs(X.astype(np.float64) - C64).max() / np.abs(C64).max())

    e_ref = e(PR.multiply(f, n, m, p, A, B, "bf16"))
    e_gpu = e(algorithm(name, golden)(place(A, "bf16"), place(B, "bf16")).cpu().numpy())
    print(f"{name}: e(gpu) = {e_gpu:.3e}, e(restatement) = {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
    assert e_ref > 0 and e_gpu <= 4 * e_ref
