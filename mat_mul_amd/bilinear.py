"""``BilinearMatmul``: a proven factorisation of <n,n,n> run as what it is, a matrix multiplication.

A list of R terms (u_r, v_r, w_r) that sums to the matmul tensor in the index convention of ``build_matmul_tensor``
(a = i*n+j, b = j*n+k, c = i*n+k) multiplies matrices cut into n x n row-major blocks with R block products instead of
n^3:

    C_c = sum_r w_r[c] * (sum_a u_r[a] * A_a) (sum_b v_r[b] * B_b)

The two sums over blocks are ``ops.bilinear_encode`` (include/tensor_game_bilinear.h), the sum over r is
``ops.bilinear_decode``; the block products go to ``leaf`` (``torch.bmm``), or, with ``levels`` > 1, through the same
algorithm again: the (batch,R,h,w) output of one encode is the (batch*R,h,w) input of the next.

    alg = BilinearMatmul(tokens, rank, n=2, shift=1, levels=2)    # tokens int8 (K,3S) on the device
    alg = BilinearMatmul.from_archive(arch, index=None, levels=1) # index None: the lowest-rank entry (first of equals)
    C = alg(A, B)                                                 # A (..., P, Q), B (..., Q, T), float32 or float64
    C = alg(A, B, out=C, pad=True, leaf=torch.bmm)
    alg.n, alg.rank, alg.levels, alg.products                     # products = rank ** levels (against n ** (3*levels))

Construction proves the list (``ops.solution_canon`` against ``build_matmul_tensor(1, n, n, n)``) and runs the canonical
form, so null terms and a term followed by its negative cost no products; there is no way round the proof.  The kernels'
arithmetic is defined bit for bit by the header; the result as a whole is as exact as the algorithm is: integer inputs
whose intermediates stay below 2^24 (2^53 in float64) give the exact product, real inputs the error growth of the list.
Not done here: a leaf GEMM of our own, half-precision operands, choosing ``levels``.

``RectBilinearMatmul`` is the same for a rectangular <n,m,p> (include/tensor_game_rect.h: A in n x m blocks, B in m x p,
C in n x p, a list of any cube size S >= max(n*m, m*p, n*p)), and ``standard_rect`` its schoolbook list.

``FusedBilinearMatmul`` runs a proven list for <n,m,p> on bfloat16 or float16 operands: one ``ops.bilinear_products`` (the
block combinations formed while the products load their tiles, include/tensor_game_products.h) and one float32 decode.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import functional, ops
from ._lib import TG_BILINEAR_MAX_N, TG_BILINEAR_MIN_N, TG_MAX_S, TG_SOL_MAX_SHIFT, TensorGameError

__all__ = ["BilinearMatmul", "RectBilinearMatmul", "FusedBilinearMatmul", "standard_rect"]


def _byte_range(t: torch.Tensor):
    """[first, one past the last) byte of a tensor's elements (strides of either sign)."""
    lo = hi = 0
    for size, stride in zip(t.shape, t.stride()):
        if size == 0:
            return t.data_ptr(), t.data_ptr()
        lo, hi = lo + min(0, (size - 1) * stride), hi + max(0, (size - 1) * stride)
    return t.data_ptr() + lo * t.element_size(), t.data_ptr() + (hi + 1) * t.element_size()


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (a0, a1), (b0, b1) = _byte_range(a), _byte_range(b)
    return a0 < b1 and b0 < a1


def _need_device(fn: str, t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise TensorGameError(fn, -1, f"{name} must live on a ROCm device (got {t.device}); there is no CPU path")


class _Bilinear:
    """What the two classes share: the proof, the index choice of ``from_archive`` and the call.  A class gives ``_fn`` (its
    name in messages), ``_grid()`` (the three grid sizes and what a message calls them), ``_encode`` and ``_decode``."""

    def _prove(self, tokens: torch.Tensor, rank: int, target: torch.Tensor, what: str) -> None:
        """Sets ``rank``, ``tokens`` (the canonical form) and ``device``, or raises: the list is no factorisation of
        ``what``.  One host sync."""
        lengths = torch.full((1,), int(rank), dtype=torch.int64, device=tokens.device)
        canon, crank, _, res = ops.solution_canon(target, tokens[None], lengths, shift=self.shift)
        res, crank = torch.stack((res, crank)).flatten().tolist()      # the one host sync
        if res != 0:
            why = "a bad row (its length, or a negation that leaves int8)" if res < 0 else f"residual_nnz={res}"
            raise TensorGameError(self._fn, -1, f"the list is no factorisation of {what}: {why}")
        self.rank = int(crank)
        self.tokens = canon[0, :self.rank].contiguous()
        self.device = tokens.device

    @staticmethod
    def _entry(fn: str, arch, index: Optional[int]):
        """(tokens, rank) of entry ``index`` of an archive (None: the entry of lowest rank, the first of equals)."""
        tokens, rank, _, _ = arch.entries()
        ranks = rank.tolist()
        if not ranks:
            raise TensorGameError(fn, -1, "the archive is empty")
        if index is None:
            index = ranks.index(min(ranks))
        if not 0 <= index < len(ranks):
            raise TensorGameError(fn, -1, f"index={index} outside [0,{len(ranks)})")
        return tokens[index].contiguous(), ranks[index]

    @property
    def products(self) -> int:
        """Leaf block products of one call: rank ** levels, where the schoolbook method takes (n*m*p) ** levels
        (n ** (3 * levels) on the square grid)."""
        return self.rank ** self.levels

    def __call__(self, A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None, pad: bool = False,
                 leaf=torch.bmm) -> torch.Tensor:
        """A (...,P,Q) times B (...,Q,T), float32 or float64 on the list's device, equal leading dimensions.  P must be
        a multiple of n^levels, Q of m^levels and T of p^levels (m = p = n in the square class), or ``pad`` zero-pads
        them up (with torch) and slices the result.  ``leaf`` takes two (batch * rank^levels, ., .) operands and returns
        their batched product.  ``out`` (...,P,T) may not overlap A or B.  No host sync; capturable on one stream."""
        fn = self._fn
        for t, name in ((A, "A"), (B, "B")):
            _need_device(fn, t, name)
            if t.device != self.device:
                raise TensorGameError(fn, -1, f"{name} is on {t.device}, the list on {self.device}")
            if t.dim() < 2:
                raise TensorGameError(fn, -1, f"{name} must have at least two dimensions, got {tuple(t.shape)}")
        if A.dtype != B.dtype:
            raise TensorGameError(fn, -1, f"mixed dtypes: A is {A.dtype}, B is {B.dtype}")
        if A.dtype not in (torch.float32, torch.float64):
            raise TensorGameError(fn, -1, f"A and B must be float32 or float64, got {A.dtype}")
        lead, (P, Q), (Q2, T) = tuple(A.shape[:-2]), A.shape[-2:], B.shape[-2:]
        if tuple(B.shape[:-2]) != lead or Q2 != Q:
            raise TensorGameError(fn, -1, f"A {tuple(A.shape)} and B {tuple(B.shape)} do not multiply: equal leading "
                                          "dimensions and Q are required")
        if out is not None:
            if out.dtype != A.dtype or tuple(out.shape) != (*lead, P, T) or out.device != A.device:
                raise TensorGameError(fn, -1, f"out must be {A.dtype} {(*lead, P, T)} on {A.device}, got {out.dtype} "
                                              f"{tuple(out.shape)} on {out.device}")
            for t, name in ((A, "A"), (B, "B")):
                if _overlap(out, t):
                    raise TensorGameError(fn, -1, f"out overlaps {name}: in-place operation is not supported")
        sizes = {name: (size, d, letter) for name, size, (d, letter) in zip("PQT", (P, Q, T), self._grid())}
        up = {name: -size % d ** self.levels for name, (size, d, _) in sizes.items()}
        if any(up.values()) and not pad:
            name = next(k for k, v in up.items() if v)
            size, d, letter = sizes[name]
            raise TensorGameError(fn, -1, f"{name}={size} is no multiple of {letter}^levels={d ** self.levels} (pad=True "
                                          "pads with zeros)")
        batch = math.prod(lead)
        a, b = A.reshape(batch, P, Q), B.reshape(batch, Q, T)
        if any(up.values()):
            a = torch.nn.functional.pad(a, (0, up["Q"], 0, up["P"]))
            b = torch.nn.functional.pad(b, (0, up["T"], 0, up["Q"]))
        a = a if a.stride(2) == 1 else a.contiguous()
        b = b if b.stride(2) == 1 else b.contiguous()
        for _ in range(self.levels):
            a = self._encode(a, 0).flatten(0, 1)
            b = self._encode(b, 1).flatten(0, 1)
        m = leaf(a, b)
        if tuple(m.shape) != (a.shape[0], a.shape[1], b.shape[2]) or m.dtype != A.dtype:
            raise TensorGameError(fn, -1, f"leaf returned {m.dtype} {tuple(m.shape)}, expected {A.dtype} "
                                          f"{(a.shape[0], a.shape[1], b.shape[2])}")
        m = m.contiguous()
        direct = None                                   # the last decode writes into `out` itself where it can
        if out is not None and not any(up.values()) and out.stride(-1) == 1:
            try:
                direct = out.view(batch, P, T)
            except RuntimeError:
                pass
        for level in range(self.levels):
            m = m.view(m.shape[0] // self.rank, self.rank, m.shape[1], m.shape[2])
            m = self._decode(m, direct if level == self.levels - 1 else None)
        if direct is not None:
            return out
        m = m[:, :P, :T].reshape(*lead, P, T)
        if out is None:
            return m
        out.copy_(m)
        return out


class BilinearMatmul(_Bilinear):
    _fn = "BilinearMatmul"

    def __init__(self, tokens: torch.Tensor, rank: int, n: int = 2, shift: int = 1, levels: int = 1):
        """``tokens`` int8 (K,3n^2) on a ROCm device, of which the first ``rank`` rows are the list.  Raises
        TensorGameError unless the list is proven against <n,n,n>.  One host sync (the proof's verdict)."""
        fn = self._fn
        _need_device(fn, tokens, "tokens")
        self.n, self.shift, self.levels = int(n), int(shift), int(levels)
        if not TG_BILINEAR_MIN_N <= self.n <= TG_BILINEAR_MAX_N:
            raise TensorGameError(fn, -1, f"n={n} outside [{TG_BILINEAR_MIN_N},{TG_BILINEAR_MAX_N}]")
        if self.levels < 1:
            raise TensorGameError(fn, -1, f"levels={levels} < 1")
        S = self.n * self.n
        if tokens.dtype != torch.int8 or tokens.dim() != 2 or tokens.shape[1] != 3 * S:
            raise TensorGameError(fn, -1, f"tokens must be int8 (K,{3 * S}) for n={n}, got {tokens.dtype} "
                                          f"{tuple(tokens.shape)}")
        target = functional.build_matmul_tensor(1, self.n, self.n, self.n, device=tokens.device)
        self._prove(tokens, rank, target, f"<{n},{n},{n}>")

    @classmethod
    def from_archive(cls, arch, index: Optional[int] = None, levels: int = 1) -> "BilinearMatmul":
        """The algorithm of entry ``index`` of a ``SolutionArchive`` (None: the entry of lowest rank, the first of
        equals).  The entry is proven again, against <n,n,n> with n = sqrt(arch.S): an archive may hold factorisations
        of other targets.  Synchronises (``entries``)."""
        fn = "BilinearMatmul.from_archive"
        n = math.isqrt(arch.S)
        if n * n != arch.S:
            raise TensorGameError(fn, -1, f"the archive is of S={arch.S}, which is no square: no <n,n,n>")
        tokens, rank = cls._entry(fn, arch, index)
        return cls(tokens, rank, n=n, shift=arch.shift, levels=levels)

    def _grid(self):
        return ((self.n, "n"),) * 3

    def _encode(self, x, part):
        return ops.bilinear_encode(x, self.tokens, self.rank, self.n, part, self.shift)

    def _decode(self, m, out):
        return ops.bilinear_decode(m, self.tokens, self.rank, self.n, self.shift, out=out)


def standard_rect(n: int, m: int, p: int, S: Optional[int] = None, shift: int = 1) -> torch.Tensor:
    """The schoolbook algorithm for <n,m,p> (include/tensor_game_rect.h) as archive-format tokens: int8 (n*m*p,3S) on the
    host, term (i,j,k) in ascending order with u[i*m+j] = v[j*p+k] = w[i*p+k] = 1, every other coefficient 0.  S
    defaults to max(n*m, m*p, n*p).  A proven list to start walks from, or to run."""
    n, m, p = int(n), int(m), int(p)
    if min(n, m, p) < 1:
        raise TensorGameError("standard_rect", -1, f"n={n}, m={m}, p={p}: every dimension must be at least 1")
    need = max(n * m, m * p, n * p)
    S = need if S is None else int(S)
    if not need <= S <= TG_MAX_S:
        raise TensorGameError("standard_rect", -1, f"S={S} outside [max(n*m, m*p, n*p)={need},{TG_MAX_S}]")
    if not 0 <= shift <= TG_SOL_MAX_SHIFT:
        raise TensorGameError("standard_rect", -1, f"shift={shift} outside [0,{TG_SOL_MAX_SHIFT}]")
    i, j, k = (x.reshape(-1) for x in torch.meshgrid(torch.arange(n), torch.arange(m), torch.arange(p), indexing="ij"))
    tokens = torch.full((n * m * p, 3 * S), int(shift), dtype=torch.int8)
    t = torch.arange(n * m * p)
    tokens[t, i * m + j] = tokens[t, S + j * p + k] = tokens[t, 2 * S + i * p + k] = int(shift) + 1
    return tokens


class RectBilinearMatmul(_Bilinear):
    """A proven factorisation of the rectangular tensor <n,m,p> in a cube of size S, run as a matrix multiplication:
    A is cut into n x m blocks, B into m x p, C into n x p, and R block products replace n*m*p.

        alg = RectBilinearMatmul(tokens, rank, n=2, m=2, p=3, S=None, shift=1, levels=1)   # tokens int8 (K,3S), device
        alg = RectBilinearMatmul.from_archive(arch, 2, 2, 3, index=None, levels=1)
        C = alg(A, B, out=None, pad=False, leaf=torch.bmm)        # A (...,P,Q) @ B (...,Q,T), float32 or float64
        alg.n, alg.m, alg.p, alg.S, alg.rank, alg.levels, alg.products

    Construction proves the list (``ops.solution_canon`` against ``functional.matmul_target(1, n, m, p, S)``) and runs
    the canonical form; there is no way round the proof.  The encodes and decodes are ``ops.bilinear_rect_encode`` and
    ``ops.bilinear_rect_decode`` (include/tensor_game_rect.h states their arithmetic bit for bit); the padding entries
    of the list (beyond n*m, m*p, n*p) are not read."""
    _fn = "RectBilinearMatmul"

    def __init__(self, tokens: torch.Tensor, rank: int, n: int, m: int, p: int, S: Optional[int] = None, shift: int = 1,
                 levels: int = 1):
        """``tokens`` int8 (K,3S) on a ROCm device, of which the first ``rank`` rows are the list; S defaults to the
        width of ``tokens``.  Raises TensorGameError unless the list is proven against <n,m,p> in that cube.  One host
        sync (the proof's verdict)."""
        fn = self._fn
        _need_device(fn, tokens, "tokens")
        self.n, self.m, self.p, self.shift, self.levels = int(n), int(m), int(p), int(shift), int(levels)
        if min(self.n, self.m, self.p) < 1:
            raise TensorGameError(fn, -1, f"n={n}, m={m}, p={p}: every dimension must be at least 1")
        if self.levels < 1:
            raise TensorGameError(fn, -1, f"levels={levels} < 1")
        need = max(self.n * self.m, self.m * self.p, self.n * self.p)
        if tokens.dtype != torch.int8 or tokens.dim() != 2 or tokens.shape[1] % 3:
            raise TensorGameError(fn, -1, f"tokens must be int8 (K,3S), got {tokens.dtype} {tuple(tokens.shape)}")
        self.S = tokens.shape[1] // 3 if S is None else int(S)
        if not need <= self.S <= TG_MAX_S:
            raise TensorGameError(fn, -1, f"S={self.S} outside [max(n*m, m*p, n*p)={need},{TG_MAX_S}] for "
                                          f"<{n},{m},{p}>")
        if tokens.shape[1] != 3 * self.S:
            raise TensorGameError(fn, -1, f"tokens must be int8 (K,{3 * self.S}) for S={self.S}, got "
                                          f"{tuple(tokens.shape)}")
        target = functional.matmul_target(1, self.n, self.m, self.p, self.S, device=tokens.device)
        self._prove(tokens, rank, target, f"<{n},{m},{p}> at S={self.S}")

    @classmethod
    def from_archive(cls, arch, n: int, m: int, p: int, index: Optional[int] = None,
                     levels: int = 1) -> "RectBilinearMatmul":
        """The algorithm of entry ``index`` of a ``SolutionArchive`` of cube size arch.S (None: the entry of lowest rank,
        the first of equals).  The entry is proven again, against <n,m,p>.  Synchronises (``entries``)."""
        tokens, rank = cls._entry("RectBilinearMatmul.from_archive", arch, index)
        return cls(tokens, rank, n, m, p, S=arch.S, shift=arch.shift, levels=levels)

    def _grid(self):
        return (self.n, "n"), (self.m, "m"), (self.p, "p")

    def _encode(self, x, part):
        gr, gc = ((self.n, self.m), (self.m, self.p))[part]
        return ops.bilinear_rect_encode(x, self.tokens, self.rank, gr, gc, part, self.shift)

    def _decode(self, m, out):
        return ops.bilinear_rect_decode(m, self.tokens, self.rank, self.n, self.p, self.shift, out=out)


class FusedBilinearMatmul(_Bilinear):
    """A proven factorisation of <n,m,p> in a cube of size S, run on bfloat16 or float16 operands in two launches: the R
    block products with the block combinations formed on load (``ops.bilinear_products``: include/tensor_game_products.h
    states the arithmetic; the combinations are rounded to the operands' type, the products accumulated in float32 on the
    matrix cores), and ``ops.bilinear_rect_decode`` in float32 on the grid n x p.

        alg = FusedBilinearMatmul(tokens, rank, n, m=None, p=None, S=None, shift=1)      # tokens int8 (K,3S), device
        alg = FusedBilinearMatmul.from_archive(arch, n, m=None, p=None, index=None)
        C = alg(A, B, out=None, pad=False)                        # A (...,P,Q) @ B (...,Q,T), bfloat16 or float16
        alg.n, alg.m, alg.p, alg.S, alg.rank, alg.products        # products = rank

    m and p default to n, S to the width of ``tokens``.  Construction proves the list (``ops.solution_canon`` against
    ``functional.matmul_target(1, n, m, p, S)``) and runs the canonical form; there is no way round the proof.  The result is
    float32.  There is no ``levels``: nothing is written between levels here that a second level could read, and a larger
    grid does that job in one (the 49-term list for <4,4,4> is two levels of Strassen)."""
    _fn = "FusedBilinearMatmul"

    def __init__(self, tokens: torch.Tensor, rank: int, n: int, m: Optional[int] = None, p: Optional[int] = None,
                 S: Optional[int] = None, shift: int = 1):
        """``tokens`` int8 (K,3S) on a ROCm device, of which the first ``rank`` rows are the list.  Raises TensorGameError
        unless the list is proven against <n,m,p> in that cube.  One host sync (the proof's verdict)."""
        fn = self._fn
        _need_device(fn, tokens, "tokens")
        self.n, self.shift = int(n), int(shift)
        self.m, self.p = self.n if m is None else int(m), self.n if p is None else int(p)
        if min(self.n, self.m, self.p) < 1:
            raise TensorGameError(fn, -1, f"n={self.n}, m={self.m}, p={self.p}: every dimension must be at least 1")
        need = max(self.n * self.m, self.m * self.p, self.n * self.p)
        if tokens.dtype != torch.int8 or tokens.dim() != 2 or tokens.shape[1] % 3:
            raise TensorGameError(fn, -1, f"tokens must be int8 (K,3S), got {tokens.dtype} {tuple(tokens.shape)}")
        self.S = tokens.shape[1] // 3 if S is None else int(S)
        if not need <= self.S <= TG_MAX_S:
            raise TensorGameError(fn, -1, f"S={self.S} outside [max(n*m, m*p, n*p)={need},{TG_MAX_S}] for "
                                          f"<{self.n},{self.m},{self.p}>")
        if tokens.shape[1] != 3 * self.S:
            raise TensorGameError(fn, -1, f"tokens must be int8 (K,{3 * self.S}) for S={self.S}, got "
                                          f"{tuple(tokens.shape)}")
        target = functional.matmul_target(1, self.n, self.m, self.p, self.S, device=tokens.device)
        self._prove(tokens, rank, target, f"<{self.n},{self.m},{self.p}> at S={self.S}")

    @classmethod
    def from_archive(cls, arch, n: int, m: Optional[int] = None, p: Optional[int] = None,
                     index: Optional[int] = None) -> "FusedBilinearMatmul":
        """The algorithm of entry ``index`` of a ``SolutionArchive`` of cube size arch.S (None: the entry of lowest rank,
        the first of equals).  The entry is proven again, against <n,m,p>.  Synchronises (``entries``)."""
        tokens, rank = cls._entry("FusedBilinearMatmul.from_archive", arch, index)
        return cls(tokens, rank, n, m, p, S=arch.S, shift=arch.shift)

    @property
    def products(self) -> int:
        """Block products of one call: the rank, where the schoolbook method takes n*m*p."""
        return self.rank

    def __call__(self, A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None,
                 pad: bool = False) -> torch.Tensor:
        """A (...,P,Q) times B (...,Q,T), both bfloat16 or both float16 on the list's device, equal leading dimensions;
        returns float32 (...,P,T).  P must be a multiple of n, Q of m and T of p, or ``pad`` zero-pads them up (with
        torch) and slices the result.  ``out`` (...,P,T) may be float32 (the decode writes into it where it can) or of
        the operands' dtype (filled by ``copy_``, one more rounding); it may not overlap A or B.  No host sync;
        capturable on one stream."""
        fn = self._fn
        for t, name in ((A, "A"), (B, "B")):
            _need_device(fn, t, name)
            if t.device != self.device:
                raise TensorGameError(fn, -1, f"{name} is on {t.device}, the list on {self.device}")
            if t.dim() < 2:
                raise TensorGameError(fn, -1, f"{name} must have at least two dimensions, got {tuple(t.shape)}")
        if A.dtype != B.dtype:
            raise TensorGameError(fn, -1, f"mixed dtypes: A is {A.dtype}, B is {B.dtype}")
        if A.dtype not in (torch.bfloat16, torch.float16):
            raise TensorGameError(fn, -1, f"A and B must be bfloat16 or float16, got {A.dtype}")
        lead, (P, Q), (Q2, T) = tuple(A.shape[:-2]), A.shape[-2:], B.shape[-2:]
        if tuple(B.shape[:-2]) != lead or Q2 != Q:
            raise TensorGameError(fn, -1, f"A {tuple(A.shape)} and B {tuple(B.shape)} do not multiply: equal leading "
                                          "dimensions and Q are required")
        if out is not None:
            if out.dtype not in (torch.float32, A.dtype) or tuple(out.shape) != (*lead, P, T) or out.device != A.device:
                raise TensorGameError(fn, -1, f"out must be torch.float32 or {A.dtype} {(*lead, P, T)} on {A.device}, got "
                                              f"{out.dtype} {tuple(out.shape)} on {out.device}")
            for t, name in ((A, "A"), (B, "B")):
                if _overlap(out, t):
                    raise TensorGameError(fn, -1, f"out overlaps {name}: in-place operation is not supported")
        sizes = {"P": (P, self.n, "n"), "Q": (Q, self.m, "m"), "T": (T, self.p, "p")}
        up = {name: -size % d for name, (size, d, _) in sizes.items()}
        if any(up.values()) and not pad:
            name = next(k for k, v in up.items() if v)
            size, d, letter = sizes[name]
            raise TensorGameError(fn, -1, f"{name}={size} is no multiple of {letter}={d} (pad=True pads with zeros)")
        batch = math.prod(lead)
        a, b = A.reshape(batch, P, Q), B.reshape(batch, Q, T)
        if any(up.values()):
            a = torch.nn.functional.pad(a, (0, up["Q"], 0, up["P"]))
            b = torch.nn.functional.pad(b, (0, up["T"], 0, up["Q"]))
        a = a if a.stride(2) == 1 else a.contiguous()
        b = b if b.stride(2) == 1 else b.contiguous()
        m = ops.bilinear_products(a, b, self.tokens, self.rank, self.n, self.m, self.p, self.shift)
        direct = None                                   # the decode writes into a float32 `out` itself where it can
        if out is not None and out.dtype == torch.float32 and not any(up.values()) and out.stride(-1) == 1:
            try:
                direct = out.view(batch, P, T)
            except RuntimeError:
                pass
        c = ops.bilinear_rect_decode(m, self.tokens, self.rank, self.n, self.p, self.shift, out=direct)
        if direct is not None:
            return out
        c = c[:, :P, :T].reshape(*lead, P, T)
        if out is None:
            return c
        out.copy_(c)
        return out
