"""``SymmetryGroup``: a finite set of symmetries of a target, for ``ops.orbit_canon`` and ``SolutionArchive(group=)``.

An element is a row of uint8 (3S+1) in the encoding of include/tensor_game_symmetry.h (``ops.symmetry_sample``,
``ops.symmetry_apply``): the code of a mode permutation and a signed index permutation per mode.  On the 3S factor values
of a term it is one signed permutation, f^g[i] = s[i] * f[p[i]] with i = m*S + a, p[i] = rho[m]*S + pi_m[a], and that is
how the host side here composes elements: (g then h) has p = p_g[p_h], s = s_h * s_g[p_h].

    grp = SymmetryGroup.matmul(2, "cuda:0")                 # the 1 536 symmetries of <2,2,2> that keep the vocabulary
    grp.order, grp.closed(), grp.fixes(targets)             # 1536, True, device bool (M,)
    small = grp.modulo_term_signs()                         # 384 rows: the same orbit form at a quarter of the work
    arch = SolutionArchive(S=4, max_rank=16, capacity=65536, device="cuda:0", group=small)

Generation, validation and closure run on the host in numpy, once; the rows then live on the device.  Nothing here finds
a target's symmetries: the caller names generators (``generate``) or takes the matrix-multiplication group (``matmul``),
and ``fixes`` checks the result against a target on the device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import TG_MAX_S, TG_ORBIT_MAX_G, TensorGameError

__all__ = ["SymmetryGroup"]

STATE_VERSION = 1
_RHO = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # code -> (rho[0], rho[1], rho[2])


def _encode(rho, pi, sign) -> np.ndarray:
    """One row from rho (3), pi (3,S) and sign (3,S) of +-1."""
    pi, sign = np.asarray(pi, np.int64), np.asarray(sign, np.int64)
    return np.concatenate([[_RHO.index(tuple(int(r) for r in rho))], (pi | np.where(sign < 0, 0x80, 0)).reshape(-1)]).astype(np.uint8)


def _flat(rows: np.ndarray, S: int):
    """(p, s) of validated rows (N,3S+1): the signed permutation of the 3S factor positions, int64 (N,3S) each."""
    rho = np.array(_RHO, np.int64)[rows[:, 0]]                                   # (N,3)
    p = np.repeat(rho, S, axis=1) * S + (rows[:, 1:] & 0x7F).astype(np.int64)
    s = np.where(rows[:, 1:] & 0x80, -1, 1).astype(np.int64)
    return p, s


def _rows(p: np.ndarray, s: np.ndarray, S: int) -> np.ndarray:
    """The rows of signed permutations (N,3S) that keep the three blocks together."""
    out = np.empty((p.shape[0], 3 * S + 1), np.uint8)
    rho = p[:, ::S] // S                                                          # (N,3)
    out[:, 0] = (rho[:, 0] * 2 + (rho[:, 1] > rho[:, 2])).astype(np.uint8)        # the lexicographic rank
    out[:, 1:] = ((p % S) | np.where(s < 0, 0x80, 0)).astype(np.uint8)
    return out


def _validate(sym, fn: str) -> np.ndarray:
    rows = np.ascontiguousarray(sym.cpu().numpy() if isinstance(sym, torch.Tensor) else sym)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 4 or (rows.shape[1] - 1) % 3:
        raise TensorGameError(fn, -1, f"sym must be uint8 (G,3S+1) with G >= 1, got {rows.dtype} {rows.shape}")
    S = (rows.shape[1] - 1) // 3
    if S > TG_MAX_S:
        raise TensorGameError(fn, -1, f"S={S} outside [1,{TG_MAX_S}]")
    if (rows[:, 0] > 5).any():
        raise TensorGameError(fn, -1, f"row {int(np.flatnonzero(rows[:, 0] > 5)[0])}: mode code above 5")
    idx = (rows[:, 1:] & 0x7F).reshape(-1, 3, S)
    if (idx >= S).any():
        raise TensorGameError(fn, -1, f"row {int(np.flatnonzero((idx >= S).any(axis=(1, 2)))[0])}: index >= S={S}")
    if (np.sort(idx, axis=2) != np.arange(S)).any():
        bad = int(np.flatnonzero((np.sort(idx, axis=2) != np.arange(S)).any(axis=(1, 2)))[0])
        raise TensorGameError(fn, -1, f"row {bad}: an index repeats: not a permutation")
    return rows


def _as_keys(rows: np.ndarray) -> np.ndarray:
    """Each row as one opaque value, so rows can be sorted and searched."""
    return np.ascontiguousarray(rows).view(np.dtype((np.void, rows.shape[1]))).reshape(-1)


class SymmetryGroup:
    """A set of group elements, validated: ``rows`` uint8 (G,3S+1) on the host, ``sym`` the same on ``device``.  Built by
    ``from_elements``, ``generate`` or ``matmul``; a set made by ``modulo_term_signs`` is a transversal, not a group, and
    carries ``overlap``: how many elements of its parent each row stands for."""

    def __init__(self, rows: np.ndarray, device, overlap: Optional[np.ndarray] = None):
        self.rows = rows
        self.S = (rows.shape[1] - 1) // 3
        self.device = None if device is None else torch.device(device)
        self.overlap = np.ones(rows.shape[0], np.int64) if overlap is None else np.asarray(overlap, np.int64)
        self._sym = None

    # ---- construction
    @classmethod
    def from_elements(cls, sym, device=None) -> "SymmetryGroup":
        """The set with exactly these rows (a uint8 (G,3S+1) tensor or array), in this order.  Validated on the host:
        every mode code at most 5, every index below S, every pi_m a permutation; at most TG_ORBIT_MAX_G rows."""
        rows = _validate(sym, "SymmetryGroup.from_elements")
        if rows.shape[0] > TG_ORBIT_MAX_G:
            raise TensorGameError("SymmetryGroup.from_elements", -1, f"G={rows.shape[0]} outside [1,{TG_ORBIT_MAX_G}]")
        if device is None and isinstance(sym, torch.Tensor):
            device = sym.device
        return cls(rows.copy(), device)

    @classmethod
    def generate(cls, generators, S: int, device=None, max_order: int = TG_ORBIT_MAX_G) -> "SymmetryGroup":
        """The group the generator rows (uint8 (N,3S+1), N >= 0) generate: closure by breadth-first composition from the
        identity, which is element 0; the order of the elements depends on the generators' order only.  A closure of
        more than ``max_order`` elements is refused (before it is complete)."""
        fn = "SymmetryGroup.generate"
        S = int(S)
        if not 1 <= S <= TG_MAX_S:
            raise TensorGameError(fn, -1, f"S={S} outside [1,{TG_MAX_S}]")
        ident = _encode((0, 1, 2), np.tile(np.arange(S), (3, 1)), np.ones((3, S)))[None]
        gens = np.asarray(generators.cpu().numpy() if isinstance(generators, torch.Tensor) else generators, np.uint8)
        gens = gens.reshape(-1, 3 * S + 1)
        if gens.shape[0]:
            gp, gs = _flat(_validate(gens, fn), S)
        found = {ident[0].tobytes()}
        layers, frontier = [ident], ident
        total = 1
        while frontier.shape[0] and gens.shape[0]:
            fp, fs = _flat(frontier, S)
            fresh = []
            for k in range(gens.shape[0]):                     # the frontier's elements, then generator k
                cand = _rows(fp[:, gp[k]], gs[k][None] * fs[:, gp[k]], S)
                for row in cand:
                    b = row.tobytes()
                    if b not in found:
                        found.add(b)
                        fresh.append(row)
            total += len(fresh)
            if total > max_order:
                raise TensorGameError(fn, -1, f"the closure has more than max_order={max_order} elements")
            frontier = np.stack(fresh) if fresh else np.empty((0, 3 * S + 1), np.uint8)
            if fresh:
                layers.append(frontier)
        return cls(np.concatenate(layers), device)

    @classmethod
    def matmul(cls, n: int, device=None, signs: bool = True) -> "SymmetryGroup":
        """The symmetries of the matrix-multiplication tensor <n,n,n> (T[i*n+j, j*n+k, i*n+k] = 1, S = n*n) that keep the
        vocabulary.  Generated by the two mode elements rho = (0,2,1) with (tr, id, id) and rho = (1,0,2) with
        (tr, tr, tr), tr: p*n+q -> q*n+p, and by the sandwich elements A -> P A Q^-1, B -> Q B R^-1, C -> P C R^-1 for
        P, Q, R adjacent transpositions and, with ``signs``, single sign flips: pi_0[i*n+j] = P(i)*n+Q(j),
        pi_1[j*n+k] = Q(j)*n+R(k), pi_2[i*n+k] = P(i)*n+R(k), signs a_i*b_j, b_j*c_k, a_i*c_k.  Orders: 48 (n=2 without
        signs), 1 536 (n=2), 1 296 (n=3 without signs); n=3 with signs (331 776) is above TG_ORBIT_MAX_G and refused."""
        n = int(n)
        S = n * n
        if n < 1 or S > TG_MAX_S:
            raise TensorGameError("SymmetryGroup.matmul", -1, f"n={n}: S=n*n outside [1,{TG_MAX_S}]")
        ar = np.arange(n)
        ident, tr, one = np.arange(S), (ar[None, :] * n + ar[:, None]).reshape(-1), np.ones((3, S), np.int64)
        gens = [_encode((0, 2, 1), [tr, ident, ident], one), _encode((1, 0, 2), [tr, tr, tr], one)]

        def sandwich(P, Q, R, a, b, c):
            pi = [(P[:, None] * n + Q[None, :]).reshape(-1), (Q[:, None] * n + R[None, :]).reshape(-1),
                  (P[:, None] * n + R[None, :]).reshape(-1)]
            sg = [np.outer(a, b).reshape(-1), np.outer(b, c).reshape(-1), np.outer(a, c).reshape(-1)]
            return _encode((0, 1, 2), pi, sg)

        plus = np.ones(n, np.int64)
        for which in range(3):
            for i in range(n - 1):
                perm = [ar.copy(), ar.copy(), ar.copy()]
                perm[which][[i, i + 1]] = [i + 1, i]
                gens.append(sandwich(*perm, plus, plus, plus))
            for i in range(n if signs else 0):
                sg = [plus.copy(), plus.copy(), plus.copy()]
                sg[which][i] = -1
                gens.append(sandwich(ar, ar, ar, *sg))
        return cls.generate(np.stack(gens), S, device)

    @classmethod
    def matmul_rect(cls, n: int, m: int, p: int, S: Optional[int] = None, device=None, signs: bool = True) -> "SymmetryGroup":
        """The symmetries of the rectangular tensor <n,m,p> in a cube of size S (include/tensor_game_rect.h:
        T[i*m+j, j*p+k, i*p+k] = 1, S >= max(n*m, m*p, n*p), the default) that keep the vocabulary.  The sandwich elements
        are those of ``matmul`` with P in S_n, Q in S_m, R in S_p: pi_0[i*m+j] = P(i)*m+Q(j), pi_1[j*p+k] = Q(j)*p+R(k),
        pi_2[i*p+k] = P(i)*p+R(k), signs a_i*b_j, b_j*c_k, a_i*c_k.  A mode element exists only where two dimensions agree:
        n == m: rho = (0,2,1) with (tr, id, id); n == p: rho = (1,0,2) with (tr, tr, tr); m == p: rho = (2,1,0) with
        (id, tr, id), tr the transpose of the mode's own r x c grid, x*c+y -> y*r+x.  A padding index (at or beyond its
        mode's size) maps to itself with sign +1.  Without signs the order is n! m! p! times the number of permutations
        of the triple (n,m,p) that leave it unchanged: 1 296 at (3,3,3), which is ``matmul(3, signs=False)``, 48 at
        (2,2,3), 12 at (2,3,1); with signs (2,2,3) has 3 072 elements, above TG_ORBIT_MAX_G, and is refused."""
        fn = "SymmetryGroup.matmul_rect"
        n, m, p = int(n), int(m), int(p)
        if min(n, m, p) < 1:
            raise TensorGameError(fn, -1, f"n={n}, m={m}, p={p}: every dimension must be at least 1")
        need = max(n * m, m * p, n * p)
        S = need if S is None else int(S)
        if not need <= S <= TG_MAX_S:
            raise TensorGameError(fn, -1, f"S={S} outside [max(n*m, m*p, n*p)={need},{TG_MAX_S}]")
        grids = [(n, m), (m, p), (n, p)]                                   # mode d is an r x c grid

        def padded(part, fill):
            """(3,S) from the three modes' own entries, ``fill`` (None: the index itself) on the padding."""
            out = np.tile(np.arange(S), (3, 1)) if fill is None else np.full((3, S), fill, np.int64)
            for d in range(3):
                out[d, :part[d].shape[0]] = part[d]
            return out

        def tr(d):
            r, c = grids[d]
            return (np.arange(c)[None, :] * r + np.arange(r)[:, None]).reshape(-1)   # x*c+y -> y*r+x

        ident = [np.arange(r * c) for r, c in grids]
        one = np.ones((3, S), np.int64)
        gens = []
        if n == m:
            gens.append(_encode((0, 2, 1), padded([tr(0), ident[1], ident[2]], None), one))
        if n == p:
            gens.append(_encode((1, 0, 2), padded([tr(0), tr(1), tr(2)], None), one))
        if m == p:
            gens.append(_encode((2, 1, 0), padded([ident[0], tr(1), ident[2]], None), one))

        def sandwich(P, Q, R, a, b, c):
            pi = [(P[:, None] * m + Q[None, :]).reshape(-1), (Q[:, None] * p + R[None, :]).reshape(-1),
                  (P[:, None] * p + R[None, :]).reshape(-1)]
            sg = [np.outer(a, b).reshape(-1), np.outer(b, c).reshape(-1), np.outer(a, c).reshape(-1)]
            return _encode((0, 1, 2), padded(pi, None), padded(sg, 1))

        dims = (n, m, p)
        for which in range(3):
            for i in range(dims[which] - 1):
                perm = [np.arange(d) for d in dims]
                perm[which][[i, i + 1]] = [i + 1, i]
                gens.append(sandwich(*perm, *[np.ones(d, np.int64) for d in dims]))
            for i in range(dims[which] if signs else 0):
                sg = [np.ones(d, np.int64) for d in dims]
                sg[which][i] = -1
                gens.append(sandwich(*[np.arange(d) for d in dims], *sg))
        gens = np.stack(gens) if gens else np.empty((0, 3 * S + 1), np.uint8)
        return cls.generate(gens, S, device)

    # ---- the set
    @property
    def order(self) -> int:
        return int(self.rows.shape[0])

    @property
    def sym(self) -> torch.Tensor:
        """The rows on the device: uint8 (G,3S+1), usable with ``ops.symmetry_apply`` and the orbit entries."""
        if self._sym is None:
            if self.device is None:
                raise TensorGameError("SymmetryGroup.sym", -1, "the group was made without a device")
            self._sym = torch.from_numpy(self.rows).to(self.device)
        return self._sym

    def closed(self) -> bool:
        """Whether the composition of any two elements is an element (for a finite set: whether it is a group)."""
        keys = np.sort(_as_keys(self.rows))
        p, s = _flat(self.rows, self.S)
        for k in range(self.order):
            prod = _as_keys(_rows(p[:, p[k]], s[k][None] * s[:, p[k]], self.S))
            at = np.minimum(np.searchsorted(keys, prod), keys.shape[0] - 1)
            if (keys[at] != prod).any():
                return False
        return True

    def fixes(self, targets: torch.Tensor) -> torch.Tensor:
        """Device bool (M,): every element maps targets[m] (int8 (M,S,S,S)) to itself (``ops.orbit_fixes``)."""
        return ops.orbit_fixes(targets, self.sym).to(torch.bool)

    def modulo_term_signs(self) -> "SymmetryGroup":
        """A transversal modulo the four elements (e0, e1, e2) that multiply mode m by a constant sign e_m with
        e0*e1*e2 = +1.  Such an element changes no term after sign normalisation, so g and g*(e0,e1,e2) give the same
        canonical form: the first element of every class (in this set's order) gives the same canon, rank and key at a
        fraction of the work, and ``stab`` counts classes; ``overlap`` holds each class's size in this set (4 for every
        class of ``matmul(2)``: its stab is a quarter of the full group's).  ``which`` indexes the transversal."""
        S = self.S
        p, s = _flat(self.rows, S)
        eps = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.int64)
        variants = np.stack([_as_keys(_rows(p, s * np.repeat(e, S)[None], S)) for e in eps])   # (4,G)
        klass = np.sort(variants, axis=0)[0]                                                    # the class's smallest row
        _, first, inverse, counts = np.unique(klass, return_index=True, return_inverse=True, return_counts=True)
        pick = np.sort(first)
        return SymmetryGroup(self.rows[pick].copy(), self.device, counts[inverse.reshape(-1)[pick]])

    # ---- persistence
    def state_dict(self) -> dict:
        """Host tensors and plain scalars (loads with ``weights_only=True``)."""
        return {"version": STATE_VERSION, "S": self.S, "sym": torch.from_numpy(self.rows.copy()),
                "overlap": torch.from_numpy(self.overlap.copy())}

    @classmethod
    def from_state_dict(cls, sd: dict, device=None) -> "SymmetryGroup":
        if sd.get("version") != STATE_VERSION:
            raise TensorGameError("SymmetryGroup.from_state_dict", -1, f"version {sd.get('version')!r}, expected "
                                                                       f"{STATE_VERSION}")
        g = cls.from_elements(sd["sym"].cpu(), device)
        if g.S != int(sd["S"]) or tuple(sd["overlap"].shape) != (g.order,):
            raise TensorGameError("SymmetryGroup.from_state_dict", -1, "S, sym and overlap do not fit together")
        g.overlap = sd["overlap"].cpu().numpy().astype(np.int64)
        return g
