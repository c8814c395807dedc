"""Solve in random bases: ``BasisSet`` and ``solve_in_bases``.

In the AlphaTensor paper the change of basis is the main source of diversity when acting: every game is played on
T' = (A,B,C).T for a random unimodular (A,B,C), and a factorisation found there, T' = sum u' (x) v' (x) w', is carried
back as T = sum (A^-1 u') (x) (B^-1 v') (x) (C^-1 w'): a factorisation of the target in its own basis, usually another
one than a search there finds (not in the reference).  Everything stays on the device and is exact
integer arithmetic (include/tensor_game_bases.h):

    bases = BasisSet.sample(n=8, S=4, device="cuda:0", seed=3)           # basis 0 is the identity
    reb = solve_in_bases(policy, states, scalars, bases, n_samples=8, max_actions=12, slots=256)
    rep = arch.add_result(reb, states)          # proven against the ORIGINAL targets, deduplicated across the bases
    save_run(..., extra={"bases": bases.state_dict()}); bases = BasisSet.from_state_dict(sd, "cuda:0")

The lists that come back are int8 tokens, not vocabulary tokens (the inverse of a basis has entries beyond the factor
values): they are for ``SolutionArchive`` and ``ops.solution_canon``, not for the network.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import torch

from . import ops, rollout
from ._lib import TG_MAX_S, TensorGameError

__all__ = ["BasisSet", "RebasedSolutions", "solve_in_bases"]

STATE_VERSION = 1


class BasisSet:
    """``n`` matrix triples and their exact inverses on the device: ``forward`` int32 (n,3,S,S), ``inverse`` int32
    (n,3,S,S), ``bad`` uint8 (n,) (1: ``ops.basis_inverse`` refused the triple; its inverse is all zero and ``expand``
    does not use it).  With ``identity_first`` basis 0 is the identity, so the given basis is always among them."""

    def __init__(self, forward: torch.Tensor, inverse: torch.Tensor, bad: torch.Tensor, identity_first: bool):
        fn = "BasisSet"
        if not forward.is_cuda:
            raise TensorGameError(fn, -1, f"a ROCm device is required (got {forward.device}); there is no CPU path")
        if forward.dtype != torch.int32 or forward.dim() != 4 or forward.shape[0] < 1 or forward.shape[1] != 3 or \
                forward.shape[2] != forward.shape[3] or not 1 <= forward.shape[2] <= TG_MAX_S:
            raise TensorGameError(fn, -1, f"forward must be int32 (n,3,S,S) with n >= 1 and S in [1,{TG_MAX_S}], got "
                                          f"{forward.dtype} {tuple(forward.shape)}")
        n = forward.shape[0]
        if inverse.dtype != torch.int32 or inverse.shape != forward.shape or inverse.device != forward.device:
            raise TensorGameError(fn, -1, f"inverse must be int32 {tuple(forward.shape)} on {forward.device}, got "
                                          f"{inverse.dtype} {tuple(inverse.shape)} on {inverse.device}")
        if bad.dtype != torch.uint8 or tuple(bad.shape) != (n,) or bad.device != forward.device:
            raise TensorGameError(fn, -1, f"bad must be uint8 {(n,)} on {forward.device}, got {bad.dtype} "
                                          f"{tuple(bad.shape)} on {bad.device}")
        self.forward, self.inverse, self.bad = forward.contiguous(), inverse.contiguous(), bad.contiguous()
        self.n, self.S, self.device, self.identity_first = n, forward.shape[2], forward.device, bool(identity_first)

    @classmethod
    def sample(cls, n: int, S: int, device, seed: int = 0, probs=None, identity_first: bool = True) -> "BasisSet":
        """``n`` bases P = L @ U through ``ops.sample_basis(want_factors=True)`` (``probs``: its off-diagonal weights)
        and their inverses through ``ops.basis_inverse``.  With ``identity_first`` basis 0 is replaced by the
        identity.  No host sync."""
        if int(n) < 1:
            raise TensorGameError("BasisSet.sample", -1, f"n={n} < 1")
        P, L, U = ops.sample_basis(int(n), int(S), device, probs=probs, seed=seed, want_factors=True)
        inverse, bad = ops.basis_inverse(L, U)
        forward = P.to(torch.int32)
        if identity_first:
            eye = torch.eye(int(S), dtype=torch.int32, device=forward.device)
            forward[0], inverse[0], bad[0] = eye, eye, 0
        return cls(forward, inverse, bad, identity_first)

    def expand(self, states: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Every state in every basis.  states int8 (G,T,S,S,S) -> (moved int8 (G*n,T,S,S,S), basis_of_row int64
        (G*n,)): row e = g*n + j holds every frame of state g under basis j (``ops.change_basis``).  A row of which a
        frame left int8, or whose basis is bad, holds the UNTRANSFORMED state instead and has basis_of_row[e] = 0, the
        identity -- which is why this needs ``identity_first``.  Decided on the device; no host sync."""
        fn = "BasisSet.expand"
        if not self.identity_first:
            raise TensorGameError(fn, -1, "needs a set with identity_first: a row that cannot be moved falls back to "
                                          "basis 0, which has to be the identity")
        S, n = self.S, self.n
        if states.dtype != torch.int8 or states.dim() != 5 or tuple(states.shape[2:]) != (S, S, S):
            raise TensorGameError(fn, -1, f"states must be int8 (G,T,{S},{S},{S}), got {states.dtype} "
                                          f"{tuple(states.shape)}")
        if states.device != self.device:
            raise TensorGameError(fn, -1, f"states are on {states.device}, the bases on {self.device}")
        G, T = states.shape[0], states.shape[1]
        rows = states.repeat_interleave(n, dim=0).contiguous()                      # row g*n + j = state g
        j = torch.arange(n, device=self.device, dtype=torch.int64).repeat(G)      # its basis
        overflow = torch.zeros((G * n * T,), dtype=torch.uint8, device=self.device)
        moved = ops.change_basis(rows.view(G * n * T, S, S, S), self.forward[j].repeat_interleave(T, dim=0),
                                 overflow=overflow).view(G * n, T, S, S, S)
        fall = (overflow.view(G * n, T) != 0).any(dim=1) | (self.bad[j] != 0)
        return torch.where(fall[:, None, None, None, None], rows, moved), torch.where(fall, 0, j)

    def state_dict(self) -> dict:
        """Host tensors and plain scalars (loads with ``weights_only=True``)."""
        return {"version": STATE_VERSION, "n": self.n, "S": self.S, "identity_first": self.identity_first,
                "forward": self.forward.cpu(), "inverse": self.inverse.cpu(), "bad": self.bad.cpu()}

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda") -> "BasisSet":
        if sd.get("version") != STATE_VERSION:
            raise TensorGameError("BasisSet.from_state_dict", -1, f"version {sd.get('version')!r}, expected "
                                                                  f"{STATE_VERSION}")
        b = cls(sd["forward"].to(device), sd["inverse"].to(device), sd["bad"].to(device), sd["identity_first"])
        if (b.n, b.S) != (sd["n"], sd["S"]):
            raise TensorGameError("BasisSet.from_state_dict", -1, f"n={sd['n']}, S={sd['S']} and the stored matrices "
                                                                  f"{tuple(b.forward.shape)} do not fit together")
        return b


@dataclass
class RebasedSolutions:
    """What ``solve_in_bases`` found, carried back to the basis the states were given in (device tensors): ``groups``
    int64 (M,) indexes the ORIGINAL states, ``basis`` int64 (M,) is the basis the list was found in, ``tokens`` int8
    (M,max_actions,3S) and ``lengths`` int64 (M,) are the rebased lists, ``bad`` uint8 (M,) is 1 where a mapped token
    left int8 (that list is empty), ``shift`` the token shift and ``found`` the ``SolveResult`` of the search over the
    expanded states (its ``groups`` index the expanded rows g*n + j, its lists are in the moved bases).
    ``SolutionArchive.add_result`` takes it as it is."""

    groups: torch.Tensor
    basis: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    bad: torch.Tensor
    shift: int
    found: rollout.SolveResult


def solve_in_bases(policy, states: torch.Tensor, scalars: torch.Tensor, bases: BasisSet, n_samples: int,
                   max_actions: int, *, chunk_groups=None, slots=None, **kw) -> RebasedSolutions:
    """The solution search over every state in every basis of ``bases``: ``bases.expand(states)`` (the scalars
    repeated alongside), then ``rollout.solve_states`` (``chunk_groups`` given) or ``rollout.solve_stream`` (``slots``
    given) with the remaining keywords, then ``ops.solution_rebase`` of the found lists with ``bases.inverse``.  The
    policy sees G*n start states; expanded row g*n + j is state g in basis j, or untransformed where ``expand`` fell
    back.  No host sync beyond those of the search itself."""
    fn = "solve_in_bases"
    if (chunk_groups is None) == (slots is None):
        raise TensorGameError(fn, -1, "exactly one of chunk_groups (solve_states) and slots (solve_stream) must be given")
    moved, basis_of_row = bases.expand(states)
    if scalars.dim() != 2 or scalars.shape[0] != states.shape[0]:
        raise TensorGameError(fn, -1, f"scalars must be float32 ({states.shape[0]},dim_s), got {tuple(scalars.shape)}")
    scal = scalars.repeat_interleave(bases.n, dim=0).contiguous()
    if chunk_groups is not None:
        found = rollout.solve_states(policy, moved, scal, n_samples, max_actions, chunk_groups=chunk_groups, **kw)
    else:
        found = rollout.solve_stream(policy, moved, scal, n_samples, max_actions, slots=slots, **kw)
    shift = int(kw.get("shift", 1))
    basis = basis_of_row[found.groups]
    tokens, lengths, bad = ops.solution_rebase(found.tokens, found.lengths, bases.inverse, index=basis, shift=shift)
    return RebasedSolutions(torch.div(found.groups, bases.n, rounding_mode="floor"), basis, tokens, lengths, bad, shift,
                            found)
