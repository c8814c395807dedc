"""The sign lift: Z_2 flip-graph results turned into integer factorisations with coefficients in {-1, 0, 1}.

The walks over Z_2 (``flips_mod2``) are the ones that get anywhere, but what they reach is right mod 2 only.  The sign
lift keeps a Z_2 list's support and looks for signs on it (include/tensor_game_lift.h): one unknown per support position
says whether the coefficient there is -1; one linear system over Z_2 makes the list right mod 4; every solution of that
system is a concrete +-1 candidate, and each candidate is checked exactly over the integers, ``tries`` of them per list
(the free variables zero first, then drawn from Philox).  The elimination and the tries run on the device, a workgroup
per list:

    res = lift_signs(walks.best, walks.best_rank, int_targets, tries=32)   # LiftResult of device tensors, no host sync
    res.lifted, res.tokens, res.lengths                                    # status == 0; int8 (W,K,3S); int64 (W,)
    res = walks.lift(int_targets)                                          # the same from a Mod2Walks (list0 = walk0)
    rep, mod2, res = reduce_archive_lifted(arch, n_steps=100_000)          # walk over Z_2, lift, arch.add: proven there

Nothing enters a ``SolutionArchive`` on the lift's word: ``arch.add`` proves every lifted list again by itself.

Not done here: lifting beyond +-1 coefficients (a list whose only integer lifts need a 2 somewhere comes back with
status 3), a Z_2 archive, choosing the entries to walk adaptively.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import ops
from ._lib import TG_LIFT2_MAX_WS_LISTS, TensorGameError
from .flips_mod2 import Mod2Result, reduce_mod2

__all__ = ["LiftResult", "lift_signs", "reduce_archive_lifted"]

MAX_WORKSPACE_BYTES = 1 << 30
_RESIDENT_LISTS = 2048   # workgroups a device holds at once, generously: more workspace slices than that are never used


class LiftResult(NamedTuple):
    """What ``lift_signs`` found, per list (device tensors).  ``tokens`` int8 (W,K,3S): the lifted list as token rows
    ({-1,0,1} + shift), all-zero where ``status`` != 0; ``lengths`` int64 (W,): ranks where status is 0, else 0;
    ``status`` int32: 0 lifted and exact, 1 the list is not right mod 2, 2 the sign system has no solution, 3 no try was
    exact, -1 a rank outside [0,K]; ``try_used`` int32: the first exact try (-1: none); ``unknowns``, ``sys_rank`` int32:
    the columns of the system and its rank; ``miss`` int32: the non-zero cells of the best try (0 when lifted; the odd
    cells for status 1; -1 for status 2 and -1)."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    status: torch.Tensor
    try_used: torch.Tensor
    unknowns: torch.Tensor
    sys_rank: torch.Tensor
    miss: torch.Tensor

    @property
    def lifted(self) -> torch.Tensor:
        """bool (W,): status == 0."""
        return self.status == 0


def lift_signs(lists: torch.Tensor, ranks: torch.Tensor, targets: torch.Tensor, tries: int = 32, seed: int = 0,
               shift: int = 1, list0: int = 0, max_workspace_bytes: int = MAX_WORKSPACE_BYTES,
               ws_lists: Optional[int] = None) -> LiftResult:
    """The sign lift of W lists over Z_2 (``lists`` int32 (W,K,3), ``ranks`` int32 (W,)) against their INTEGER
    ``targets`` int8 (W,S,S,S): ``ops.lift2_signs``, one launch.  Where the system does not fit in LDS the workspace is
    allocated here, for as many lists at a time as stay under ``max_workspace_bytes`` (at least one; ``ws_lists``
    overrides the choice).  List w has the global id ``list0 + w``: its tries depend on (seed, id) alone.  No host
    sync."""
    fn = "lift_signs"
    for t, name in ((lists, "lists"), (ranks, "ranks"), (targets, "targets")):
        if not t.is_cuda:
            raise TensorGameError(fn, -1, f"{name} must live on a ROCm device (got {t.device}); there is no CPU path")
    if lists.dim() != 3 or targets.dim() != 4:
        raise TensorGameError(fn, -1, f"lists must be int32 (W,K,3) and targets int8 (W,S,S,S), got {tuple(lists.shape)} "
                                      f"and {tuple(targets.shape)}")
    W, K, S = lists.shape[0], lists.shape[1], targets.shape[1]
    ops.lift2_check(W, K, S, shift, tries, 1)
    per_list = ops.lift2_workspace_bytes(K, S)
    workspace = None
    if per_list and W:
        if ws_lists is None:
            ws_lists = max(1, min(W, int(max_workspace_bytes) // per_list, _RESIDENT_LISTS, TG_LIFT2_MAX_WS_LISTS))
        ops.lift2_check(W, K, S, shift, tries, ws_lists)
        workspace = torch.empty((int(ws_lists) * per_list,), dtype=torch.uint8, device=lists.device)
    elif ws_lists is None:
        ws_lists = 1
    ranks = ranks if ranks.dtype == torch.int32 else ranks.to(torch.int32)
    tokens, out = ops.lift2_signs(targets, lists.contiguous(), ranks.contiguous(), tries=tries, seed=seed, list0=list0,
                                  shift=shift, workspace=workspace, ws_lists=ws_lists)
    lengths = torch.where(out["status"] == 0, ranks, torch.zeros_like(ranks)).to(torch.int64)
    return LiftResult(tokens, lengths, out["status"], out["try_used"], out["unknowns"], out["sys_rank"], out["miss"])


def reduce_archive_lifted(arch, n_steps: int, walks_per_entry: int = 8, tries: int = 32, seed: int = 0, plus_after: int = 0,
                          plus_slack: int = 1) -> Optional[Tuple[object, Mod2Result, LiftResult]]:
    """``reduce_archive_mod2``, then the sign lift of every walk's best list against the INTEGER sum of the entry it
    started from (``flips.term_sum``), then ``arch.add`` of the lifted ones: the archive proves them itself
    (``tg_solution_canon``, or the orbit form), so nothing enters on the lift's word.  A list that did not lift is
    offered with length 0, which sums to its target only where that is zero.  Returns (the ``AddReport``, the
    ``Mod2Result``, the ``LiftResult``); None for an empty archive.  Synchronises (``entries``, ``term_sum``)."""
    tokens, rank, _, _ = arch.entries()
    if tokens.shape[0] == 0:
        return None
    tokens, lengths = tokens.contiguous(), rank.to(torch.int64)
    mod2 = reduce_mod2(tokens, lengths, n_steps, walks_per_list=walks_per_entry, shift=arch.shift, seed=seed,
                       plus_after=plus_after, plus_slack=plus_slack)
    walks = mod2.walks
    from .flips import term_sum
    targets = term_sum(tokens, lengths, arch.shift)[walks.src].contiguous()
    res = lift_signs(walks.best, walks.best_rank, targets, tries=tries, seed=seed, shift=arch.shift, list0=walks.walk0)
    rep = arch.add(targets, res.tokens, res.lengths)
    return rep, mod2, res
