"""``SolutionArchive``: the distinct proven factorisations a run has found, resident in HBM.

The solution search (``sample_rollouts``, ``solve_states``, ``solve_stream``) ends with action lists that replayed a
start state to zero in int8 arithmetic, which wraps: a list can be reported although it is no factorisation, the same
factorisation comes back written in many ways (term order, signs inside a term, null actions, a term and later its
negative), and it comes back again and again across samples, chunks, epochs and resumed runs.  The reference only
counts (``num_solutions_found``, training.py:346).  The archive runs every list through ``ops.solution_canon``
(include/tensor_game_solutions.h: exact verification, canonical form, effective rank, 64-bit key) and appends what is
proven and new to a device-resident store, with no host round trip:

    arch = SolutionArchive(S=4, max_rank=16, capacity=65536, device="cuda:0")
    rep = arch.add_result(res, states)                    # res: a RolloutResult / SolveResult of these start states
    rep.proven, rep.rank, rep.key, rep.fresh              # device tensors (M,)
    arch.count, arch.lowest_rank                          # 0-d device tensors
    tokens, rank, key, target_key = arch.entries()        # the first host sync
    save_run(..., extra={"solutions": arch.state_dict()}); arch2 = SolutionArchive.from_state_dict(sd, "cuda:0")

With ``group=`` (a ``SymmetryGroup`` whose elements fix the targets) the archive goes through ``ops.orbit_canon``
instead (include/tensor_game_orbits.h): the stored form and its key are the smallest canonical form over the group, so a
factorisation and its images under the target's symmetries are ONE entry, and ``count`` counts inequivalent algorithms:

    arch = SolutionArchive(S=4, max_rank=16, capacity=65536, device="cuda:0", group=SymmetryGroup.matmul(2, "cuda:0"))

Not factored out: rescalings between the factors of a term, and symmetries of the target outside the group the caller
supplied (without a group: none of the target's symmetries), so two entries can still be the same factorisation up to
those.  Archives of several GPUs are not merged.  The archive itself does not improve an entry; ``reduce_archive``
(mat_mul_amd/flips.py) walks the flip graph from every entry and adds what got shorter through ``add``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import ops
from ._lib import TG_MAX_S, TG_SOL_MAX_K, TensorGameError
from .orbits import SymmetryGroup

__all__ = ["SolutionArchive", "AddReport"]

STATE_VERSION = 1        # an archive without a group
STATE_VERSION_GROUP = 2  # ... with one: version 1 plus the group's state


@dataclass
class AddReport:
    """What one ``SolutionArchive.add`` found, per row of the batch (device tensors (M,)): ``proven`` bool -- the list
    sums to its target exactly; ``rank`` int32 -- the terms of its canonical form; ``key`` int64 (the 64 bits) -- the
    key of that form; ``fresh`` bool -- this call stored the row; ``residual_nnz`` int32 -- the non-zero entries of
    target - sum (-1: a bad row, see ``SolutionArchive.canon_status``).  Of an archive with a group, also: ``fixed``
    bool -- every element of the group fixes the row's target (a row is stored only then); ``which`` int32 -- the
    smallest index of a group element that maps the list to the stored form (-1: a bad row); ``stab`` int32 -- how many
    elements do.  None without a group."""

    proven: torch.Tensor
    rank: torch.Tensor
    key: torch.Tensor
    fresh: torch.Tensor
    residual_nnz: torch.Tensor
    fixed: Optional[torch.Tensor] = None
    which: Optional[torch.Tensor] = None
    stab: Optional[torch.Tensor] = None


class SolutionArchive:
    def __init__(self, S: int, max_rank: int, capacity: int, device="cuda", shift: int = 1,
                 group: Optional[SymmetryGroup] = None):
        """Room for ``capacity`` factorisations of at most ``max_rank`` terms of (S,S,S) targets.  ``count`` and
        ``lowest_rank`` (``max_rank + 1`` while the archive is empty) are 0-d device tensors; ``status`` int32 (1,):
        bit 0 is set once a new factorisation found no room; ``canon_status`` uint32 (1,): the bad-row bits of
        ``ops.solution_canon`` (of ``ops.orbit_canon`` with a ``group``: the archive then stores the form modulo that
        group, for the rows whose target it fixes)."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TensorGameError("SolutionArchive", -1, f"a ROCm device is required (got {self.device}); there is no "
                                                         "CPU path")
        self.S, self.max_rank, self.capacity, self.shift = int(S), int(max_rank), int(capacity), int(shift)
        if not 1 <= self.S <= TG_MAX_S:
            raise TensorGameError("SolutionArchive", -1, f"S={S} outside [1,{TG_MAX_S}]")
        if not 1 <= self.max_rank <= TG_SOL_MAX_K:
            raise TensorGameError("SolutionArchive", -1, f"max_rank={max_rank} outside [1,{TG_SOL_MAX_K}]")
        if self.capacity < 1:
            raise TensorGameError("SolutionArchive", -1, f"capacity={capacity} < 1")
        ops.solution_check(0, self.max_rank, self.S, self.shift)
        self.group = group
        if group is not None:
            if group.S != self.S:
                raise TensorGameError("SolutionArchive", -1, f"the group is of S={group.S}, the archive of S={self.S}")
            ops.orbit_check(0, self.max_rank, self.S, self.shift, group.order)
            self._sym = group.sym.to(self.device)
        dev, cap = self.device, self.capacity
        # row `capacity` of every store is the sink of the rows that are not stored: one scatter serves all rows
        self._tokens = torch.zeros((cap + 1, self.max_rank, 3 * self.S), dtype=torch.int8, device=dev)
        self._rank = torch.zeros((cap + 1,), dtype=torch.int32, device=dev)
        self._key = torch.zeros((cap + 1,), dtype=torch.int64, device=dev)
        self._target_key = torch.zeros((cap + 1,), dtype=torch.int64, device=dev)
        self.table = ops.alloc_seen_table(1 << max(1, (2 * cap - 1).bit_length()), dev)  # a power of two >= 2 * capacity
        self.table_status = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.canon_status = torch.zeros((1,), dtype=torch.uint32, device=dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.count = torch.zeros((), dtype=torch.int64, device=dev)
        self.lowest_rank = torch.full((), self.max_rank + 1, dtype=torch.int32, device=dev)

    def add(self, targets: torch.Tensor, tokens: torch.Tensor, lengths: torch.Tensor) -> AddReport:
        """Verify, canonicalise and store what is new.  targets int8 (M,S,S,S): the start heads; tokens int8
        (M,K,3S) and lengths int64 (M,) as ``solutions()`` returns them.  In this order: ``ops.solution_canon`` (with a
        group: ``ops.orbit_canon`` and ``ops.orbit_fixes``); a row is valid when its residual is zero and its rank is at
        most ``max_rank`` (and the group fixes its target: only then is the stored form a factorisation of that target);
        among valid rows with equal key only
        the lowest batch index stays (a stable sort of the keys and a neighbour compare); ``ops.seen(insert=True)`` on
        the archive's own table tells which of those keys are new; the new rows are appended in batch order at
        ``count`` + the exclusive prefix sum of the new flags, and a row that would land at or beyond ``capacity`` is
        dropped and sets bit 0 of ``status``.  No host sync."""
        if targets is None:
            raise TensorGameError("SolutionArchive.add", -1, "targets must be given: nothing is stored unproven")
        fixed = which = stab = None
        if self.group is None:
            canon, rank, key, res = ops.solution_canon(targets, tokens, lengths, shift=self.shift, status=self.canon_status)
        else:
            canon, rank, key, res, which, stab = ops.orbit_canon(targets, tokens, lengths, self._sym, shift=self.shift,
                                                                 status=self.canon_status)
        M, K = canon.shape[0], canon.shape[1]
        if canon.shape[2] != 3 * self.S:
            raise TensorGameError("SolutionArchive.add", -1, f"tokens are of S={canon.shape[2] // 3}, the archive of "
                                                             f"S={self.S}")
        proven = res == 0
        if M == 0:
            return AddReport(proven, rank, key, proven.clone(), res, None if self.group is None else proven.clone(), which,
                             stab)
        valid = proven & (rank <= self.max_rank)
        if self.group is not None:
            fixed = ops.orbit_fixes(targets, self._sym).to(torch.bool)
            valid &= fixed
        # valid rows first, then by key, both stable: the first row of a run of equal keys is its lowest valid row
        by_valid = torch.sort((~valid).to(torch.uint8), stable=True).indices
        sorted_key, by_key = torch.sort(key[by_valid], stable=True)
        order = by_valid[by_key]
        first = torch.ones_like(valid)
        first[1:] = sorted_key[1:] != sorted_key[:-1]
        mask = torch.zeros((M,), dtype=torch.uint8, device=self.device)
        mask[order] = (first & valid[order]).to(torch.uint8)
        new = ops.seen(key, self.table, mask=mask, insert=True, status=self.table_status).to(torch.int64)
        at = self.count + torch.cumsum(new, 0) - new
        fresh = (new != 0) & (at < self.capacity)
        at = torch.where(fresh, at, self.capacity)
        R = min(K, self.max_rank)  # (a valid row has no term beyond max_rank; the store is zero beyond K)
        self._tokens[:, :R].index_copy_(0, at, canon[:, :R])
        self._rank.index_copy_(0, at, rank)
        self._key.index_copy_(0, at, key)
        self._target_key.index_copy_(0, at, ops.state_hash(targets if targets.is_contiguous() else targets.contiguous()))
        self.status |= ((new != 0) & ~fresh).any().to(torch.int32)
        self.count += fresh.sum()
        self.lowest_rank.copy_(torch.minimum(self.lowest_rank,
                                             torch.where(fresh, rank, self.max_rank + 1).min().to(torch.int32)))
        return AddReport(proven, rank, key, fresh, res, fixed, which, stab)

    def add_result(self, res, states: torch.Tensor) -> AddReport:
        """``add`` for a ``RolloutResult`` (its ``solutions()``) or a ``SolveResult`` and the start states int8
        (G,T,S,S,S) the search ran on: the target of a solution is the newest frame of its group's start state."""
        if hasattr(res, "solutions"):
            groups, tokens, lengths = res.solutions()
        else:
            groups, tokens, lengths = res.groups, res.tokens, res.lengths
        if getattr(res, "shift", self.shift) != self.shift:
            raise TensorGameError("SolutionArchive.add_result", -1, f"the rollout ran with shift={res.shift}, the "
                                                                    f"archive with shift={self.shift}")
        if states.dim() != 5:
            raise TensorGameError("SolutionArchive.add_result", -1, f"states must be int8 (G,T,S,S,S), got "
                                                                    f"{tuple(states.shape)}")
        return self.add(states[groups, 0].contiguous(), tokens, lengths)

    def entries(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The stored factorisations in the order they were found (synchronises): tokens int8 (n,max_rank,3S) -- the
        canonical terms, zero rows behind them -- rank int32 (n,), key int64 (n,), target_key int64 (n,) =
        ``ops.state_hash`` of the target."""
        n = int(self.count)
        return self._tokens[:n], self._rank[:n], self._key[:n], self._target_key[:n]

    def state_dict(self) -> dict:
        """Host tensors and plain scalars (loads with ``weights_only=True``): the stored entries, the count and the
        configuration.  Version 1 without a group; version 2 = version 1 plus ``group``: the group's own state."""
        tokens, rank, key, target_key = self.entries()
        extra = {} if self.group is None else {"group": self.group.state_dict()}
        return {"version": STATE_VERSION_GROUP if extra else STATE_VERSION, **extra, "S": self.S, "max_rank": self.max_rank, "capacity": self.capacity,
                "shift": self.shift, "count": int(rank.shape[0]), "status": int(self.status.item()),
                "lowest_rank": int(self.lowest_rank.item()), "tokens": tokens.cpu(), "rank": rank.cpu(), "key": key.cpu(),
                "target_key": target_key.cpu()}

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda") -> "SolutionArchive":
        """The archive ``state_dict`` described, on ``device``: the entries are copied back and the table is rebuilt
        by inserting their keys, so every later ``add`` is answered as the original would have answered it."""
        if sd.get("version") not in (STATE_VERSION, STATE_VERSION_GROUP):
            raise TensorGameError("SolutionArchive.from_state_dict", -1, f"version {sd.get('version')!r}, expected "
                                                                         f"{STATE_VERSION} or {STATE_VERSION_GROUP}")
        group = SymmetryGroup.from_state_dict(sd["group"], device) if sd["version"] == STATE_VERSION_GROUP else None
        a = cls(sd["S"], sd["max_rank"], sd["capacity"], device, sd["shift"], group)
        n = int(sd["count"])
        shapes = {"tokens": (n, a.max_rank, 3 * a.S), "rank": (n,), "key": (n,), "target_key": (n,)}
        if n > a.capacity or any(tuple(sd[k].shape) != s for k, s in shapes.items()):
            raise TensorGameError("SolutionArchive.from_state_dict", -1, f"count={n} and the stored entries do not fit "
                                                                         f"together (capacity {a.capacity})")
        for store, name in ((a._tokens, "tokens"), (a._rank, "rank"), (a._key, "key"), (a._target_key, "target_key")):
            store[:n].copy_(sd[name])
        if n:
            ops.seen(a._key[:n].contiguous(), a.table, insert=True, status=a.table_status)
        a.count.fill_(n)
        a.status.fill_(int(sd["status"]))
        a.lowest_rank.fill_(int(sd["lowest_rank"]))
        return a
