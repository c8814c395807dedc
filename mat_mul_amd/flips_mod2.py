"""``Mod2Walks``: random walks on the flip graph over Z_2, the field with two elements.

The flip-graph results that matter were found over Z_2 and lifted to the integers afterwards.  Over Z_2 no flip is ever
refused (there is no coefficient bound to leave), the graph is far better connected than over the integers with bound 1,
and there are no signs and no normal form: a factor of S <= 32 values is one 32-bit mask, a term is three of them.  The
rules are those of include/tensor_game_flips_mod2.h: every walk is a wavefront's registers on the device, independent of
every other walk, and a function of (its list, seed, walk id, step) alone:

    walks = Mod2Walks.start(tokens, lengths, walks_per_list=8, seed=0)     # tokens int8 (M,K,3S), lengths int64 (M,)
    walks.advance(100_000)                                                 # launches of <= 65 536 steps, no host sync
    Mod2Walks.start(..., plus_after=10_000, plus_slack=1)                  # with plus transitions
    walks.best, walks.best_rank, walks.best_step, walks.state, walks.src   # device tensors; lists int32 (W,K,3)
    walks.tokens("best")                                                   # int8 (W,K,3S) of {0,1} + shift
    walks.residual(targets)                                                # the proof: 0 where best sums to targets mod 2
    res = reduce_mod2(tokens, lengths, n_steps=100_000)                    # (walks, residual, proven, best_rank per list)
    res = reduce_archive_mod2(arch, n_steps=100_000)                       # the same from an archive's entries
    save_run(..., extra={"mod2": walks.state_dict()}); Mod2Walks.from_state_dict(sd, "cuda:0").advance(n)  # bit for bit

    walks.lift(int_targets)                                                # mat_mul_amd.lift: the sign lift to {-1,0,1}

A list is reported as proven only through ``tg_flip2_residual``: the exact count of cells where the list's sum and the
target differ mod 2.  Z_2 lists do NOT enter ``SolutionArchive``: its proof is over the integers, and a list that is
right mod 2 need not be right there.  ``mat_mul_amd.lift`` lifts a Z_2 list to integer coefficients in {-1, 0, 1}
where such a lift exists and its system's solutions find it; what it lifts enters the archive through the archive's own
proof (``reduce_archive_lifted``).

Not done here: lifting beyond +-1 coefficients, an archive and a canonical form for Z_2 lists, choosing the entries to
walk adaptively.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops
from ._lib import TG_FLIP_MAX_STEPS, TensorGameError
from .flips import term_sum

__all__ = ["Mod2Walks", "Mod2Result", "reduce_mod2", "reduce_archive_mod2"]

STATE_VERSION = 1
_STATE = tuple(name for name, _ in ops._FLIP2_STATE)


class Mod2Walks:
    """W walks over Z_2 on the device.  ``cur``, ``best`` int32 (W,K,3): rows of three masks, bit e of mask d the e-th
    value of the mode-d factor; ``cur_rank``, ``best_rank``, ``state`` (0 walking, 1 stuck, -1 bad), ``since`` int32 (W,);
    ``best_step``, ``flips``, ``pluses`` int64 (W,); ``src`` int64 (W,): the list each walk started from; ``status`` uint32
    (1,): the bad-row bits of ``ops.flip2_begin``; ``steps_done``: a host integer."""

    def __init__(self, st: dict, src: torch.Tensor, status: torch.Tensor, S: int, seed: int, walk0: int, steps_done: int = 0,
                 plus_after: int = 0, plus_slack: int = 1):
        self._st = st
        self.src, self.status = src, status
        self.S, self.seed, self.walk0 = int(S), int(seed), int(walk0)
        self.steps_done = int(steps_done)
        self.plus_after, self.plus_slack = int(plus_after), int(plus_slack)

    def __getattr__(self, name):
        if name in _STATE and "_st" in self.__dict__:
            return self.__dict__["_st"][name]
        raise AttributeError(name)

    @classmethod
    def start(cls, tokens: torch.Tensor, lengths: torch.Tensor, walks_per_list: int = 1, shift: int = 1, seed: int = 0,
              walk0: int = 0, plus_after: int = 0, plus_slack: int = 1) -> "Mod2Walks":
        """``walks_per_list`` walks from each of the M lists taken mod 2 (walk w starts from list w // walks_per_list and
        has the global id walk0 + w): ``ops.flip2_begin``.  ``plus_after`` > 0: ``advance`` takes plus transitions.  No
        host sync."""
        if not tokens.is_cuda:
            raise TensorGameError("Mod2Walks.start", -1, f"tokens must live on a ROCm device (got {tokens.device}); "
                                                         "there is no CPU path")
        if walks_per_list < 1:
            raise TensorGameError("Mod2Walks.start", -1, f"walks_per_list={walks_per_list} < 1")
        M = tokens.shape[0]
        src = torch.arange(M, dtype=torch.int64, device=tokens.device).repeat_interleave(int(walks_per_list))
        status = torch.zeros((1,), dtype=torch.uint32, device=tokens.device)
        if tokens.dim() == 3:
            ops.flip2_check(M, src.shape[0], tokens.shape[1], tokens.shape[2] // 3, shift, 0, 1, plus_after, plus_slack)
        st = ops.flip2_begin(tokens, lengths, src=src, shift=shift, status=status)
        return cls(st, src, status, tokens.shape[2] // 3, seed, walk0, 0, plus_after, plus_slack)

    @property
    def W(self) -> int:
        return self._st["cur"].shape[0]

    @property
    def K(self) -> int:
        return self._st["cur"].shape[1]

    def advance(self, n_steps: int) -> "Mod2Walks":
        """``n_steps`` more steps of every walk, in launches of at most TG_FLIP_MAX_STEPS.  No host sync."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise TensorGameError("Mod2Walks.advance", -1, f"n_steps={n_steps} < 0")
        while n_steps:
            n = min(n_steps, TG_FLIP_MAX_STEPS)
            ops.flip2_advance(self._st, n, self.S, self.plus_after, self.plus_slack, seed=self.seed, walk0=self.walk0,
                              step0=self.steps_done)
            self.steps_done += n
            n_steps -= n
        return self

    def _which(self, which: str, fn: str):
        if which not in ("best", "cur"):
            raise TensorGameError(fn, -1, f"which={which!r}: 'best' or 'cur'")
        return self._st[which], self._st[which + "_rank"]

    def tokens(self, which: str = "best", shift: int = 1) -> torch.Tensor:
        """int8 (W,K,3S): the ``best`` (or ``cur``) lists as token rows with values {0,1} + shift; rows at or beyond the
        rank are zero bytes.  Plain torch, no host sync."""
        lists, rank = self._which(which, "Mod2Walks.tokens")
        bits = (lists[:, :, :, None] >> torch.arange(self.S, dtype=torch.int32, device=lists.device)) & 1   # (W,K,3,S)
        live = torch.arange(self.K, device=lists.device)[None, :] < rank[:, None]
        return ((bits + int(shift)) * live[:, :, None, None]).to(torch.int8).reshape(self.W, self.K, 3 * self.S)

    def residual(self, targets: torch.Tensor, which: str = "best") -> torch.Tensor:
        """int32 (W,): ``ops.flip2_residual`` of the ``best`` (or ``cur``) lists against ``targets`` int8 (W,S,S,S), one
        per walk: 0 where the list sums to its target mod 2."""
        lists, rank = self._which(which, "Mod2Walks.residual")
        return ops.flip2_residual(targets, lists, rank)

    def lift(self, targets: torch.Tensor, which: str = "best", tries: int = 32, seed: Optional[int] = None):
        """``lift.lift_signs`` of the ``best`` (or ``cur``) lists against the INTEGER ``targets`` int8 (W,S,S,S), one per
        walk, with list0 = walk0 and the walks' seed unless ``seed`` is given: a ``LiftResult``.  No host sync."""
        from .lift import lift_signs
        lists, rank = self._which(which, "Mod2Walks.lift")
        return lift_signs(lists, rank, targets, tries=tries, seed=self.seed if seed is None else seed, list0=self.walk0)

    def state_dict(self) -> dict:
        """Host tensors and plain scalars (loads with ``weights_only=True``); synchronises."""
        return {"version": STATE_VERSION, "S": self.S, "seed": self.seed, "walk0": self.walk0,
                "steps_done": self.steps_done, "plus_after": self.plus_after, "plus_slack": self.plus_slack,
                "status": int(self.status.cpu().view(torch.int32).item()), "src": self.src.cpu(),
                **{k: self._st[k].cpu() for k in _STATE}}

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda") -> "Mod2Walks":
        """The walks ``state_dict`` described, on ``device``: ``advance`` continues them bit for bit."""
        fn = "Mod2Walks.from_state_dict"
        if sd.get("version") != STATE_VERSION:
            raise TensorGameError(fn, -1, f"version {sd.get('version')!r}, expected {STATE_VERSION}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError(fn, -1, f"a ROCm device is required (got {dev}); there is no CPU path")
        st = {k: sd[k].to(dev).contiguous() for k in _STATE}
        W = st["cur"].shape[0]
        if st["cur"].dim() != 3 or any(st[k].shape[0] != W for k in _STATE) or st["best"].shape != st["cur"].shape \
                or sd["src"].shape != (W,):
            raise TensorGameError(fn, -1, "the stored tensors do not fit together")
        status = torch.tensor([int(sd["status"])], dtype=torch.int32, device=dev).view(torch.uint32)
        return cls(st, sd["src"].to(dev), status, sd["S"], sd["seed"], sd["walk0"], sd["steps_done"], sd["plus_after"],
                   sd["plus_slack"])


class Mod2Result(NamedTuple):
    """What ``reduce_mod2`` reached.  ``walks``: the ``Mod2Walks``; ``residual`` int32 (W,): ``tg_flip2_residual`` of each
    walk's best list against the sum of the list it started from; ``proven`` bool (W,): residual == 0; ``best_rank``
    int32 (M,): per source list the lowest proven best_rank among its walks (-1: none)."""
    walks: Mod2Walks
    residual: torch.Tensor
    proven: torch.Tensor
    best_rank: torch.Tensor


def reduce_mod2(tokens: torch.Tensor, lengths: torch.Tensor, n_steps: int, walks_per_list: int = 8, shift: int = 1,
                seed: int = 0, plus_after: int = 0, plus_slack: int = 1) -> Mod2Result:
    """Walk M lists over Z_2 and prove what the walks reached: the targets are the lists' own sums (``flips.term_sum``,
    one host sync), ``walks_per_list`` walks start from each list, run ``n_steps`` steps, and ``tg_flip2_residual`` counts
    the cells where a walk's best list and its target differ mod 2.  Nothing is reported as proven but through that
    count, and nothing enters a ``SolutionArchive``: its proof is over the integers."""
    targets = term_sum(tokens, lengths, shift)
    walks = Mod2Walks.start(tokens, lengths, walks_per_list=walks_per_list, shift=shift, seed=seed, plus_after=plus_after,
                            plus_slack=plus_slack)
    walks.advance(n_steps)
    residual = walks.residual(targets[walks.src].contiguous())
    proven = residual == 0
    M, big = tokens.shape[0], torch.iinfo(torch.int32).max
    rank = torch.where(proven & (walks.state >= 0), walks.best_rank, torch.full_like(walks.best_rank, big))
    lowest = rank.view(M, int(walks_per_list)).min(dim=1).values if M else rank
    return Mod2Result(walks, residual, proven, torch.where(lowest == big, torch.full_like(lowest, -1), lowest))


def reduce_archive_mod2(arch, n_steps: int, walks_per_entry: int = 8, seed: int = 0, plus_after: int = 0,
                        plus_slack: int = 1) -> Optional[Mod2Result]:
    """``reduce_mod2`` from every entry of a ``SolutionArchive`` (its lists taken mod 2, ``walks_per_entry`` walks each).
    The archive is only read: what the walks reach is proven mod 2, which is no proof over the integers, so nothing is
    added to it.  None for an empty archive.  Synchronises (``entries``)."""
    tokens, rank, _, _ = arch.entries()
    if tokens.shape[0] == 0:
        return None
    return reduce_mod2(tokens.contiguous(), rank.to(torch.int64), n_steps, walks_per_list=walks_per_entry, shift=arch.shift,
                       seed=seed, plus_after=plus_after, plus_slack=plus_slack)
