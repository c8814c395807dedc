"""``FlipWalks``: random walks on the flip graph, which lower the rank of factorisations that are already known.

The archive (``SolutionArchive``) proves, canonicalises and stores what the solution search finds; the walks improve it.
Two terms that share a factor are rewritten into two other terms with the same sum (Kauers and Moosbauer, "Flip graphs
for matrix multiplication", 2022); whenever two terms come to share two factors they merge and the rank drops.  The
rules are those of include/tensor_game_flips.h: every walk is a wavefront's worth of state on the device, independent of
every other walk, without floating point, and a function of (its list, seed, walk id, step) alone:

    walks = FlipWalks.start(tokens, lengths, walks_per_list=8, bound=1, seed=0)   # tokens int8 (M,K,3S), lengths int64 (M,)
    walks.advance(100_000)                                                        # launches of <= 65 536 steps, no host sync
    FlipWalks.start(..., plus_after=10_000, plus_slack=1)                         # with plus transitions (below)
    walks.best, walks.best_rank, walks.best_step, walks.state, walks.src          # device tensors
    rep, walks = reduce_archive(arch, n_steps=100_000)                            # walk the archive's entries; what is
    arch.lowest_rank                                                              # shorter and PROVEN enters the archive
    save_run(..., extra={"flips": walks.state_dict()}); FlipWalks.from_state_dict(sd, "cuda:0").advance(n)  # bit for bit

A shorter list enters an archive only through ``SolutionArchive.add``: the exact proof against the sum of the list the
walk started from (``term_sum``) and, with a group, ``orbit_fixes``.

A walk without a match is stuck: flips only move inside one component of the graph.  With ``plus_after=N`` the walks
follow include/tensor_game_flips_plus.h instead: a walk that has no flip left, or has not lowered its rank for N steps,
rewrites two terms into three with the same sum (a "plus" transition) while its list is shorter than
min(K, best_rank + plus_slack), and goes on in another component.  ``plus_after=None`` (the default) gives the plain
walks, unchanged.  The same walks over the field with two elements are ``Mod2Walks`` (flips_mod2.py).  Not done here:
choosing the entries to walk adaptively, reviving stuck walks.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from ._lib import TG_FLIP_MAX_STEPS, TensorGameError

__all__ = ["FlipWalks", "term_sum", "reduce_archive"]

STATE_VERSION = 1        # plain walks
STATE_VERSION_PLUS = 2   # walks with plus transitions: also since, pluses, plus_after, plus_slack
_STATE = ("cur", "cur_rank", "best", "best_rank", "best_step", "flips", "state")
_PLUS_STATE = ("since", "pluses")


def term_sum(tokens: torch.Tensor, lengths: torch.Tensor, shift: int = 1) -> torch.Tensor:
    """int8 (M,S,S,S): the tensor each list sums to, sum_{t < lengths[m]} u (x) v (x) w with (u,v,w) = tokens[m][t] -
    shift.  Plain torch in int32, which cannot wrap (tensor_game_solutions.h); a sum outside int8 is refused (one host
    sync)."""
    if tokens.dim() != 3 or tokens.shape[2] % 3 or tokens.dtype != torch.int8:
        raise TensorGameError("term_sum", -1, f"tokens must be int8 (M,K,3S), got {tokens.dtype} {tuple(tokens.shape)}")
    M, K, S = tokens.shape[0], tokens.shape[1], tokens.shape[2] // 3
    live = torch.arange(K, device=tokens.device)[None, :] < lengths.to(tokens.device)[:, None]
    f = (tokens.to(torch.int32) - int(shift)) * live[:, :, None].to(torch.int32)
    u, v, w = f[:, :, :S], f[:, :, S:2 * S], f[:, :, 2 * S:]
    uv = (u[:, :, :, None] * v[:, :, None, :]).reshape(M, K, S * S)
    total = torch.zeros((M, S * S, S), dtype=torch.int32, device=tokens.device)
    for t in range(K):  # (no int32 matmul on the device; K rank-1 updates, not hot)
        total += uv[:, t, :, None] * w[:, t, None, :]
    if M and (int(total.min()) < -128 or int(total.max()) > 127):
        raise TensorGameError("term_sum", -1, "a list sums to a tensor outside int8")
    return total.to(torch.int8).view(M, S, S, S)


class FlipWalks:
    """W walks on the device.  ``cur``, ``best`` int8 (W,K,3S); ``cur_rank``, ``best_rank``, ``state`` int32 (W,)
    (0 walking, 1 stuck, -1 bad); ``best_step``, ``flips`` int64 (W,); ``src`` int64 (W,): the list each walk started
    from; ``status`` uint32 (1,): the bad-row bits of ``ops.flip_begin``; ``steps_done``: a host integer.  With
    ``plus_after`` (not None) also ``since`` int32 (W,) and ``pluses`` int64 (W,) of tensor_game_flips_plus.h."""

    def __init__(self, st: dict, src: torch.Tensor, status: torch.Tensor, bound: int, shift: int, seed: int, walk0: int,
                 steps_done: int = 0, plus_after: Optional[int] = None, plus_slack: int = 1):
        self._st = st
        self.src, self.status = src, status
        self.bound, self.shift, self.seed, self.walk0 = int(bound), int(shift), int(seed), int(walk0)
        self.steps_done = int(steps_done)
        self.plus_after, self.plus_slack = None if plus_after is None else int(plus_after), int(plus_slack)

    def __getattr__(self, name):
        if name in _STATE or (name in _PLUS_STATE and name in self.__dict__.get("_st", ())):
            return self._st[name]
        raise AttributeError(name)

    @classmethod
    def start(cls, tokens: torch.Tensor, lengths: torch.Tensor, walks_per_list: int = 1, bound: int = 1, shift: int = 1,
              seed: int = 0, walk0: int = 0, plus_after: Optional[int] = None, plus_slack: int = 1) -> "FlipWalks":
        """``walks_per_list`` walks from each of the M lists (walk w starts from list w // walks_per_list and has the
        global id walk0 + w): ``ops.flip_begin``.  ``plus_after``: None for plain walks, else ``advance`` takes plus
        transitions (``ops.flip_advance_plus``) with this ``plus_after`` and ``plus_slack``.  No host sync."""
        if not tokens.is_cuda:
            raise TensorGameError("FlipWalks.start", -1, f"tokens must live on a ROCm device (got {tokens.device}); "
                                                         "there is no CPU path")
        if walks_per_list < 1:
            raise TensorGameError("FlipWalks.start", -1, f"walks_per_list={walks_per_list} < 1")
        M = tokens.shape[0]
        src = torch.arange(M, dtype=torch.int64, device=tokens.device).repeat_interleave(int(walks_per_list))
        status = torch.zeros((1,), dtype=torch.uint32, device=tokens.device)
        if plus_after is not None:
            ops.flip_plus_check(src.shape[0], tokens.shape[1], tokens.shape[2] // 3, shift, bound, 0, 1, plus_after, plus_slack)
        st = ops.flip_begin(tokens, lengths, src=src, bound=bound, shift=shift, status=status)
        if plus_after is not None:
            st["since"] = torch.zeros_like(st["cur_rank"])
            st["pluses"] = torch.zeros_like(st["flips"])
        return cls(st, src, status, bound, shift, seed, walk0, 0, plus_after, plus_slack)

    @property
    def W(self) -> int:
        return self._st["cur"].shape[0]

    def advance(self, n_steps: int) -> "FlipWalks":
        """``n_steps`` more steps of every walk, in launches of at most TG_FLIP_MAX_STEPS.  No host sync."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise TensorGameError("FlipWalks.advance", -1, f"n_steps={n_steps} < 0")
        while n_steps:
            n = min(n_steps, TG_FLIP_MAX_STEPS)
            if self.plus_after is None:
                ops.flip_advance(self._st, n, bound=self.bound, shift=self.shift, seed=self.seed, walk0=self.walk0,
                                 step0=self.steps_done)
            else:
                ops.flip_advance_plus(self._st, n, self.plus_after, self.plus_slack, bound=self.bound, shift=self.shift,
                                      seed=self.seed, walk0=self.walk0, step0=self.steps_done)
            self.steps_done += n
            n_steps -= n
        return self

    def state_dict(self) -> dict:
        """Host tensors and plain scalars (loads with ``weights_only=True``); synchronises."""
        sd = {"version": STATE_VERSION, "bound": self.bound, "shift": self.shift, "seed": self.seed, "walk0": self.walk0,
              "steps_done": self.steps_done, "status": int(self.status.cpu().view(torch.int32).item()),
              "src": self.src.cpu(), **{k: self._st[k].cpu() for k in _STATE}}
        if self.plus_after is not None:
            sd.update(version=STATE_VERSION_PLUS, plus_after=self.plus_after, plus_slack=self.plus_slack,
                      **{k: self._st[k].cpu() for k in _PLUS_STATE})
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda") -> "FlipWalks":
        """The walks ``state_dict`` described, on ``device``: ``advance`` continues them bit for bit."""
        if sd.get("version") not in (STATE_VERSION, STATE_VERSION_PLUS):
            raise TensorGameError("FlipWalks.from_state_dict", -1, f"version {sd.get('version')!r}, expected {STATE_VERSION} "
                                                                   f"or {STATE_VERSION_PLUS}")
        names = _STATE + (_PLUS_STATE if sd["version"] == STATE_VERSION_PLUS else ())
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError("FlipWalks.from_state_dict", -1, f"a ROCm device is required (got {dev}); there is no "
                                                                   "CPU path")
        st = {k: sd[k].to(dev).contiguous() for k in names}
        W = st["cur"].shape[0]
        if st["cur"].dim() != 3 or any(st[k].shape[0] != W for k in names) or st["best"].shape != st["cur"].shape \
                or sd["src"].shape != (W,):
            raise TensorGameError("FlipWalks.from_state_dict", -1, "the stored tensors do not fit together")
        status = torch.tensor([int(sd["status"])], dtype=torch.int32, device=dev).view(torch.uint32)
        return cls(st, sd["src"].to(dev), status, sd["bound"], sd["shift"], sd["seed"], sd["walk0"], sd["steps_done"],
                   sd.get("plus_after"), sd.get("plus_slack", 1))


def reduce_archive(arch, n_steps: int, walks_per_entry: int = 8, bound: Optional[int] = None, seed: int = 0,
                   plus_after: Optional[int] = None, plus_slack: int = 1) -> Tuple[object, Optional[FlipWalks]]:
    """Walk every entry of a ``SolutionArchive`` and add what the walks reached: the targets are the entries' own sums
    (``term_sum``), ``walks_per_entry`` walks start from each entry, run ``n_steps`` steps, and
    ``arch.add(targets[src], best, best_rank)`` proves each walk's shortest list exactly and stores what is new.
    ``bound`` defaults to ``arch.shift``, so that every value stays a playable token.  ``plus_after``, ``plus_slack``: as
    in ``FlipWalks.start`` (walks with plus transitions; the proof is the only way in all the same, and a list of
    ``arch.max_rank`` terms has no free slot for a plus).  Returns (the ``AddReport`` of
    that add, the ``FlipWalks``); (None, None) for an empty archive.  Synchronises (``entries``)."""
    tokens, rank, _, _ = arch.entries()
    if tokens.shape[0] == 0:
        return None, None
    lengths = rank.to(torch.int64)
    targets = term_sum(tokens, lengths, arch.shift)
    walks = FlipWalks.start(tokens.contiguous(), lengths, walks_per_list=walks_per_entry,
                            bound=arch.shift if bound is None else bound, shift=arch.shift, seed=seed,
                            plus_after=plus_after, plus_slack=plus_slack)
    walks.advance(n_steps)
    rep = arch.add(targets[walks.src].contiguous(), walks.best, walks.best_rank.to(torch.int64))
    return rep, walks
