"""Replay buffers of played games and the mixed training dataset, on the device.

``GameBuffer`` stands in for ``PlayedGamesDataset`` (reference datasets.py:161-230) and ``TensorGameData`` for
``TensorGameDataset`` (datasets.py:233-359).  The games live in HBM (include/tensor_game_replay.h): adding the games of
an act step is three kernel launches with no host round trip, and a training batch of the synthetic / played / best
mixture is ONE ``tg_replay_items`` launch, as a pure synthetic batch is (``SyntheticDemos.batches``).
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import TG_REPLAY_BEST, TG_REPLAY_PLAYED, TG_REPLAY_SYNTH, ReplayBufferDesc, TensorGameError

__all__ = ["GameBuffer", "TensorGameData"]

_BAD_KIND = 3  # a row whose index the reference's lists do not hold: an all-zero item with status bit 0


class GameBuffer:
    """A ring of ``capacity`` finished games of up to ``max_actions`` moves, each move stored as its ``T`` frames, its
    argmax tokens and its reward (``PlayedGamesDataset``: ``buffer_size`` = capacity).  Flat move indices walk the slots
    in slot order, as the reference walks ``game_lengths``.  ``status`` (uint32 (1,)) collects bit 0 for a game that was
    not stored (length 0 or > max_actions) and for a bad item index."""

    def __init__(self, capacity: int, max_actions: int, T: int, S: int, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TensorGameError("GameBuffer", -1, f"the buffer lives on a ROCm device (got {self.device}); there is "
                                  "no CPU path")
        self.C, self.L, self.T, self.S = int(capacity), int(max_actions), int(T), int(S)
        dev = self.device
        self.frames = torch.zeros((self.C, self.L, self.T, S, S, S), dtype=torch.int8, device=dev)
        self.tokens = torch.zeros((self.C, self.L, 3 * S), dtype=torch.int8, device=dev)
        self.rewards = torch.zeros((self.C, self.L), dtype=torch.float32, device=dev)
        self.length = torch.zeros((self.C,), dtype=torch.int32, device=dev)
        self.offset = torch.zeros((self.C + 1,), dtype=torch.int64, device=dev)
        self.ring = torch.zeros((2,), dtype=torch.int64, device=dev)  # next slot, games ever added
        self.status = torch.zeros((1,), dtype=torch.uint32, device=dev)
        self.desc = ReplayBufferDesc(self.C, self.L, self.T, self.S, *(t.data_ptr() for t in (
            self.frames, self.tokens, self.rewards, self.length, self.offset, self.ring)))

    def _add(self, states, policy, rewards, lengths, select: bool) -> None:
        rewards = torch.as_tensor(rewards, device=self.device).to(torch.float32).contiguous()
        lengths = torch.as_tensor(lengths, device=self.device).to(torch.int64).contiguous()
        ops.replay_add(self, states, policy, rewards, lengths, select=select, status=self.status)

    def add_games(self, states, policy, rewards, lengths) -> None:
        """Store every game of a batch, in order (``add_game`` once per game): states int8 (B,L,T,S,S,S), policy float32
        (B,L,3S,n_logits), rewards (B,L) (any real dtype: search.actor_prediction's int64 is converted), lengths (B,).
        Only the argmax tokens of the policy are kept (datasets.py:206).  Asynchronous."""
        self._add(states, policy, rewards, lengths, False)

    def add_best(self, states, policy, rewards, lengths) -> None:
        """Store only the first game with the greatest final reward (act_step's best game, training.py:468-483; nothing
        when no final reward exceeds -1e6).  Asynchronous."""
        self._add(states, policy, rewards, lengths, True)

    def __len__(self) -> int:
        """Moves stored (``sum(game_lengths.values())``).  A host sync."""
        return int(self.offset[self.C])

    def games_added(self) -> int:
        """Games ever added (a host sync)."""
        return int(self.ring[1])

    def items(self, idx, dtype=torch.float32):
        """The ``__getitem__`` tuples of a batch of flat move indices in one launch (``ops.replay_items``): (state
        (N,T,S,S,S) of ``dtype``, scalar fp32 (N,1) = the move index, action int8 (N,3S), reward fp32 (N,1)).  An index
        outside the stored moves gives an all-zero item and sets bit 0 of ``status``."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int64).reshape(-1)
        return ops.replay_items(idx, self.T, self.S, self.device, played=self, direct_kind=TG_REPLAY_PLAYED,
                                dtype=dtype, status=self.status)

    def __getitem__(self, i: int):
        """One item, shaped as the reference returns it: (state (T,S,S,S) fp32, scalar (1,), action (3S,), reward (1,)).
        Checks the index against ``len`` (a host sync)."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(f"move {i} outside [0, {len(self)})")
        state, scalar, action, reward = self.items(torch.tensor([i], device=self.device))
        return state[0], scalar[0], action[0], reward[0]


def _take(index: Optional[torch.Tensor], pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(index[pos], pos inside index) with out-of-range positions (and a missing index) flagged instead of raising."""
    if index is None or index.numel() == 0:
        return torch.zeros_like(pos), torch.zeros_like(pos, dtype=torch.bool)
    ok = (pos >= 0) & (pos < index.numel())
    return index[pos.clamp(0, index.numel() - 1)], ok


class TensorGameData:
    """The training dataset of the self-play loop (``TensorGameDataset``): ``len_data`` items drawn each epoch from the
    synthetic demos (``tokens`` int8 (n_demos,R,3S), ``targets`` int8 (n_demos,S,S,S)), the played-games buffer and the
    best-games buffer, in the fractions ``fract_synth`` / ``fract_best``.

    Resampling follows datasets.py:309-343, with the random streams of the DEVICE (a ``torch.Generator`` on it seeded
    with ``seed``), not numpy's or torch's CPU stream, so the draws are not the reference's draws; their rules are:
      - while the played buffer is empty, the epoch stays all synthetic with the initial ``index_synth`` (``len_data``
        distinct draws from [0, n_demos*R); construction raises when len_data > n_demos*R, as np.random.choice does);
      - is_synth = rand < fract_synth; the synthetic indexes are drawn without replacement;
      - played and best indexes are drawn with replacement exactly when more are needed than the buffer holds;
      - THE REFERENCE'S SPLIT IS KEPT AS IT IS: with best games present and fract_best > 0, len_played =
        int(1 - fract_synth - fract_best) * len_data, which is 0 (datasets.py:321), so every non-synthetic item is a
        best-game item.  The "intended" split could go negative for a random len_synth and nothing could check it.
    Routing follows __getitem__ (datasets.py:286-303): the non-synthetic remainder r of item x goes to
    best[index_best[r]] while r < len(index_best) (when fract_best > 0 and index_best exists), then to played.
    One intended difference: ``set_fractions`` takes effect at the next resample (or ``set_indexes``), because the epoch
    table is composed there; training.py always resamples right after it."""

    def __init__(self, tokens: torch.Tensor, targets: torch.Tensor, len_data: int, fract_synth: float,
                 played_capacity: int = 10000, best_capacity: int = 100, dim_t: int = 1, shift: int = 1,
                 seed: int = 0, max_actions: Optional[int] = None):
        self.tokens, self.targets = tokens, targets
        self.device = targets.device
        if self.device.type != "cuda":
            raise TensorGameError("TensorGameData", -1, "the demos must live on a ROCm device; there is no CPU path")
        n_demos, R, A3 = tokens.shape
        self.S, self.R, self.dim_t, self.shift = A3 // 3, R, int(dim_t), int(shift)
        self.n_synth = n_demos * R
        self.len_data = int(len_data)
        if self.len_data > self.n_synth:
            raise ValueError(f"len_data={self.len_data} > {self.n_synth} synthetic items: cannot take a larger sample "
                             "than population when replace=False")
        L = R if max_actions is None else int(max_actions)
        self.played = GameBuffer(played_capacity, L, self.dim_t, self.S, self.device)
        self.best = GameBuffer(best_capacity, L, self.dim_t, self.S, self.device)
        self.status = torch.zeros((1,), dtype=torch.uint32, device=self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.fract_synth, self.fract_best = float(fract_synth), 0.0
        self.is_synth = torch.ones((self.len_data,), dtype=torch.bool, device=self.device)
        self.index_synth = self._draw(self.n_synth, self.len_data, False)
        self.index_played: Optional[torch.Tensor] = None
        self.index_best: Optional[torch.Tensor] = None
        self._compose()

    @classmethod
    def from_demos(cls, demos, len_data: int, fract_synth: float, **kw) -> "TensorGameData":
        """The dataset over a ``SyntheticDemos`` set (its tokens, targets, dim_t and shift)."""
        kw.setdefault("dim_t", demos.dim_t)
        kw.setdefault("shift", demos.shift)
        return cls(demos.action_seq, demos.target_tensor, len_data, fract_synth, **kw)

    # ---- the epoch ---------------------------------------------------------------------------------------------------
    def _draw(self, n: int, k: int, replace: bool) -> torch.Tensor:
        """np.random.choice(n, k, replace) on the device stream."""
        if k < 0:
            raise ValueError(f"negative sample size {k}")
        if k == 0:
            return torch.zeros((0,), dtype=torch.int64, device=self.device)
        if n <= 0:
            raise ValueError("a non-empty sample from an empty buffer")
        if replace:
            return torch.randint(0, n, (k,), generator=self.generator, device=self.device)
        if k > n:
            raise ValueError(f"cannot take {k} of {n} without replacement")
        return torch.randperm(n, generator=self.generator, device=self.device)[:k]

    def set_fractions(self, fract_synth: float, fract_best: float) -> None:
        """As the reference's; the epoch table follows at the next ``resample_buffer_indexes`` (or ``set_indexes``)."""
        self.fract_synth, self.fract_best = float(fract_synth), float(fract_best)

    def resample_buffer_indexes(self) -> None:
        """Draw the next epoch's sources (datasets.py:309-343) and compose its table.  One host sync (the buffer
        lengths and len_synth, read together)."""
        rand = torch.rand((self.len_data,), generator=self.generator, device=self.device)
        is_synth = rand < self.fract_synth
        n_played, n_best, len_synth = (int(v) for v in torch.stack([
            self.played.offset[self.played.C], self.best.offset[self.best.C], is_synth.sum()]).cpu())
        if n_played == 0:
            return  # the epoch stays as it is (all synthetic until a game is played)
        self.is_synth = is_synth
        self.index_synth = self._draw(self.n_synth, len_synth, False)
        if n_best > 0 and self.fract_best > 0:
            len_played = int(1 - self.fract_synth - self.fract_best) * self.len_data  # datasets.py:321, kept as is
            len_best = self.len_data - len_synth - len_played
            self.index_played = self._draw(n_played, len_played, len_played > n_played)
            self.index_best = self._draw(n_best, len_best, len_best > n_best)
        else:
            len_played = self.len_data - len_synth
            self.index_played = self._draw(n_played, len_played, len_played > n_played)
        self._compose()

    def set_indexes(self, is_synth, index_synth, index_played=None, index_best=None) -> None:
        """Install the reference's four index arrays as given (bool (len_data,), then int64 index lists; None where the
        reference holds None) and compose the table with the current fractions."""
        dev = self.device
        self.is_synth = torch.as_tensor(np.asarray(is_synth, dtype=bool)).to(dev)
        if self.is_synth.shape != (self.len_data,):
            raise TensorGameError("set_indexes", -1, f"is_synth must be ({self.len_data},)")
        as_idx = lambda x: None if x is None else torch.as_tensor(np.asarray(x, dtype=np.int64)).to(dev).reshape(-1)
        self.index_synth, self.index_played, self.index_best = as_idx(index_synth), as_idx(index_played), \
            as_idx(index_best)
        self._compose()

    def _compose(self) -> None:
        """The epoch table kind uint8 / src int64 (len_data,): __getitem__'s routing, on the device, no host sync."""
        dev = self.device
        s = self.is_synth
        before = torch.cumsum(s.to(torch.int64), 0) - s.to(torch.int64)  # is_synth[:x].sum()
        r = torch.arange(self.len_data, device=dev) - before                 # the non-synthetic remainder
        v_syn, ok_syn = _take(self.index_synth, before)
        if self.fract_best > 0 and self.index_best is not None:
            lb = self.index_best.numel()
            v_best, ok_best = _take(self.index_best, r)
            v_pl, ok_pl = _take(self.index_played, r - lb)
            to_best = r < lb
            v_ns = torch.where(to_best, v_best, v_pl)
            ok_ns = torch.where(to_best, ok_best, ok_pl)
            k_ns = torch.where(to_best, TG_REPLAY_BEST, TG_REPLAY_PLAYED)
        else:
            v_ns, ok_ns = _take(self.index_played, r)
            k_ns = torch.full_like(r, TG_REPLAY_PLAYED)
        kind = torch.where(s, torch.full_like(r, TG_REPLAY_SYNTH), k_ns)
        ok = torch.where(s, ok_syn, ok_ns)
        self.kind = torch.where(ok, kind, torch.full_like(kind, _BAD_KIND)).to(torch.uint8).contiguous()
        self.src = torch.where(ok, torch.where(s, v_syn, v_ns), torch.full_like(r, -1)).contiguous()

    # ---- act step ----------------------------------------------------------------------------------------------------
    def add_act_step(self, states, policy, rewards, lengths) -> None:
        """``act_step``'s bookkeeping for a batch of games (search.actor_prediction's outputs): every game goes to the
        played buffer, the first game with the greatest final reward to the best buffer.  Asynchronous."""
        self.played.add_games(states, policy, rewards, lengths)
        self.best.add_best(states, policy, rewards, lengths)

    # ---- items -------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self.len_data

    def items(self, idx, dtype=torch.float32):
        """The ``__getitem__`` tuples of a batch of dataset indices in one launch (``ops.replay_items``): (state
        (N,dim_t,S,S,S) of ``dtype``, scalar fp32 (N,1), action int8 (N,3S), reward fp32 (N,1)).  A synthetic item's
        scalar is R - k, a played or best item's its move index (as the reference's two datasets do)."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int64).reshape(-1)
        return ops.replay_items(idx, self.dim_t, self.S, self.device, tokens=self.tokens, targets=self.targets,
                                played=self.played, best=self.best, kind=self.kind, src=self.src, dtype=dtype,
                                status=self.status, shift=self.shift)

    def __getitem__(self, i: int):
        """One item, shaped as the reference returns it: (state (dim_t,S,S,S) fp32, scalar (1,), action (3S,), reward
        (1,))."""
        i = int(i)
        if not 0 <= i < self.len_data:
            raise IndexError(f"item {i} outside [0, {self.len_data})")
        state, scalar, action, reward = self.items(torch.tensor([i], device=self.device))
        return state[0], scalar[0], action[0], reward[0]

    def batches(self, batch_size: int, shuffle: bool = True, generator: Optional[torch.Generator] = None,
                drop_last: bool = False, dtype=torch.float32) -> Iterator[Tuple[torch.Tensor, ...]]:
        """One epoch of ``DataLoader(dataset, batch_size, shuffle=True)`` (training.py:424): a permutation of
        [0, len_data) drawn on the device (``generator``: a generator of that device), each batch one
        ``tg_replay_items`` launch.  No host sync."""
        if batch_size < 1:
            raise TensorGameError("batches", -1, "batch_size must be >= 1")
        if shuffle:
            order = torch.randperm(self.len_data, generator=generator, device=self.device)
        else:
            order = torch.arange(self.len_data, device=self.device)
        stop = self.len_data - self.len_data % batch_size if drop_last else self.len_data
        for lo in range(0, stop, batch_size):
            yield self.items(order[lo:lo + batch_size], dtype=dtype)
