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

from . import ops, replay_io
from ._lib import TG_REPLAY_BEST, TG_REPLAY_PLAYED, TG_REPLAY_SYNTH, ReplayBufferDesc, TensorGameError

__all__ = ["GameBuffer", "TensorGameData"]

_BAD_KIND = 3  # a row whose index the reference's lists do not hold: an all-zero item with status bit 0


class GameBuffer:
    """A ring of ``capacity`` finished games of up to ``max_actions`` moves, each move stored as its ``T`` frames, its
    argmax tokens and its reward (``PlayedGamesDataset``: ``buffer_size`` = capacity).  Flat move indices walk the slots
    in slot order, as the reference walks ``game_lengths``.  ``status`` (uint32 (1,)) collects bit 0 for a game that was
    not stored (length 0 or > max_actions) and for a bad item index, and bits 2, 3 and 4 for a move list ``add_lists``
    refused (a bad group, a head outside int8, a last head that is not zero)."""

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

    def add_lists(self, starts, tokens, lengths, groups=None, shift: int = 1, best: bool = False) -> torch.Tensor:
        """Store move lists that take their start states to zero -- what ``solutions()`` of the solution search returns
        -- as games (``ops.replay_add_lists``): starts int8 (G,T,S,S,S), tokens int8 (M,K,3S), lengths (M,), groups
        (M,) (None: list m starts from starts[m]).  Every valid list is stored, or with ``best`` only the first
        shortest one; an invalid list (a bad length or group, a head that leaves int8, a last head that is not zero)
        stores nothing and sets bit 0, 2, 3 or 4 of ``status``.  Returns stored uint8 (M,).  Asynchronous."""
        dev = self.device
        lengths = torch.as_tensor(lengths, device=dev).to(torch.int64).contiguous()
        if groups is not None:
            groups = torch.as_tensor(groups, device=dev).to(torch.int64).contiguous()
        return ops.replay_add_lists(self, starts, tokens, lengths, groups=groups, shift=shift, select=best,
                                    status=self.status)

    def __len__(self) -> int:
        """Moves stored (``sum(game_lengths.values())``).  A host sync."""
        return int(self.offset[self.C])

    def games_added(self) -> int:
        """Games ever added (a host sync)."""
        return int(self.ring[1])

    def items(self, idx, dtype=torch.float32, augment=None):
        """The ``__getitem__`` tuples of a batch of flat move indices in one launch (``ops.replay_items``): (state
        (N,T,S,S,S) of ``dtype``, scalar fp32 (N,1) = the move index, action int8 (N,3S), reward fp32 (N,1)).  An index
        outside the stored moves gives an all-zero item and sets bit 0 of ``status``.  ``augment`` (an ``Augment``):
        the items are gathered as int8 and the augmenter emits state and action in a random symmetric copy (two more
        launches); scalar and reward pass through."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int64).reshape(-1)
        if augment is not None:
            state, scalar, action, reward = ops.replay_items(idx, self.T, self.S, self.device, played=self,
                                                             direct_kind=TG_REPLAY_PLAYED, dtype=torch.int8,
                                                             status=self.status)
            state, action = augment(state, action, dtype, status=self.status)
            return state, scalar, action, reward
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

    # ---- dense form and disk (include/tensor_game_replay_io.h, replay_io) ----------------------------------------
    def pack(self):
        """The stored games as dense device tensors, oldest first: (frames int8 (M,T,S,S,S), tokens int8 (M,3S), rewards
        float32 (M,), lengths int32 (G,), ring int64 (2,)).  One host sync (G and M, read together), then one
        ``tg_replay_pack`` call into exactly M rows."""
        G, M = (int(v) for v in torch.stack([(self.length > 0).sum(), self.offset[self.C]]).cpu())
        frames, tokens, rewards, lengths, _, _ = ops.replay_pack(self, M, status=self.status)
        return frames, tokens, rewards, lengths[:G], self.ring.clone()

    def add_packed(self, frames, tokens, rewards, lengths, first_slot: Optional[int] = None,
                   games_added: Optional[int] = None) -> None:
        """Store games given in the dense form of ``pack`` (``tg_replay_add_packed``): oldest first into consecutive
        slots from the ring's next slot, or from ``first_slot``; ``games_added`` sets the games-ever-added counter
        instead of growing it.  No float policy is needed.  Asynchronous."""
        dev = self.device
        ops.replay_add_packed(self, torch.as_tensor(frames, device=dev).contiguous(),
                              torch.as_tensor(tokens, device=dev).contiguous(),
                              torch.as_tensor(rewards, device=dev).to(torch.float32).contiguous(),
                              torch.as_tensor(lengths, device=dev).to(torch.int32).contiguous(),
                              -1 if first_slot is None else int(first_slot),
                              -1 if games_added is None else int(games_added), status=self.status)

    def packed(self) -> "replay_io.PackedGames":
        """``pack`` on the host (``replay_io.PackedGames``)."""
        frames, tokens, rewards, lengths, ring = (t.cpu().numpy() for t in self.pack())
        return replay_io.PackedGames(self.C, self.L, self.T, self.S, (int(ring[0]), int(ring[1])), lengths, rewards,
                                     tokens, frames)

    @classmethod
    def from_packed(cls, p: "replay_io.PackedGames", device="cuda", capacity: Optional[int] = None,
                    max_actions: Optional[int] = None) -> "GameBuffer":
        """A buffer holding the games of ``p``.  With ``p``'s capacity every game returns to the slot it had
        (first_slot = (ring[0] - G) mod C, games_added = ring[1]; the stored games of a ring the adds filled are
        consecutive), so flat move indices stay what they were.  With another capacity the buffer is what adding the
        games oldest first to an empty buffer leaves, the newest ``capacity`` of them when it holds fewer.  A game
        longer than ``max_actions`` is refused."""
        C = p.C if capacity is None else int(capacity)
        L = p.L if max_actions is None else int(max_actions)
        if p.G and int(p.lengths.max()) > L:
            raise ValueError(f"a stored game has {int(p.lengths.max())} moves, max_actions={L}")
        buf = cls(C, L, p.T, p.S, device)
        if C == p.C:
            first, added, row0, g0 = (p.ring[0] - p.G) % C, p.ring[1], 0, 0
            if p.G == 0:  # add_packed of no games is a no-op: the ring words of an empty ring that had games
                buf.ring.copy_(torch.tensor(p.ring, dtype=torch.int64))
        else:
            g0 = max(0, p.G - C)
            first, added, row0 = None, None, int(p.starts()[g0])
        buf.add_packed(torch.from_numpy(p.frames[row0:]), torch.from_numpy(p.tokens[row0:]),
                       torch.from_numpy(p.rewards[row0:]), torch.from_numpy(p.lengths[g0:]), first_slot=first,
                       games_added=added)
        return buf

    def save(self, path) -> None:
        """The stored games to one file (``replay_io``: a header, then lengths, rewards, tokens, frames)."""
        replay_io.save_games(path, self.packed())

    @classmethod
    def load(cls, path, device="cuda", capacity: Optional[int] = None, max_actions: Optional[int] = None) -> "GameBuffer":
        """The buffer ``save`` wrote (``from_packed``: the same slots at the saved capacity)."""
        return cls.from_packed(replay_io.load_games(path), device, capacity, max_actions)


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

    def add_solutions(self, res, states: torch.Tensor) -> torch.Tensor:
        """The factorisations a solution search found, as games to train on: ``res`` is a ``RolloutResult`` (its
        ``solutions()``) or a ``SolveResult`` (its groups, tokens and lengths), resolved as
        ``SolutionArchive.add_result`` resolves it, and ``states`` int8 (G,dim_t,S,S,S) the start states the search ran
        on.  Every valid list goes to the played buffer and the first shortest one to the best buffer, as
        ``add_act_step`` does for played games.  For ``bases.solve_in_bases`` pass ``reb.found`` with
        ``bases.expand(states)[0]``: the lists of ``found`` start from the expanded states.  Returns stored uint8 (M,):
        1 where the list was stored in the played buffer.  No host sync of its own."""
        if hasattr(res, "solutions"):
            groups, tokens, lengths = res.solutions()
        else:
            groups, tokens, lengths = res.groups, res.tokens, res.lengths
        if getattr(res, "shift", self.shift) != self.shift:
            raise TensorGameError("add_solutions", -1, f"res.shift={res.shift}, the dataset's shift={self.shift}")
        want = (self.dim_t, self.S, self.S, self.S)
        if states.dim() != 5 or tuple(states.shape[1:]) != want or states.dtype != torch.int8:
            raise TensorGameError("add_solutions", -1, f"states must be int8 (G,T,S,S,S) with (T,S,S,S) = {want}, got "
                                                       f"{states.dtype} {tuple(states.shape)}")
        if tokens.dim() != 3 or tokens.shape[1] > self.played.L:
            raise TensorGameError("add_solutions", -1, f"max_actions: the lists have {tuple(tokens.shape)[1:2]} moves, "
                                                       f"the buffers hold {self.played.L}")
        stored = self.played.add_lists(states, tokens, lengths, groups=groups, shift=self.shift)
        self.best.add_lists(states, tokens, lengths, groups=groups, shift=self.shift, best=True)
        return stored

    # ---- disk -----------------------------------------------------------------------------------------------------
    def _targets_hash(self, targets) -> int:
        h = ops.state_hash(targets).cpu().numpy()
        return int(np.bitwise_xor.reduce(h)) if h.size else 0

    def save(self, path, demos: bool = True) -> None:
        """The dataset to one file (``replay_io.save_dataset``): both buffers, the sizes and fractions, the epoch's four
        index arrays (``kind`` / ``src`` are recomposed at load), the device generator's state and, unless ``demos`` is
        false, the demos.  Without them the caller passes the same demos to ``load``."""
        host = lambda t: None if t is None else t.cpu().numpy()
        replay_io.save_dataset(path, dict(
            len_data=self.len_data, dim_t=self.dim_t, shift=self.shift, R=self.R, S=self.S,
            n_demos=self.tokens.shape[0], fract_synth=self.fract_synth, fract_best=self.fract_best,
            targets_hash=self._targets_hash(self.targets), is_synth=host(self.is_synth),
            index_synth=host(self.index_synth), index_played=host(self.index_played), index_best=host(self.index_best),
            generator=self.generator.get_state().numpy(), played=self.played.packed(), best=self.best.packed(),
            tokens=host(self.tokens) if demos else None, targets=host(self.targets) if demos else None))

    @classmethod
    def load(cls, path, device="cuda", tokens=None, targets=None) -> "TensorGameData":
        """The dataset ``save`` wrote, on ``device``: its next ``resample_buffer_indexes`` and its batches are those of
        the object that was saved.  ``tokens`` / ``targets`` (device tensors) are needed exactly when the file holds no
        demos; their shapes and the hash of the targets must match what the file recorded."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError("TensorGameData", -1, "the demos must live on a ROCm device; there is no CPU path")
        d = replay_io.load_dataset(path)
        self = cls.__new__(cls)
        self.device = dev
        self.S, self.R, self.dim_t, self.shift = d["S"], d["R"], d["dim_t"], d["shift"]
        if d["tokens"] is not None:
            if tokens is not None or targets is not None:
                raise ValueError(f"{path} holds its demos; pass none")
            tokens, targets = torch.from_numpy(d["tokens"]).to(dev), torch.from_numpy(d["targets"]).to(dev)
        else:
            if tokens is None or targets is None:
                raise ValueError(f"{path} holds no demos; pass the tokens and targets it was saved with")
            want = ((d["n_demos"], self.R, 3 * self.S), (d["n_demos"], self.S, self.S, self.S))
            if (tuple(tokens.shape), tuple(targets.shape)) != want or tokens.device != dev or targets.device != dev:
                raise ValueError(f"the demos must be {want[0]} and {want[1]} on {dev}, got {tuple(tokens.shape)} and "
                                 f"{tuple(targets.shape)} on {tokens.device}")
            if self._targets_hash(targets) != d["targets_hash"]:
                raise ValueError(f"the targets are not the ones {path} was saved with")
        self.tokens, self.targets = tokens, targets
        self.n_synth, self.len_data = d["n_demos"] * self.R, d["len_data"]
        self.played = GameBuffer.from_packed(d["played"], dev)
        self.best = GameBuffer.from_packed(d["best"], dev)
        self.status = torch.zeros((1,), dtype=torch.uint32, device=dev)
        self.generator = torch.Generator(device=dev)
        self.generator.set_state(torch.from_numpy(d["generator"].copy()))
        self.fract_synth, self.fract_best = d["fract_synth"], d["fract_best"]
        on_dev = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        self.is_synth = on_dev(d["is_synth"])
        self.index_synth, self.index_played, self.index_best = (on_dev(d[k]) for k in (
            "index_synth", "index_played", "index_best"))
        self._compose()
        return self

    # ---- items -------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self.len_data

    def items(self, idx, dtype=torch.float32, augment=None):
        """The ``__getitem__`` tuples of a batch of dataset indices in one launch (``ops.replay_items``): (state
        (N,dim_t,S,S,S) of ``dtype``, scalar fp32 (N,1), action int8 (N,3S), reward fp32 (N,1)).  A synthetic item's
        scalar is R - k, a played or best item's its move index (as the reference's two datasets do).  ``augment`` (an
        ``Augment``): as in ``GameBuffer.items``."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int64).reshape(-1)
        if augment is not None:
            if augment.shift != self.shift:
                raise TensorGameError("items", -1, f"augment.shift={augment.shift} != the dataset's shift={self.shift}")
            state, scalar, action, reward = ops.replay_items(
                idx, self.dim_t, self.S, self.device, tokens=self.tokens, targets=self.targets, played=self.played,
                best=self.best, kind=self.kind, src=self.src, dtype=torch.int8, status=self.status, shift=self.shift)
            state, action = augment(state, action, dtype, status=self.status)
            return state, scalar, action, reward
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
                drop_last: bool = False, dtype=torch.float32, augment=None) -> Iterator[Tuple[torch.Tensor, ...]]:
        """One epoch of ``DataLoader(dataset, batch_size, shuffle=True)`` (training.py:424): a permutation of
        [0, len_data) drawn on the device (``generator``: a generator of that device), each batch one
        ``tg_replay_items`` launch (``augment``: as in ``items``).  No host sync."""
        if batch_size < 1:
            raise TensorGameError("batches", -1, "batch_size must be >= 1")
        if shuffle:
            order = torch.randperm(self.len_data, generator=generator, device=self.device)
        else:
            order = torch.arange(self.len_data, device=self.device)
        stop = self.len_data - self.len_data % batch_size if drop_last else self.len_data
        for lo in range(0, stop, batch_size):
            yield self.items(order[lo:lo + batch_size], dtype=dtype, augment=augment)
