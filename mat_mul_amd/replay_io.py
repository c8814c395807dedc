"""Save and resume a run: replay buffers, the mixed dataset and the trainer on disk.

The reference keeps its played games as three ``torch.save`` pickles per game (datasets.py:210-230).  Here a ring leaves
the device as its stored moves only (``tg_replay_pack``, include/tensor_game_replay_io.h), goes to ONE file in the style
of ``demo_io``, and comes back without a float policy (``tg_replay_add_packed``) into the slots it had, so flat move
indices -- and with them every later batch -- stay what they were.  With the dataset's epoch table and device generator
and the trainer's parameters and dropout counter stored too, a resumed run equals the uninterrupted one bit for bit.

Everything that writes or reads a file works on HOST arrays (``PackedGames``), so it runs without a GPU; the device
halves are ``GameBuffer.pack / add_packed / save / load``, ``TensorGameData.save / load`` and
``FusedTrainer.checkpoint / from_checkpoint``.

Buffer file: 128-byte header ``TGREPLY1`` + little-endian int64 (C, L, T, S, G, M, ring[0], ring[1], 7 zeros), then
lengths int32 (G,), rewards float32 (M,), tokens int8 (M,3S), frames int8 (M,T,S,S,S); games oldest first.
Dataset file: 128-byte header ``TGDATA01`` + int64 (len_data, dim_t, shift, R, S, n_demos, demos stored,
len(index_synth), len(index_played) or -1, len(index_best) or -1, generator state bytes, XOR of the targets' state
hashes, 0) + float64 (fract_synth, fract_best), then is_synth uint8, the three int64 index lists, the generator state,
the played and the best buffer in the form above, and (when stored) tokens int8 (n_demos,R,3S) and targets int8
(n_demos,S,S,S).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Mapping, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._lib import TensorGameError

__all__ = ["PackedGames", "write_games", "read_games", "save_games", "load_games", "export_reference_games",
           "import_reference_games", "save_dataset", "load_dataset", "save_run", "load_run", "RunState"]

MAGIC = b"TGREPLY1"
HEADER = struct.Struct("<8s15q")
DATA_MAGIC = b"TGDATA01"
DATA_HEADER = struct.Struct("<8s13q2d")
assert HEADER.size == 128 and DATA_HEADER.size == 128


@dataclass
class PackedGames:
    """The stored games of a ring of capacity C, oldest first, on the host: lengths int32 (G,), and M = lengths.sum()
    rows of rewards float32 (M,), tokens int8 (M,3S), frames int8 (M,T,S,S,S); ring = (next slot, games ever added)."""

    C: int
    L: int
    T: int
    S: int
    ring: Tuple[int, int]
    lengths: np.ndarray
    rewards: np.ndarray
    tokens: np.ndarray
    frames: np.ndarray

    def __post_init__(self):
        self.C, self.L, self.T, self.S = int(self.C), int(self.L), int(self.T), int(self.S)
        self.ring = (int(self.ring[0]), int(self.ring[1]))
        self.lengths = np.ascontiguousarray(self.lengths, np.int32).reshape(-1)
        M, S = int(self.lengths.sum()), self.S
        if self.lengths.size and (self.lengths.min() < 1 or self.lengths.max() > self.L):
            raise ValueError(f"game lengths outside [1, {self.L}]")
        if len(self.lengths) > self.C:
            raise ValueError(f"{len(self.lengths)} games in a ring of {self.C}")
        for name, dtype, shape in (("rewards", np.float32, (M,)), ("tokens", np.int8, (M, 3 * S)),
                                   ("frames", np.int8, (M, self.T, S, S, S))):
            a = np.asarray(getattr(self, name))
            if a.dtype != dtype or a.shape != shape:
                raise ValueError(f"{name} must be {np.dtype(dtype).name} {shape}, got {a.dtype} {a.shape}")
            setattr(self, name, np.ascontiguousarray(a))

    @property
    def G(self) -> int:
        return len(self.lengths)

    @property
    def M(self) -> int:
        return len(self.rewards)

    def slots(self) -> np.ndarray:
        """The slot of every game in a ring whose stored games are consecutive (what the adds leave): the newest sits
        just before ring[0]."""
        return (self.ring[0] - self.G + np.arange(self.G)) % self.C

    def starts(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.lengths, dtype=np.int64)])

    def equals(self, other: "PackedGames") -> bool:
        return (self.C, self.L, self.T, self.S, self.ring) == (other.C, other.L, other.T, other.S, other.ring) and all(
            np.array_equal(getattr(self, k), getattr(other, k), equal_nan=k == "rewards")
            for k in ("lengths", "rewards", "tokens", "frames"))


# ---- the buffer file ---------------------------------------------------------------------------------------------------
def _read_exact(f, n: int, what: str) -> bytes:
    raw = f.read(n)
    if len(raw) != n:
        raise ValueError(f"{what}: truncated ({len(raw)} of {n} bytes)")
    return raw


def _array(f, dtype, shape, what: str) -> np.ndarray:
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return np.frombuffer(_read_exact(f, n, what), dtype=np.dtype(dtype).newbyteorder("<")).astype(dtype).reshape(shape)


def _bytes(a: np.ndarray, dtype) -> bytes:
    return np.ascontiguousarray(a, dtype=np.dtype(dtype).newbyteorder("<")).tobytes()


def write_games(f, p: PackedGames) -> None:
    """One buffer, header and arrays, to a binary file object."""
    f.write(HEADER.pack(MAGIC, p.C, p.L, p.T, p.S, p.G, p.M, p.ring[0], p.ring[1], *([0] * 7)))
    f.write(_bytes(p.lengths, np.int32))
    f.write(_bytes(p.rewards, np.float32))
    f.write(p.tokens.tobytes())
    f.write(p.frames.tobytes())


def read_games(f, what: str = "replay buffer") -> PackedGames:
    """The buffer ``write_games`` wrote at the file object's position.  ValueError for a wrong magic, a header that does
    not describe a buffer, or a file that ends early."""
    magic, C, L, T, S, G, M, r0, r1, *_ = HEADER.unpack(_read_exact(f, HEADER.size, what))
    if magic != MAGIC:
        raise ValueError(f"{what}: not a packed replay buffer")
    if min(C, L, T, S) < 1 or not 0 <= G <= C or not G <= M <= G * L or not 0 <= r0 < C or r1 < 0:
        raise ValueError(f"{what}: inconsistent header (C={C} L={L} T={T} S={S} G={G} M={M} ring=({r0},{r1}))")
    lengths = _array(f, np.int32, (G,), what)
    if int(lengths.sum(dtype=np.int64)) != M:
        raise ValueError(f"{what}: the lengths sum to {int(lengths.sum(dtype=np.int64))}, the header says M={M}")
    return PackedGames(C, L, T, S, (r0, r1), lengths, _array(f, np.float32, (M,), what),
                       _array(f, np.int8, (M, 3 * S), what), _array(f, np.int8, (M, T, S, S, S), what))


def save_games(path, p: PackedGames) -> None:
    with open(path, "wb") as f:
        write_games(f, p)


def load_games(path) -> PackedGames:
    """The one buffer of a file ``save_games`` wrote; the file must end where the header says."""
    with open(path, "rb") as f:
        p = read_games(f, str(path))
        if f.read(1):
            raise ValueError(f"{path}: longer than its header says")
    return p


# ---- the reference's layout -------------------------------------------------------------------------------------------
def export_reference_games(save_dir, p: PackedGames, n_logits: int) -> Tuple[Dict[int, int], int]:
    """Write the files a reference ``PlayedGamesDataset`` reads (datasets.py:196-208), slot i = file i:
    ``state_seq_{i}.pt`` a list of float32 (T,S,S,S), ``action_seq_{i}.pt`` a list of float32 (3S,n_logits) one-hot
    rows (their ``argmax(-1)`` is the stored token) and ``reward_seq_{i}.pt`` float32 (n,).  Returns (game_lengths,
    game_pointer) to install on that dataset.  The reference walks slots from 0, so the ring must hold its games in
    slots 0 .. G-1 (any ring the adds filled does)."""
    n_logits = int(n_logits)
    if p.M and not 0 <= int(p.tokens.min()) <= int(p.tokens.max()) < n_logits:
        raise ValueError(f"stored tokens outside [0, {n_logits})")
    slots, starts = p.slots(), p.starts()
    if sorted(slots.tolist()) != list(range(p.G)):
        raise ValueError("the reference walks slots from 0: the stored games must fill slots 0 .. G-1")
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    eye = torch.eye(n_logits, dtype=torch.float32)
    for r, slot in enumerate(slots.tolist()):
        lo, hi = int(starts[r]), int(starts[r + 1])
        frames = torch.from_numpy(p.frames[lo:hi].astype(np.float32))
        tokens = torch.from_numpy(p.tokens[lo:hi].astype(np.int64))
        torch.save([frames[m].clone() for m in range(hi - lo)], save_dir / f"state_seq_{slot}.pt")
        torch.save([eye[tokens[m]].clone() for m in range(hi - lo)], save_dir / f"action_seq_{slot}.pt")
        torch.save(torch.from_numpy(p.rewards[lo:hi].copy()), save_dir / f"reward_seq_{slot}.pt")
    return {int(s): int(n) for s, n in sorted(zip(slots.tolist(), p.lengths.tolist()))}, p.ring[0]


def import_reference_games(save_dir, game_lengths: Mapping[int, int], game_pointer: Optional[int] = None,
                           buffer_size: Optional[int] = None, max_actions: Optional[int] = None,
                           games_added: Optional[int] = None) -> PackedGames:
    """Read the games a reference ``PlayedGamesDataset`` wrote (its ``game_lengths``; ``game_pointer`` and
    ``buffer_size`` default to a ring that has not wrapped) into the dense form, oldest first: the argmax tokens of the
    stored policies (datasets.py:206) and the frames as int8.  Values that do not fit int8 are refused."""
    save_dir = Path(save_dir)
    G = len(game_lengths)
    C = int(buffer_size) if buffer_size is not None else max(G, 1)
    pointer = int(game_pointer) if game_pointer is not None else G % C
    if sorted(int(s) for s in game_lengths) != list(range(G)) or G > C:
        raise ValueError("game_lengths must hold slots 0 .. G-1 of a ring of buffer_size")
    lengths, frames, tokens, rewards = [], [], [], []
    for slot in ((pointer - G + np.arange(G)) % C).tolist():
        n = int(game_lengths[slot])
        st = torch.load(save_dir / f"state_seq_{slot}.pt")
        ac = torch.load(save_dir / f"action_seq_{slot}.pt")
        rw = torch.load(save_dir / f"reward_seq_{slot}.pt")
        f = torch.stack([torch.as_tensor(x) for x in st]).to(torch.float32) if not isinstance(st, torch.Tensor) else st
        a = torch.stack([torch.as_tensor(x) for x in ac]) if not isinstance(ac, torch.Tensor) else ac
        r = torch.stack([torch.as_tensor(x).reshape(()) for x in rw]) if not isinstance(rw, torch.Tensor) else rw
        if not (len(f) == len(a) == r.numel() == n) or n < 1:
            raise ValueError(f"game {slot}: {len(f)} states, {len(a)} policies, {r.numel()} rewards for length {n}")
        if float(f.abs().max()) > 127 or not torch.equal(f, f.round()):
            raise ValueError(f"game {slot}: its frames do not fit int8")
        tok = a.argmax(dim=-1)
        if int(tok.max()) > 127:
            raise ValueError(f"game {slot}: its tokens do not fit int8")
        lengths.append(n)
        frames.append(f.to(torch.int8).numpy())
        tokens.append(tok.to(torch.int8).numpy())
        rewards.append(r.reshape(-1).to(torch.float32).numpy())
    if not G:
        raise ValueError("no games: the shapes of an empty reference buffer are unknown")
    T, S = frames[0].shape[1], frames[0].shape[2]
    L = int(max_actions) if max_actions is not None else max(lengths)
    return PackedGames(C, L, T, S, (pointer, G if games_added is None else games_added), np.array(lengths, np.int32),
                       np.concatenate(rewards), np.concatenate(tokens), np.concatenate(frames))


# ---- the dataset file -------------------------------------------------------------------------------------------------
def save_dataset(path, d: Mapping) -> None:
    """The host state of a ``TensorGameData`` (``TensorGameData.save`` collects it) to one file.  ``d``: len_data,
    dim_t, shift, R, S, n_demos, fract_synth, fract_best, targets_hash, is_synth bool (len_data,), index_synth int64,
    index_played / index_best int64 or None, generator uint8 (the device generator's state), played / best
    ``PackedGames``, tokens / targets int8 or None (both: the demos are not stored)."""
    has_demos = d["tokens"] is not None
    n = lambda x: -1 if x is None else len(x)
    idx = lambda x: b"" if x is None else _bytes(x, np.int64)
    gen = np.ascontiguousarray(d["generator"], np.uint8)
    with open(path, "wb") as f:
        f.write(DATA_HEADER.pack(DATA_MAGIC, d["len_data"], d["dim_t"], d["shift"], d["R"], d["S"], d["n_demos"],
                                 int(has_demos), n(d["index_synth"]), n(d["index_played"]), n(d["index_best"]),
                                 gen.size, int(d["targets_hash"]), 0, float(d["fract_synth"]), float(d["fract_best"])))
        f.write(np.ascontiguousarray(d["is_synth"], np.uint8).tobytes())
        for key in ("index_synth", "index_played", "index_best"):
            f.write(idx(d[key]))
        f.write(gen.tobytes())
        write_games(f, d["played"])
        write_games(f, d["best"])
        if has_demos:
            f.write(np.ascontiguousarray(d["tokens"], np.int8).tobytes())
            f.write(np.ascontiguousarray(d["targets"], np.int8).tobytes())


def load_dataset(path) -> dict:
    """The dict ``save_dataset`` took.  ValueError for a wrong magic, a truncated or an overlong file."""
    what = str(path)
    with open(path, "rb") as f:
        (magic, len_data, dim_t, shift, R, S, n_demos, has_demos, n_synth, n_played, n_best, n_gen, thash, _,
         fract_synth, fract_best) = DATA_HEADER.unpack(_read_exact(f, DATA_HEADER.size, what))
        if magic != DATA_MAGIC:
            raise ValueError(f"{what}: not a saved TensorGameData")
        if min(len_data, n_demos, n_synth, n_gen) < 0 or min(dim_t, R, S) < 1 or min(n_played, n_best) < -1:
            raise ValueError(f"{what}: inconsistent header")
        d = dict(len_data=len_data, dim_t=dim_t, shift=shift, R=R, S=S, n_demos=n_demos, targets_hash=thash,
                 fract_synth=fract_synth, fract_best=fract_best)
        d["is_synth"] = _array(f, np.uint8, (len_data,), what).astype(bool)
        for key, k in (("index_synth", n_synth), ("index_played", n_played), ("index_best", n_best)):
            d[key] = None if k < 0 else _array(f, np.int64, (k,), what)
        d["generator"] = _array(f, np.uint8, (n_gen,), what)
        d["played"] = read_games(f, what + " (played)")
        d["best"] = read_games(f, what + " (best)")
        d["tokens"] = _array(f, np.int8, (n_demos, R, 3 * S), what) if has_demos else None
        d["targets"] = _array(f, np.int8, (n_demos, S, S, S), what) if has_demos else None
        if f.read(1):
            raise ValueError(f"{what}: longer than its header says")
    return d


# ---- a whole run ------------------------------------------------------------------------------------------------------
class RunState(NamedTuple):
    """What ``load_run`` returns: the rebuilt trainer and dataset, the optimizer's ``state_dict`` (host tensors, for
    ``optimizer.load_state_dict`` of an optimizer over ``trainer.params``), the named device generators, ``extra``."""

    trainer: object
    optimizer_state: Optional[dict]
    data: object
    generators: Dict[str, torch.Generator]
    extra: object


def _gpu(device, fn: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise TensorGameError(fn, -1, f"a run lives on a ROCm device (got {dev}); there is no CPU path")
    return dev


def save_run(path, trainer, optimizer, data, generators: Optional[Mapping[str, torch.Generator]] = None,
             extra=None) -> None:
    """Everything a train / act / replay loop needs to continue, into the directory ``path``: ``trainer.pt`` (the
    ``FusedTrainer.checkpoint()``, ``optimizer.state_dict()``, the states of the named device ``generators`` -- the
    batch loader's, for instance -- and ``extra``: plain scalars, strings, tensors and containers of them) through
    ``torch.save``, and ``data.tgd`` (``TensorGameData.save``).  One host copy of each; the device is synchronised."""
    generators = dict(generators or {})
    for name, g in generators.items():
        _gpu(g.device, f"save_run (generator {name!r})")
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    cpu = lambda x: x.detach().cpu() if isinstance(x, torch.Tensor) else x
    opt = None
    if optimizer is not None:
        sd = optimizer.state_dict()
        opt = {"state": {k: {n: cpu(v) for n, v in s.items()} for k, s in sd["state"].items()},
               "param_groups": sd["param_groups"]}
    torch.save({"trainer": trainer.checkpoint(), "optimizer": opt,
                "generators": {name: g.get_state() for name, g in generators.items()}, "extra": extra},
               path / "trainer.pt")
    data.save(path / "data.tgd")


def load_run(path, device) -> RunState:
    """The run ``save_run`` wrote, rebuilt on ``device``.  ``trainer.pt`` is read with ``weights_only=True``."""
    from .replay import TensorGameData
    from .train import FusedTrainer, SlicedTrainer, SlicedTrainer25

    dev = _gpu(device, "load_run")
    path = Path(path)
    d = torch.load(path / "trainer.pt", map_location="cpu", weights_only=True)
    gens = {}
    for name, state in d["generators"].items():
        gens[name] = torch.Generator(device=dev)
        gens[name].set_state(state)
    # the class the checkpoint names; a file without the key is a FusedTrainer's
    kinds = {"fused": FusedTrainer, "sliced": SlicedTrainer, "sliced25": SlicedTrainer25}
    cls = kinds[d["trainer"].get("kind", "fused")]
    return RunState(cls.from_checkpoint(d["trainer"], dev), d["optimizer"],
                    TensorGameData.load(path / "data.tgd", dev), gens, d["extra"])
