#!/usr/bin/env python3
"""Golden fixture for the replay buffers and the mixed dataset (include/tensor_game_replay.h, mat_mul_amd.replay),
recorded by RUNNING THE REFERENCE's ``PlayedGamesDataset`` and ``TensorGameDataset`` (/root/reference/datasets.py) in a
temporary directory.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_replay.py      (build container only)

Stored:
  ring_<c>_*   (c = S4_T2, S16_T1: games of search_games.npz, then hand-made policies with tied maxima and NaN)
      states int8 (A,L,T,S,S,S), policy f32 (A,L,3S,n_logits), rewards f32 (A,L), lengths int64 (A,): the games added,
      one add_game per game, to a PlayedGamesDataset of buffer_size 3 (it wraps);
      snap<a>_frames int8 (n,T,S,S,S), snap<a>_scalar f32 (n,), snap<a>_action int64 (n,3S), snap<a>_reward f32 (n,):
      every __getitem__ after add a;
  best_<i>_rewards f32 (G,L), best_<i>_lengths int64 (G,), best_<i>_pick int64: the game act_step's loop
      (training.py:468-483, reward_seq[-1] > best_reward from -1e6) picks, -1 for none;
  mix_*: a TensorGameDataset (len_data 40, max_actions 4, dim_t 2, S 4): its synthetic demos read back from its save dir
      (mix_tokens int64 (40,4,12), mix_targets f32 (40,4,4,4)), the games added (mix_states, mix_policy, mix_rewards,
      mix_lengths; the first 3 to the played buffer, the last to the best buffer), and per state <k> (0 played buffer
      empty, 1 played only, 2 best present with fract_best > 0, 3 played with replacement): is_synth, index_synth,
      index_played / index_best (with has_played / has_best), fract (fract_synth, fract_best) and every __getitem__
      (frames f32 (40,2,4,4,4), scalar, action int64 (40,12), reward).
The archive is written deterministically (fixed member order and time stamps), so a rerun reproduces it byte for byte.
Nothing of the reference is copied.
"""
import io
import os
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
OUT = HERE / "replay_cases.npz"


def tied_policy(rng, L, A3, n_logits, kind):
    """Hand-made policies: 'tie' = equal maxima at several indices, 'nan' = a NaN somewhere in some rows."""
    p = rng.integers(0, 3, size=(L, A3, n_logits)).astype(np.float32) / 4
    if kind == "tie":
        p[..., :] = np.float32(0.25)
        p[::2, ::3, 1:] = np.float32(0.5)  # first maximum at 1, tied with 2
    else:
        p[1::2, ::2, 2] = np.nan
        p[0, 0, :] = np.nan                 # NaN everywhere: argmax 0
    return p


def ring_case(torch, datasets, name, g, rng):
    S, T = int(g[f"{name}_meta"][0]), int(g[f"{name}_meta"][1])
    states, policy = g[f"{name}_states"], g[f"{name}_policy"]
    rewards, lengths = g[f"{name}_rewards"].astype(np.float32), g[f"{name}_lengths"]
    L, A3, nl = policy.shape[1], policy.shape[2], policy.shape[3]
    games = [(states[i], policy[i], rewards[i], int(lengths[i])) for i in range(len(lengths))]
    for kind in ("tie", "nan", "tie"):
        i = len(games) % len(lengths)
        games.append((states[i], tied_policy(rng, L, A3, nl, kind), rewards[i], int(lengths[i])))
    buf = datasets.PlayedGamesDataset(3, "cpu", save_dir=f"ring_{name}")
    out = {}
    for a, (st, po, rw, n) in enumerate(games):
        buf.add_game([torch.from_numpy(st[m].astype(np.float32)) for m in range(n)], torch.from_numpy(po[:n]),
                     torch.from_numpy(rw[:n]))
        items = [buf[i] for i in range(len(buf))]
        out[f"ring_{name}_snap{a}_frames"] = np.stack([it[0].numpy() for it in items]).astype(np.int8)
        out[f"ring_{name}_snap{a}_scalar"] = np.array([it[1].item() for it in items], np.float32)
        out[f"ring_{name}_snap{a}_action"] = np.stack([it[2].numpy() for it in items]).astype(np.int64)
        out[f"ring_{name}_snap{a}_reward"] = np.array([it[3].item() for it in items], np.float32)
    out[f"ring_{name}_states"] = np.stack([x[0] for x in games])
    out[f"ring_{name}_policy"] = np.stack([x[1] for x in games])
    out[f"ring_{name}_rewards"] = np.stack([x[2] for x in games])
    out[f"ring_{name}_lengths"] = np.array([x[3] for x in games], np.int64)
    return out


def best_cases(torch):
    """act_step's selection loop over a batch of games, on torch tensors as the reference compares them."""
    L = 4
    batches = [
        (np.array([[-1, -2, -5, 0], [-1, -2, -3, 0], [-1, -2, -3, 0], [-1, -9, 0, 0]], np.float32), [3, 3, 3, 2]),
        (np.array([[-1, -4, 0, 0], [-2, -4, 0, 0], [-7, 0, 0, 0]], np.float32), [2, 2, 1]),
        (np.array([[-1, np.nan, 0, 0], [-1, -3, -2e6, 0], [-1, -1e6, 0, 0]], np.float32), [2, 3, 2]),
        (np.array([[-1, -2, -3, -4], [-1, -2, -3, -4.5]], np.float32), [4, 4]),
    ]
    out = {}
    for i, (rw, ln) in enumerate(batches):
        best_reward, best = -1e6, -1
        for gi in range(len(ln)):
            reward_seq = torch.from_numpy(rw[gi, :ln[gi]])
            if reward_seq[-1] > best_reward:
                best_reward, best = reward_seq[-1], gi
        out[f"best_{i}_rewards"], out[f"best_{i}_lengths"] = rw, np.array(ln, np.int64)
        out[f"best_{i}_pick"] = np.array(best, np.int64)
    return out


def mixture(torch, datasets, g):
    name = "S4_T2_lowrank"
    states, policy = g[f"{name}_states"], g[f"{name}_policy"]
    rewards, lengths = g[f"{name}_rewards"].astype(np.float32), g[f"{name}_lengths"]
    ds = datasets.TensorGameDataset(40, 0.9, 4, 2, 4, "cpu")
    out = {"mix_tokens": np.stack([np.stack([a.numpy() for a in torch.load(ds.buffer_synth.save_dir / f"action_seq_{i}.pt")])
                                   for i in range(40)]).astype(np.int64),
           "mix_targets": np.stack([torch.load(ds.buffer_synth.save_dir / f"target_tensor_{i}.pt").numpy()
                                    for i in range(40)]).astype(np.float32),
           "mix_states": states, "mix_policy": policy, "mix_rewards": rewards, "mix_lengths": lengths}

    def game(i):
        n = int(lengths[i])
        return ([torch.from_numpy(states[i, m].astype(np.float32)) for m in range(n)], torch.from_numpy(policy[i, :n]),
                torch.from_numpy(rewards[i, :n]))

    def record(k):
        out[f"mix_{k}_is_synth"] = ds.is_synth.numpy().astype(bool)
        out[f"mix_{k}_index_synth"] = ds.index_synth.numpy().astype(np.int64)
        for key in ("played", "best"):
            idx = getattr(ds, f"index_{key}")
            out[f"mix_{k}_has_{key}"] = np.array(idx is not None)
            out[f"mix_{k}_index_{key}"] = np.zeros(0, np.int64) if idx is None else idx.numpy().astype(np.int64)
        out[f"mix_{k}_fract"] = np.array([ds.fract_synth, ds.fract_best], np.float64)
        items = [ds[x] for x in range(len(ds))]
        out[f"mix_{k}_frames"] = np.stack([it[0].numpy() for it in items]).astype(np.float32)
        out[f"mix_{k}_scalar"] = np.array([it[1].item() for it in items], np.float32)
        out[f"mix_{k}_action"] = np.stack([it[2].numpy() for it in items]).astype(np.int64)
        out[f"mix_{k}_reward"] = np.array([it[3].item() for it in items], np.float32)

    ds.resample_buffer_indexes()            # 0: the played buffer is empty: nothing changes
    record(0)
    for i in range(3):
        ds.add_played_game(*game(i))
    ds.resample_buffer_indexes()            # 1: played only, few items: without replacement
    record(1)
    ds.add_best_game(*game(3))
    ds.set_fractions(0.5, 0.2)
    ds.resample_buffer_indexes()            # 2: best present, fract_best > 0: every non-synthetic item is a best item
    record(2)
    ds.set_fractions(0.2, 0.0)
    ds.resample_buffer_indexes()            # 3: played only again, more items than moves: with replacement
    record(3)
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member order and time stamps: reruns are byte-identical."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, member.getvalue())
    Path(path).write_bytes(buf.getvalue())


def main(out_path=OUT):
    sys.dont_write_bytecode = True
    g = np.load(HERE / "search_games.npz")
    os.chdir(tempfile.mkdtemp(prefix="golden_replay_"))
    sys.path.insert(0, REF)
    import torch

    torch.manual_seed(0)
    np.random.seed(0)
    import datasets  # noqa: E402  (reference)

    rng = np.random.default_rng(7)
    arrays = {}
    for name in ("S4_T2", "S16_T1"):
        arrays.update(ring_case(torch, datasets, name, g, rng))
    arrays.update(best_cases(torch))
    arrays.update(mixture(torch, datasets, g))
    write_npz(out_path, arrays)
    print(f"wrote {out_path} ({Path(out_path).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
