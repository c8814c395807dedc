#!/usr/bin/env python3
"""Golden fixture for move lists stored as games (include/tensor_game_replay_lists.h), recorded by RUNNING THE
REFERENCE: every list is played from (target, zero history) with the chain of ``get_child_states`` (act.py:266-275),
``get_rank`` (utils.py:134-140) of the end state gives the end reward of ``reward_seq`` (act.py:59-62), and the game goes
through ``PlayedGamesDataset.add_game`` and every ``__getitem__`` (datasets.py:161-230) in a temporary directory.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_replay_lists.py      (build container only)

The lists are fixtures the repository already has: the 7 Strassen actions of strassen.npz and demos of
synthetic_demos.npz (a demo's action list factorises its own target by construction).  Stored, per case <c>:
  <c>_starts int8 (A,T,S,S,S) (frame 0 the target, the history zero), <c>_tokens int8 (A,K,3S) (zero behind a list),
  <c>_lengths int64 (A,), <c>_rank int64 (A,) (get_rank of every end state: 0), <c>_rewards f32 (A,K) (reward_seq);
  <c>_snap<a>_frames int8 (n,T,S,S,S), _scalar f32 (n,), _action int64 (n,3S), _reward f32 (n,): every __getitem__ of a
  PlayedGamesDataset of buffer_size 3 (it wraps) after add a (S4_T2: every add; S9_T4: the adds in SNAPS).
The archive is written deterministically (fixed member order and time stamps), so a rerun reproduces it byte for byte.
Nothing of the reference is copied.
"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_golden_replay import REF, write_npz  # noqa: E402

OUT = HERE / "replay_lists_cases.npz"
CASES = {  # name -> (T, [(file, key of the tokens, key of the target)]), snapshots after these adds
    "S4_T2": (2, [("strassen", "tokens", "tensor")] + [("synthetic_demos", f"fn_S4_R7_{i}_tokens", f"fn_S4_R7_{i}_target")
                                                       for i in range(4)], range(5)),
    "S9_T4": (4, [("synthetic_demos", f"fn_S9_R12_{i}_tokens", f"fn_S9_R12_{i}_target") for i in range(3)] +
              [("synthetic_demos", "ds_S9_R10_T4_0_tokens", "ds_S9_R10_T4_0_target")], (2, 3)),
}


def play(torch, act, utils, target, tokens, T):
    """The reference's own moves: (state_seq, reward_seq, rank of the end state)."""
    S = target.shape[0]
    state = torch.cat([torch.from_numpy(target.astype(np.float32))[None, None], torch.zeros(1, T - 1, S, S, S)], dim=1)
    state_seq = []
    for tok in tokens:
        state_seq.append(state[0])
        state = act.get_child_states(state, torch.from_numpy(tok.astype(np.int64))[None, None])[0]
    rank = utils.get_rank(state)
    reward_seq = torch.cumsum(torch.tensor([-1] * (len(tokens) - 1) + [-1 - rank]), dim=0)
    return state_seq, reward_seq, rank


def case(torch, act, utils, datasets, name, T, lists, snaps):
    files = {f: np.load(HERE / f"{f}.npz") for f in {x[0] for x in lists}}
    games = [(files[f][tk], files[f][tg]) for f, tk, tg in lists]
    K, S = max(len(tk) for tk, _ in games), games[0][1].shape[0]
    out = {f"{name}_starts": np.zeros((len(games), T, S, S, S), np.int8),
           f"{name}_tokens": np.zeros((len(games), K, 3 * S), np.int8),
           f"{name}_lengths": np.array([len(tk) for tk, _ in games], np.int64),
           f"{name}_rank": np.zeros(len(games), np.int64), f"{name}_rewards": np.zeros((len(games), K), np.float32)}
    buf = datasets.PlayedGamesDataset(3, "cpu", save_dir=f"lists_{name}")
    for a, (tk, target) in enumerate(games):
        out[f"{name}_starts"][a, 0], out[f"{name}_tokens"][a, :len(tk)] = target, tk
        state_seq, reward_seq, rank = play(torch, act, utils, target, tk, T)
        out[f"{name}_rank"][a], out[f"{name}_rewards"][a, :len(tk)] = rank, reward_seq.numpy()
        one_hot = torch.nn.functional.one_hot(torch.from_numpy(tk.astype(np.int64)), int(tk.max()) + 1).float()
        buf.add_game(state_seq, one_hot, reward_seq.float())
        if a in snaps:
            items = [buf[i] for i in range(len(buf))]
            out[f"{name}_snap{a}_frames"] = np.stack([it[0].numpy() for it in items]).astype(np.int8)
            out[f"{name}_snap{a}_scalar"] = np.array([it[1].item() for it in items], np.float32)
            out[f"{name}_snap{a}_action"] = np.stack([it[2].numpy() for it in items]).astype(np.int64)
            out[f"{name}_snap{a}_reward"] = np.array([it[3].item() for it in items], np.float32)
    return out


def main(out_path=OUT):
    sys.dont_write_bytecode = True
    os.chdir(tempfile.mkdtemp(prefix="golden_replay_lists_"))
    sys.path.insert(0, REF)
    import torch

    import act  # noqa: E402  (reference)
    import datasets  # noqa: E402  (reference)
    import utils  # noqa: E402  (reference)

    arrays = {}
    for name, (T, lists, snaps) in CASES.items():
        arrays.update(case(torch, act, utils, datasets, name, T, lists, snaps))
    write_npz(out_path, arrays)
    print(f"wrote {out_path} ({Path(out_path).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
