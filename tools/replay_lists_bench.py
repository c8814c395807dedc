"""tg_replay_add_lists (include/tensor_game_replay_lists.h) against the composed path on the same GPU.

    python tools/replay_lists_bench.py OUT_DIR [--reps 20] [--warmup 3] [--shapes 4,2,8,4096 25,2,8,256]

One process, one GPU.  Per shape S,T,K,M: M valid lists of K moves each (factor values from {-1,0,1}; a list's start is
the sum of its terms, the history frames are random) into a ring of M slots of K moves.  ``lists`` is
``ops.replay_add_lists``; ``composed`` is what a user had to write before it (tests/replay_lists_ref.composed_add): K
``TensorGameEnv.step`` calls, the frames stacked with the history shift, a one-hot float policy and ``ops.replay_add``.
Both are first compared through ``GameBuffer.pack`` bit for bit, then timed alternately with HIP events around the call
after warm-up (median, p10, p90 in microseconds).  ``stored_bytes`` = M K (T S^3 + 3 S + 4), the bytes of the games in
the ring; ``write_share`` = stored_bytes / lists.median_us over the HBM peak (8 TB/s): a figure for the whole call of four
launches, not for the emit kernel alone.  Writes OUT_DIR/replay_lists_bench.json.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from mat_mul_amd import GameBuffer, ops  # noqa: E402
import replay_lists_ref as LR  # noqa: E402
from solutions_bench import DEV, stats  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second


def lists_for(rng, S, T, K, M):
    tokens = rng.integers(0, 3, size=(M, K, 3 * S)).astype(np.int8)
    f = tokens.astype(np.int32).reshape(M, K, 3, S) - 1
    starts = rng.integers(-2, 3, size=(M, T, S, S, S)).astype(np.int8)
    starts[:, 0] = np.einsum("mki,mkj,mkl->mijl", f[:, :, 0], f[:, :, 1], f[:, :, 2]).astype(np.int8)
    return (torch.from_numpy(x).to(DEV) for x in (starts, tokens, np.full(M, K, np.int64)))


def timed_pair(fns, reps, warmup):
    """Both calls alternately, each between its own pair of events."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    return [stats(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["4,2,8,4096", "25,2,8,256"], help="S,T,K,M")
    args = ap.parse_args()
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "rows": []}
    for shape in args.shapes:
        S, T, K, M = (int(x) for x in shape.split(","))
        starts, tokens, lengths = lists_for(np.random.default_rng(S + M), S, T, K, M)
        a, b = GameBuffer(M, K, T, S, DEV), GameBuffer(M, K, T, S, DEV)
        stored = torch.zeros((M,), dtype=torch.uint8, device=DEV)
        new = lambda: ops.replay_add_lists(a, starts, tokens, lengths, stored=stored, status=a.status)  # noqa: E731
        old = lambda: LR.composed_add(b, starts, tokens, lengths)  # noqa: E731
        new(), old()
        assert bool(stored.all()) and int(a.status) == 0 == int(b.status)
        for x, y in zip(a.pack(), b.pack()):
            assert torch.equal(x, y), f"{shape}: the two paths differ"
        row = {"S": S, "T": T, "K": K, "M": M, "stored_bytes": M * K * (T * S ** 3 + 3 * S + 4)}
        row["lists"], row["composed"] = timed_pair((new, old), args.reps, args.warmup)
        row["speedup"] = row["composed"]["median_us"] / row["lists"]["median_us"]
        row["write_share"] = row["stored_bytes"] / (row["lists"]["median_us"] * 1e-6) / HBM_PEAK
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    out = Path(args.out) / "replay_lists_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
