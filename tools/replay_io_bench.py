"""GameBuffer.pack (tg_replay_pack) on a played buffer, beside the torch restatement of the same gather.

    python tools/replay_io_bench.py OUT_DIR [--reps 30] [--warmup 5]

One process, one GPU.  Per config (S=4 T=2 L=8 and S=16 T=2 L=48, each C = 4096 slots holding games of L/2 moves, the
ring wrapped so ring[0] != 0), HIP events around each call after warm-up; median, p10 and p90 over --reps calls
(microseconds), the two alternating:
  pack:  GameBuffer.pack(): one host sync for (G, M), the exact allocation, one tg_replay_pack call (plan + copy);
  call:  ops.replay_pack into preallocated outputs: the two launches alone;
  torch: the restatement: the slots in age order, a boolean mask over (C, L), and one masked index per array.
bytes = the stored moves read once and written once: 2 * M * (T*S^3 + 3S + 4).  The outputs of the three are compared.
Writes OUT_DIR/r16_replay_io.json.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mat_mul_amd import GameBuffer, ops  # noqa: E402

DEV = "cuda:0"
CONFIGS = [("S4_T2_L8", 4, 2, 8), ("S16_T2_L48", 16, 2, 48)]  # name, S, T, L
C = 4096


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def summary(out):
    out = sorted(out)
    return {"median_us": statistics.median(out), "p10_us": out[len(out) // 10], "p90_us": out[(9 * len(out)) // 10],
            "n": len(out)}


def played_buffer(S, T, L, gen):
    """C + C/4 games of L/2 moves through add_packed: a full ring whose oldest game sits at slot C/4."""
    buf = GameBuffer(C, L, T, S, DEV)
    n = L // 2
    for G in (C, C // 4):
        M = G * n
        buf.add_packed(torch.randint(-2, 3, (M, T, S, S, S), generator=gen, device=DEV, dtype=torch.int8),
                       torch.randint(0, 3, (M, 3 * S), generator=gen, device=DEV, dtype=torch.int8),
                       -torch.rand((M,), generator=gen, device=DEV), torch.full((G,), n, dtype=torch.int32, device=DEV))
    return buf


def torch_pack(buf):
    order = (buf.ring[0] + torch.arange(buf.C, device=buf.device)) % buf.C
    length = buf.length[order]
    mask = torch.arange(buf.L, device=buf.device)[None] < length[:, None]
    return buf.frames[order][mask], buf.tokens[order][mask], buf.rewards[order][mask], length[length > 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "replay_io_bench needs the MI355X"
    gen = torch.Generator(device=DEV).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "C": C, "configs": {}}
    for name, S, T, L in CONFIGS:
        buf = played_buffer(S, T, L, gen)
        M = len(buf)
        pre = ops.replay_pack(buf, M)
        runs = {"pack": buf.pack, "call": lambda: ops.replay_pack(buf, M, *pre), "torch": lambda: torch_pack(buf)}
        got, ref = buf.pack(), torch_pack(buf)
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got[:4], ref)) and all(
            torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(pre[:3], ref))
        for fn in runs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(event_time(fn))
        nbytes = 2 * M * (T * S ** 3 + 3 * S + 4)
        entry = {"S": S, "T": T, "L": L, "games": int((buf.length > 0).sum()), "moves": M, "ring0": int(buf.ring[0]),
                 "bytes": nbytes, "outputs_equal": bool(same)}
        for k in runs:
            entry[k] = summary(times[k])
            entry[k]["GB_per_s"] = nbytes / entry[k]["median_us"] / 1e3
        result["configs"][name] = entry
        print(name, json.dumps(entry))
        del buf, pre, got, ref
        torch.cuda.empty_cache()
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r16_replay_io.json").write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
