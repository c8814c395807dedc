"""tg_replay_items and tg_replay_add at training shapes.

    python tools/replay_bench.py OUT_DIR [--reps 30] [--warmup 5]

One process, one GPU.  HIP events around each call after warm-up; median, p10 and p90 over --reps calls (microseconds).
  items: per config (S=4 R=7, T 1 and 2; S=16 R=49; S=25 R=64), per N in {256, 4096} and per mix (all synthetic,
         0.9 synthetic / 0.1 played, all played), one ops.replay_items call through an epoch table, against
         ops.demo_items on the same synthetic rows (the rows of the mix that are synthetic; all of them for the
         all-synthetic mix, where the two calls do the same work);
  add:   ops.replay_add of B = 4096 finished games at S=4, L=8, T=1 into a ring of C = 10 000 (every game, and the best
         one), and of B = 1 game at C = 10 000 and 65 536 -- the cost of the plan and the one-workgroup offset scan.
Writes OUT_DIR/r07_replay.json.
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

from mat_mul_amd import GameBuffer, SyntheticDemos, ops  # noqa: E402

DEV = "cuda:0"
# name, S, R, T, n_demos, played capacity (games of R moves)
CONFIGS = [("S4_T1", 4, 7, 1, 65536, 10000), ("S4_T2", 4, 7, 2, 65536, 10000), ("S16", 16, 49, 1, 8192, 256),
           ("S25", 25, 64, 1, 4096, 64)]
MIXES = [("all_synth", 1.0), ("synth0.9_played0.1", 0.9), ("all_played", 0.0)]


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out.sort()
    return {"median_us": statistics.median(out), "p10_us": out[len(out) // 10], "p90_us": out[(9 * len(out)) // 10],
            "n": len(out)}


def games(B, L, T, S, gen, n_logits=3):
    states = torch.randint(-2, 3, (B, L, T, S, S, S), generator=gen, device=DEV).to(torch.int8)
    policy = torch.rand((B, L, 3 * S, n_logits), generator=gen, device=DEV)
    rewards = -torch.arange(1, L + 1, device=DEV, dtype=torch.float32).repeat(B, 1)
    lengths = torch.full((B,), L, dtype=torch.int64, device=DEV)
    return states, policy, rewards, lengths


def items_rows(args, res):
    for name, S, R, T, n_demos, cap in CONFIGS:
        gen = torch.Generator(device=DEV).manual_seed(7)
        demos = SyntheticDemos.generate(n_demos, S, R, DEV, dim_t=T, seed=1)
        played = GameBuffer(cap, R, T, S, DEV)
        for lo in range(0, cap, 1024):
            played.add_games(*games(min(1024, cap - lo), R, T, S, gen))
        n_played = len(played)
        for N in (256, 4096):
            for mix, fs in MIXES:
                kind = (torch.rand((N,), generator=gen, device=DEV) >= fs).to(torch.uint8)
                src = torch.where(kind == 0, torch.randint(0, len(demos), (N,), generator=gen, device=DEV),
                                  torch.randint(0, n_played, (N,), generator=gen, device=DEV))
                idx = torch.randperm(N, generator=gen, device=DEV)
                out = torch.empty((N, T, S, S, S), dtype=torch.float32, device=DEV)
                sc, rw = torch.empty((N, 1), device=DEV), torch.empty((N, 1), device=DEV)
                ac = torch.empty((N, 3 * S), dtype=torch.int8, device=DEV)

                def mixed():
                    ops.replay_items(idx, T, S, DEV, tokens=demos.action_seq, targets=demos.target_tensor,
                                     played=played, kind=kind, src=src, out=out, scalars=sc, actions=ac, rewards=rw)

                syn_src = src[idx][kind[idx] == 0].contiguous()
                n_syn = syn_src.numel()
                row = {"config": name, "S": S, "R": R, "T": T, "N": N, "mix": mix, "synthetic_rows": n_syn,
                       "dtype": "float32", "replay_items": event_times(mixed, args.reps, args.warmup)}
                if n_syn:
                    o2 = torch.empty((n_syn, T, S, S, S), dtype=torch.float32, device=DEV)
                    s2, r2 = torch.empty((n_syn, 1), device=DEV), torch.empty((n_syn, 1), device=DEV)
                    a2 = torch.empty((n_syn, 3 * S), dtype=torch.int8, device=DEV)

                    def demo():
                        ops.demo_items(demos.action_seq, demos.target_tensor, syn_src, T, out=o2, scalars=s2,
                                       actions=a2, rewards=r2)

                    row["demo_items_same_synthetic_rows"] = event_times(demo, args.reps, args.warmup)
                    row["ratio_vs_demo_items"] = row["replay_items"]["median_us"] / \
                        row["demo_items_same_synthetic_rows"]["median_us"]
                res["items"].append(row)
                print(json.dumps({k: row[k] for k in ("config", "N", "mix")} |
                                 {"replay_us": round(row["replay_items"]["median_us"], 1),
                                  "demo_us": round(row.get("demo_items_same_synthetic_rows", {}).get("median_us", 0), 1)}),
                      flush=True)
        del demos, played
        torch.cuda.empty_cache()


def add_rows(args, res):
    gen = torch.Generator(device=DEV).manual_seed(11)
    S, L, T = 4, 8, 1
    big = games(4096, L, T, S, gen)
    one = games(1, L, T, S, gen)
    for label, C, batch, select in (("B4096_all", 10000, big, False), ("B4096_best", 10000, big, True),
                                    ("B1_all_C10000", 10000, one, False), ("B1_all_C65536", 65536, one, False)):
        buf = GameBuffer(C, L, T, S, DEV)
        row = {"case": label, "S": S, "L": L, "T": T, "C": C, "B": batch[0].shape[0], "select": int(select),
               "replay_add": event_times(lambda: ops.replay_add(buf, *batch, select=select), args.reps, args.warmup)}
        res["add"].append(row)
        print(json.dumps({"add": label, "us": round(row["replay_add"]["median_us"], 1)}), flush=True)
        del buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps, "items": [],
           "add": []}
    add_rows(args, res)
    items_rows(args, res)
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "r07_replay.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
