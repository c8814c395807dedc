"""tg_lift2_signs (include/tensor_game_lift.h): time per list and per try, and the share of Z_2 walks that lift.

    python tools/lift_bench.py OUT_DIR [--reps 5] [--warmup 1] [--walk-steps 10000] [--rate-steps 100000] [--rate-walks 1024]
    python tools/lift_bench.py OUT_DIR --resources      (no GPU: where the library was built, its objects are at hand)

One process, one GPU.  Lists: the best lists of Z_2 walks (``Mod2Walks``, seed 0) from the standard algorithms of
<2,2,2> (S=4, K=8), <3,3,3> (S=9, K=27) and <4,4,4> (S=16, K=64), ``--walk-steps`` steps each; the targets are the integer
matmul tensors.  Timing: W in {256, 4 096} lists, tries in {1, 32}, one ``ops.lift2_signs`` launch between HIP events,
after warm-up: median, p10, p90 in microseconds, microseconds per list, and per list and try offered (a list stops at its
first exact try, so ``tries_run_mean`` says how many ran).  Also the workspace bytes used, the status counts, the
kernels' VGPRs, LDS and scratch from the code object, and, for context only, the seconds the numpy restatement
(tests/lift_ref.py) takes on the host for 8 of the same lists.  Lift rate: ``--rate-walks`` walks of ``--rate-steps``
steps at each size, without and with ``plus_after=10_000``: status counts, and the ranks that lifted.  Writes
OUT_DIR/lift_bench.json.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from collections import Counter
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from flips_bench import object_resources, standard_matmul, stats  # noqa: E402
from mat_mul_amd import Mod2Walks, build, flips, lift, ops  # noqa: E402

DEV = "cuda:0"


def walked(n, W, steps, plus_after=0):
    """(Mod2Walks after ``steps`` steps, the integer target int8 (W,S,S,S)) of W walks from the standard <n,n,n> list."""
    tokens = torch.as_tensor(standard_matmul(n)[None]).to(DEV)
    lengths = torch.tensor([n ** 3], dtype=torch.int64, device=DEV)
    walks = Mod2Walks.start(tokens, lengths, walks_per_list=W, seed=0, plus_after=plus_after).advance(steps)
    S = n * n
    return walks, flips.term_sum(tokens, lengths, 1).expand(W, S, S, S).contiguous()


def status_counts(status):
    return {str(k): int(v) for k, v in sorted(Counter(status.cpu().tolist()).items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--walk-steps", type=int, default=10_000)
    ap.add_argument("--rate-steps", type=int, default=100_000)
    ap.add_argument("--rate-walks", type=int, default=1024)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    out_dir = Path(args.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    result = {"resources": object_resources(build.OBJ_DIR / "tg_lift.o")}
    if args.resources:
        print(json.dumps(result, indent=1))
        (out_dir / "lift_bench_resources.json").write_text(json.dumps(result, indent=1))
        return
    result.update(device=torch.cuda.get_device_name(0), timing=[], rate=[], host=[])
    for n in (2, 3, 4):
        S, K = n * n, n ** 3
        per_list = ops.lift2_workspace_bytes(K, S)
        for W in (256, 4096):
            walks, targets = walked(n, W, args.walk_steps)
            ws_lists = max(1, min(W, lift.MAX_WORKSPACE_BYTES // per_list, lift._RESIDENT_LISTS)) if per_list else 0
            ws = torch.empty((ws_lists * per_list,), dtype=torch.uint8, device=DEV) if per_list else None
            for tries in (1, 32):
                call = lambda: ops.lift2_signs(targets, walks.best, walks.best_rank, tries=tries, seed=0, workspace=ws,  # noqa: E731
                                               ws_lists=ws_lists)
                ts = []
                for rep in range(args.warmup + args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    _, out = call()
                    b.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ts.append(a.elapsed_time(b) * 1e3)
                st = stats(ts)
                used = out["try_used"][out["status"] == 0].float()
                ran = torch.where(out["status"] == 0, out["try_used"] + 1,
                                  torch.where(out["status"] == 3, torch.full_like(out["try_used"], tries), torch.zeros_like(out["try_used"])))
                row = {"n": n, "S": S, "K": K, "W": W, "tries": tries, **st, "us_per_list": st["median_us"] / W,
                       "us_per_list_per_try_offered": st["median_us"] / W / tries, "tries_run_mean": float(ran.float().mean()),
                       "workspace_bytes": ws_lists * per_list, "ws_lists": ws_lists, "status": status_counts(out["status"]),
                       "unknowns_mean": float(out["unknowns"].float().mean()), "sys_rank_mean": float(out["sys_rank"].float().mean()),
                       "try_used_mean_of_lifted": float(used.mean()) if used.numel() else None,
                       "best_rank_min": int(walks.best_rank.min()), "walk_steps": args.walk_steps}
                print(json.dumps(row), flush=True)
                result["timing"].append(row)
            if W == 256:                                            # the host restatement on 8 of the same lists
                import lift_ref as LR
                t0 = time.perf_counter()
                LR.lift(targets[:8].cpu().numpy(), walks.best[:8].cpu().numpy(), walks.best_rank[:8].cpu().numpy(), S, tries=32)
                row = {"n": n, "S": S, "lists": 8, "tries": 32, "numpy_seconds_per_list": (time.perf_counter() - t0) / 8}
                print(json.dumps(row), flush=True)
                result["host"].append(row)
        for plus_after in (0, 10_000):
            walks, targets = walked(n, args.rate_walks, args.rate_steps, plus_after)
            res = walks.lift(targets, tries=32)
            lifted = res.lifted
            row = {"n": n, "S": S, "K": K, "walks": args.rate_walks, "steps": args.rate_steps, "plus_after": plus_after,
                   "status": status_counts(res.status), "lifted_share": float(lifted.float().mean()),
                   "best_rank_hist": {str(k): int(v) for k, v in sorted(Counter(walks.best_rank.cpu().tolist()).items())},
                   "lifted_rank_hist": {str(k): int(v) for k, v in sorted(Counter(walks.best_rank[lifted].cpu().tolist()).items())},
                   "try_used_hist": {str(k): int(v) for k, v in sorted(Counter(res.try_used[lifted].cpu().tolist()).items())}}
            print(json.dumps(row), flush=True)
            result["rate"].append(row)
    (out_dir / "lift_bench.json").write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
