"""The fused training loss and gradient (include/tensor_game_train.h) against the float32 restatement run eagerly
(tests/train_ref.TrainRef: forward plus autograd backward), at the training app's configuration (net_ref.CONFIGS["a"]),
p = 0.5 dropout.

    python tools/train_bench.py OUT_DIR [--config a] [--reps 20] [--warmup 3] [--fused-only] [--kernel-stats CSV]

One process, one GPU.  Per B in {256, 1024, 4096}: FusedTrainer.loss_and_grad, the AdamW step on its parameter vector
(torch.optim.AdamW, foreach) plus the inference blob refresh, and the eager forward + backward, each timed with HIP
events around the call after warm-up; median, p10 and p90 in microseconds.  --fused-only runs the fused calls alone (for
a kernel-trace run); --kernel-stats merges a rocprofv3 --stats CSV into an existing OUT_DIR/r09_train.json.
Writes OUT_DIR/r09_train.json.  --config picks another configuration of net_ref.CONFIGS or tests/net_s9_ref.CONFIGS
(a9, b9: S = 9); the file is then OUT_DIR/r09_train_<config>.json.  --config a16 or b16 (tests/net_s16_ref.CONFIGS,
S = 16) times SlicedTrainer (include/tensor_game_train_sliced.h) at B in {16, 256} and writes
OUT_DIR/r13_train_<config>.json.  --config a25 or b25 (tests/net_s25_ref.CONFIGS, S = 25) times SlicedTrainer25
(include/tensor_game_train_s25.h) at B in {16, 64, 256} (--batches picks others) and writes
OUT_DIR/r18_train_<config>.json.
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from mat_mul_amd import FusedTrainer, SlicedTrainer, SlicedTrainer25  # noqa: E402
from net_ref import CONFIGS, make_weights  # noqa: E402
from net_s9_ref import CONFIGS as CONFIGS_S9  # noqa: E402
from net_s16_ref import CONFIGS as CONFIGS_S16  # noqa: E402
from net_s25_ref import RECORDED as NAMES_S25  # noqa: E402
from net_s25_ref import CONFIGS as CONFIGS_S25_ALL  # noqa: E402
from train_ref import TrainRef, keep_mask, make_batch, multipliers  # noqa: E402

CONFIGS_S25 = {k: CONFIGS_S25_ALL[k] for k in NAMES_S25}  # a25, b25
DEV = "cuda:0"
P_DROP = 0.5


def stats(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median_us": statistics.median(ts), "p10_us": q(0.1), "p90_us": q(0.9), "n": len(ts)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return stats(ts)


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "train_" in r.get("Name", ""):
                rows.append({"name": r["Name"], "calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"]),
                             "avg_ns": float(r["AverageNs"]), "percentage": float(r["Percentage"])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--config", default="a", choices=sorted({**CONFIGS, **CONFIGS_S9, **CONFIGS_S16, **CONFIGS_S25}))
    ap.add_argument("--batches", type=int, nargs="+", help="the batch sizes, in place of the configuration's")
    args = ap.parse_args()
    sliced, s25 = args.config in CONFIGS_S16, args.config in CONFIGS_S25
    out = Path(args.out) / ("r09_train.json" if args.config == "a" else
                            f"{'r18' if s25 else 'r13' if sliced else 'r09'}_train_{args.config}.json")
    if args.kernel_stats:
        res = json.loads(out.read_text())
        res["kernel_stats"] = kernel_stats(args.kernel_stats)
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["kernel_stats"], indent=1))
        return
    cfg = {**CONFIGS, **CONFIGS_S9, **CONFIGS_S16, **CONFIGS_S25}[args.config]
    sd = make_weights(cfg, 1)
    cls = SlicedTrainer25 if s25 else SlicedTrainer if sliced else FusedTrainer
    tr = cls.from_state_dict(sd, dropout_p=P_DROP, device=DEV)
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    res = {"config": args.config, "dropout_p": P_DROP, "torch": torch.__version__,
           "device": torch.cuda.get_device_name(0), "rows": []}
    for B in args.batches or ((16, 64, 256) if s25 else (16, 256) if sliced else (256, 1024, 4096)):
        batch = tuple(torch.from_numpy(x).to(DEV) for x in make_batch(cfg, B, B))
        row = {"B": B}
        row["fused_loss_grad"] = timed(lambda: tr.loss_and_grad(*batch), args.reps, args.warmup)

        def step():
            opt.step()
            tr.refresh()
        row["fused_adamw_refresh"] = timed(step, args.reps, args.warmup)
        row["fused_losses_only"] = timed(lambda: tr.losses(*batch), args.reps, args.warmup)
        if not args.fused_only:
            ref = TrainRef(sd, cfg, device=DEV, dtype=torch.float32)
            masks = torch.from_numpy(multipliers(keep_mask(0, 0, B, tr.config, P_DROP), P_DROP)).to(DEV, torch.float32)

            def eager():
                for v in ref.w.values():
                    v.grad = None
                lp, lv = ref.losses(*batch, masks=masks)
                (lp + 1000.0 * lv).backward()
            row["eager_fwd_bwd"] = timed(eager, args.reps, args.warmup)
            row["speedup"] = row["eager_fwd_bwd"]["median_us"] / row["fused_loss_grad"]["median_us"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    assert np.isfinite(tr.params.detach().cpu().numpy()).all()


if __name__ == "__main__":
    main()
