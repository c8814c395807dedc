"""tg_flip_advance (include/tensor_game_flips.h): time per step, and how far walks get.

    python tools/flips_bench.py OUT_DIR [--reps 5] [--warmup 1] [--hist-steps 100000]
    python tools/flips_bench.py OUT_DIR --resources      (no GPU: where the library was built, its objects are at hand)
    python tools/flips_bench.py OUT_DIR --plus-after N [--plus-slack M]    (tg_flip_advance_plus: walks with plus transitions)
    python tools/flips_bench.py OUT_DIR --mod2 [--plus-after N [--plus-slack M]]   (tg_flip2_advance: the walks over Z_2)

One process, one GPU.  Starting lists: the standard algorithms of <2,2,2> (S=4, K=8), <3,3,3> (S=9, K=27) and <4,4,4>
(S=16, K=64), bound 1, shift 1.  Timing: W in {256, 4 096, 65 536} walks from one list, n_steps = 4 096 per launch;
every repetition starts again from the begin state (so all repetitions do the same work; the copy is outside the
events) and is timed with HIP events around the one launch, after warm-up: median, p10, p90 in microseconds, ns per step
per walk (over the steps walks really took: a stuck walk takes none), aggregate steps per second, and the accepted
share.  Histogram: ``best_rank`` over 4 096 walks after ``--hist-steps`` steps from each start.  Also records the
kernels' VGPRs, LDS and scratch from the code object.  Writes OUT_DIR/flips_bench.json.  With ``--plus-after`` the same
through tg_flip_advance_plus (include/tensor_game_flips_plus.h; K one above the start's length where the start fills K,
so that a plus has a slot), every row and histogram also with ``pluses`` and the stuck walks, written to
OUT_DIR/flips_bench_plus_N_M.json.  (There ``steps_taken`` is exact only while no walk gets stuck after its best step:
with plus_slack 0, or when stuck_walks is 0.)  With ``--mod2`` the same starts, W and steps per launch through
tg_flip2_advance (include/tensor_game_flips_mod2.h), written to OUT_DIR/flips_bench_mod2.json (or
flips_bench_mod2_plus_N_M.json): there every step taken is a flip or a plus, so ``steps_taken`` is exact (flips + pluses
+ one step per stuck walk, the one that found no match).  Every row also carries ``ns_per_accepted_flip``, the median
time over the flips (and pluses) made: the figure to compare the integer walks and the Z_2 walks by, since the integer
walks refuse many drawn flips cheaply and the Z_2 walks refuse none.
"""
from __future__ import annotations

import argparse
import json
import re
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mat_mul_amd import FlipWalks, Mod2Walks, build, ops  # noqa: E402

DEV = "cuda:0"
N_STEPS = 4096


def standard_matmul(n, shift=1, spare=0):
    """The n^3 terms a_ij (x) b_jk (x) c_ik of <n,n,n> as tokens (K = n^3 + spare rows)."""
    S = n * n
    rows = np.zeros((n ** 3 + spare, 3 * S), dtype=np.int64)
    t = 0
    for i in range(n):
        for j in range(n):
            for k in range(n):
                rows[t, i * n + j] = rows[t, S + j * n + k] = rows[t, 2 * S + i * n + k] = 1
                t += 1
    rows[:t] += shift
    return rows.astype(np.int8)


def stats(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median_us": statistics.median(ts), "p10_us": q(0.1), "p90_us": q(0.9), "reps": len(ts)}


def kernel_resources():
    """VGPRs, LDS and scratch of the flip kernels (integer and Z_2), from the metadata of the built objects."""
    out = {}
    for name in ("tg_flips.o", "tg_flips_mod2.o"):
        res = object_resources(build.OBJ_DIR / name)
        if "error" in res:
            return res
        out.update(res)
    return out


def object_resources(obj):
    llvm = Path("/opt/rocm/llvm/bin")
    out = {}
    if not obj.exists():  # a tree that received the library without its objects
        return {"error": f"{obj.name} is not here: run `python tools/flips_bench.py --resources` where the library was built"}
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = Path(tmp) / "fat", Path(tmp) / "co"
        try:
            subprocess.run([llvm / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, Path(tmp) / "discard.o"], check=True)
            subprocess.run([llvm / "clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
            notes = subprocess.run([llvm / "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        except (OSError, subprocess.CalledProcessError) as e:
            return {"error": str(e)}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                  for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                            "vgpr_spill_count", "sgpr_spill_count")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--resources", action="store_true", help="only (re)write the kernels' resources into OUT_DIR/flips_bench.json; no GPU")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hist-steps", type=int, default=100000)
    ap.add_argument("--walks", type=int, nargs="*", default=[256, 4096, 65536])
    ap.add_argument("--plus-after", type=int, default=None, help="walk with plus transitions (tg_flip_advance_plus)")
    ap.add_argument("--plus-slack", type=int, default=1)
    ap.add_argument("--mod2", action="store_true", help="walk over Z_2 (tg_flip2_advance)")
    args = ap.parse_args()
    plus = args.plus_after is not None
    stem = "flips_bench_mod2" if args.mod2 else "flips_bench"
    out = Path(args.out) / (f"{stem}_plus_{args.plus_after}_{args.plus_slack}.json" if plus else f"{stem}.json")
    if args.mod2:
        start = dict(shift=1, plus_after=args.plus_after or 0, plus_slack=args.plus_slack)
    else:
        start = dict(bound=1, shift=1, plus_after=args.plus_after, plus_slack=args.plus_slack)
    Walks = Mod2Walks if args.mod2 else FlipWalks
    out.parent.mkdir(parents=True, exist_ok=True)
    if args.resources:
        res = json.loads(out.read_text()) if out.exists() else {}
        res["resources"] = kernel_resources()
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["resources"], indent=1))
        return
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "n_steps": N_STEPS, "resources": kernel_resources(),
           "rows": [], "histograms": []}
    if plus:
        res.update(plus_after=args.plus_after, plus_slack=args.plus_slack)
    if args.mod2:
        res["mod2"] = True
    for n in (2, 3, 4):
        S, K = n * n, n ** 3 + (args.plus_slack if plus else 0)
        tokens = torch.from_numpy(standard_matmul(n, spare=K - n ** 3)[None]).to(DEV)
        lengths = torch.tensor([n ** 3], dtype=torch.int64, device=DEV)
        for W in args.walks:
            walks = Walks.start(tokens, lengths, walks_per_list=W, seed=1, **start)
            begin = {k: v.clone() for k, v in walks._st.items()}
            ts = []
            for rep in range(args.warmup + args.reps):
                for k, v in begin.items():
                    walks._st[k].copy_(v)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if args.mod2:
                    ops.flip2_advance(walks._st, N_STEPS, S, start["plus_after"], args.plus_slack, seed=1)
                elif plus:
                    ops.flip_advance_plus(walks._st, N_STEPS, args.plus_after, args.plus_slack, bound=1, shift=1, seed=1)
                else:
                    ops.flip_advance(walks._st, N_STEPS, bound=1, shift=1, seed=1)
                b.record()
                b.synchronize()
                if rep >= args.warmup:
                    ts.append(a.elapsed_time(b) * 1e3)
            st = stats(ts)
            # steps really taken: a list can only lose its last match in a step that lowers the rank, so a stuck walk took
            # best_step steps and one more that found no match
            stuck = walks.state == 1
            taken = int(torch.where(stuck, walks.best_step + 1, torch.full_like(walks.best_step, N_STEPS)).sum())
            made = int(walks.flips.sum()) + (int(walks.pluses.sum()) if plus or args.mod2 else 0)
            if args.mod2:  # exact: no step is refused
                taken = made + int(stuck.sum())
            row = {"n": n, "S": S, "K": K, "W": W, **st, "steps_taken": taken,
                   "ns_per_step_per_walk": st["median_us"] * 1e3 / max(taken, 1),
                   "steps_per_s": taken / (st["median_us"] * 1e-6), "accepted_share": float(walks.flips.sum()) / max(taken, 1),
                   "ns_per_accepted_flip": st["median_us"] * 1e3 / max(made, 1),
                   "stuck_walks": int(stuck.sum()), "min_best_rank": int(walks.best_rank.min())}
            if plus or args.mod2:
                row["pluses"] = int(walks.pluses.sum())
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        walks = Walks.start(tokens, lengths, walks_per_list=4096, seed=2, **start)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        walks.advance(args.hist_steps)
        b.record()
        b.synchronize()
        ranks, counts = torch.unique(walks.best_rank, return_counts=True)
        hist = {"n": n, "S": S, "K": K, "W": 4096, "steps": args.hist_steps, "seconds": a.elapsed_time(b) * 1e-3,
                "best_rank": {int(r): int(c) for r, c in zip(ranks.cpu(), counts.cpu())}, "stuck_walks": int((walks.state == 1).sum())}
        if plus or args.mod2:
            hist["pluses"] = int(walks.pluses.sum())
        res["histograms"].append(hist)
        print(json.dumps(hist), flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
