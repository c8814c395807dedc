"""tg_symmetry_apply / tg_symmetry_sample against the gather they follow and against a copy of the same footprint.

    python tools/symmetry_bench.py OUT_DIR [--reps 30] [--warmup 10]

One process, one GPU.  Per S in {4, 16, 25} (R = 7 / 49 / 64 as the BASELINE configs, T = 2), N in {256, 1024, 4096} and
output dtype in {float32, bfloat16}, the microseconds (HIP events around each call after warm-up, sustained: median and
p10-p90 over --reps calls) of
  (a) gather       ops.demo_items straight to the output dtype: a batch without augmentation, today's path;
  (b) gather_i8    ops.demo_items to int8;
  (c) apply        ops.symmetry_apply alone, int8 -> the output dtype;
  (d) sample       ops.symmetry_sample alone;
  (e) augmented    (b) + (d) + (c) back to back, as ``batches(augment=...)`` runs them;
  copy             ops.copy_states (tg_copy_i8) reading and writing N*T*S^3*(1 + sizeof(OutT)) bytes in all: the apply
                   kernel's footprint as a plain copy;
and the apply kernel's share of the HBM rate on that footprint.  Writes OUT_DIR/r19_symmetry.json.

The ablations of the S >= 6 apply kernel (A/B library only): TG_LIB_VARIANT=ab with TG_SYM_NO_PERM=1 (the body reads the
staged bytes in input order: no tables, no walk) or TG_SYM_NO_STORE=1 (the body's 16-byte stores are not issued), and
--tag _noperm / _nostore to name the output.  Their outputs are wrong on purpose; only (c) and (e) mean anything.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mat_mul_amd import SyntheticDemos, ops  # noqa: E402

DEV = "cuda:0"
HBM_BPS = 6.29e12  # measured HBM copy rate (MI355X_MICROARCH: float4 copy)
CONFIGS = [(4, 7, 4096), (16, 49, 1024), (25, 64, 512)]  # S, R, n_demos
T = 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tag", default="", help="suffix of the output file (an A/B run: TG_LIB_VARIANT=ab and a TG_SYM_* switch)")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "T": T, "hbm_bps": HBM_BPS,
           "switches": {k: v for k, v in os.environ.items() if k.startswith(("TG_SYM_", "TG_LIB_VARIANT"))}, "rows": []}
    for S, R, n_demos in CONFIGS:
        demos = SyntheticDemos.generate(n_demos, S, R, DEV, dim_t=T, seed=1)
        gen = torch.Generator(device=DEV).manual_seed(7)
        for N in (256, 1024, 4096):
            idx = torch.randint(0, len(demos), (N,), generator=gen, device=DEV)
            for dtype in (torch.float32, torch.bfloat16):
                esize = torch.empty((), dtype=dtype).element_size()
                out = torch.empty((N, T, S, S, S), dtype=dtype, device=DEV)
                raw = torch.empty((N, T, S, S, S), dtype=torch.int8, device=DEV)
                sc, rw = torch.empty((N, 1), device=DEV), torch.empty((N, 1), device=DEV)
                ac = torch.empty((N, 3 * S), dtype=torch.int8, device=DEV)
                ac2 = torch.empty_like(ac)
                sym = torch.empty((N, 3 * S + 1), dtype=torch.uint8, device=DEV)
                games = N * T * (1 + esize) // 2  # read + write of these games = the apply kernel's footprint
                src = torch.randint(-3, 4, (games, S, S, S), device=DEV).to(torch.int8)
                dst = torch.empty_like(src)

                def gather(dt, o):
                    ops.demo_items(demos.action_seq, demos.target_tensor, idx, T, dtype=dt, out=o, scalars=sc,
                                   actions=ac, rewards=rw, shift=demos.shift)

                def sample():
                    ops.symmetry_sample(N, S, DEV, seed=3, item_offset=11, out=sym)

                def apply():
                    ops.symmetry_apply(raw, ac, sym, dtype=dtype, shift=demos.shift, out=out, actions=ac2)

                def augmented():
                    gather(torch.int8, raw)
                    sample()
                    apply()

                gather(torch.int8, raw)
                sample()
                times = {"gather": event_times(lambda: gather(dtype, out), args.reps, args.warmup),
                         "gather_i8": event_times(lambda: gather(torch.int8, raw), args.reps, args.warmup),
                         "apply": event_times(apply, args.reps, args.warmup),
                         "sample": event_times(sample, args.reps, args.warmup),
                         "augmented": event_times(augmented, args.reps, args.warmup),
                         "copy": event_times(lambda: ops.copy_states(src, out=dst), args.reps, args.warmup)}
                nbytes = N * T * S ** 3 * (1 + esize)
                row = {"S": S, "R": R, "N": N, "T": T, "dtype": str(dtype).replace("torch.", ""), "apply_bytes": nbytes,
                       "apply_hbm_share": nbytes / HBM_BPS * 1e6 / times["apply"]["median_us"],
                       "apply_over_copy": times["apply"]["median_us"] / times["copy"]["median_us"],
                       "augmented_over_gather": times["augmented"]["median_us"] / times["gather"]["median_us"], **times}
                res["rows"].append(row)
                print(json.dumps({k: row[k] for k in ("S", "N", "dtype")} |
                                 {k + "_us": round(v["median_us"], 1) for k, v in times.items()} |
                                 {"hbm_share": round(row["apply_hbm_share"], 3)}), flush=True)
        del demos
        torch.cuda.empty_cache()
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / f"r19_symmetry{args.tag}.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
