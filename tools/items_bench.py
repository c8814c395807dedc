"""tg_demo_items at the BASELINE shapes against what a caller has without it, and against the reference's per-item
arithmetic on the CPU.

    python tools/items_bench.py OUT_DIR [--reps 50] [--warmup 10]

One process, one GPU.  Per config (S=4 R=7 65 536 demos; S=16 R=49 8 192 demos; S=25 R=64 4 096 demos, plain and in a
random basis) and per N in {256, 4096}, T in {1, 2}, dtype in {int8, float32}: the microseconds per ops.demo_items call
(HIP events around each call after warm-up: median and spread over --reps calls), the byte / MAC model of the call,
which bound it sits nearer to, and the same items through the grouped path -- group the batch by action index, then
per group step_many over the suffix + gen_from_factors per history frame + index_copy into the batch (this tool only;
not part of the product).  Plus the reference's per-item arithmetic (datasets.py:84-122 without the file I/O, float32
torch, 16 threads) for N = 256.  Writes OUT_DIR/r05_items.json.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mat_mul_amd import SyntheticDemos, ops  # noqa: E402

DEV = "cuda:0"
HBM_BPS = 6.29e12        # measured HBM copy rate (MI355X_MICROARCH: float4 copy)
MFMA_I8_OPS = 5.0e15     # dense int8 matrix-core peak (spec, ~5 POPS; a MAC is 2 ops)
CONFIGS = [("cfg1_S4", 4, 7, 65536, False), ("cfg3_S16", 16, 49, 8192, False), ("cfg5_S25", 25, 64, 4096, False),
           ("cfg5_S25_random_basis", 25, 64, 4096, True)]


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
    return {"median_us": statistics.median(out), "min_us": out[0], "max_us": out[-1],
            "p10_us": out[len(out) // 10], "p90_us": out[(9 * len(out)) // 10], "n": len(out)}


def grouped(demos, idx, T, dtype):
    """The caller's path without demo_items: batch grouped by action index (one host sync for the groups)."""
    R, S = demos.max_actions, demos.dim_3d
    N = idx.shape[0]
    out = torch.empty((N, T, S, S, S), dtype=torch.int8, device=DEV)
    k_all, d_all = idx % R, idx // R
    for k in torch.unique(k_all).tolist():
        sel = (k_all == k).nonzero().flatten()
        d = d_all[sel]
        head = demos.target_tensor[d].contiguous()
        if k < R - 1:
            head, _ = ops.step_many(head, demos.action_seq[d, k + 1:].contiguous(), shift=demos.shift)
        frames = [head] + [ops.gen_from_factors(demos.action_seq[d, j:j + 1].contiguous(), S, shift=demos.shift)
                           for j in reversed(range(k + 1, min(k + T, R)))]
        frames += [torch.zeros_like(head)] * (T - len(frames))
        out.index_copy_(0, sel, torch.stack(frames, 1))
    return out if dtype == torch.int8 else out.to(dtype)


def cpu_reference(tok, tgt, idx, R, T, shift=1):
    """datasets.py:84-122 per item in float32 torch (files excluded): suffix replay, history frames, zero padding."""
    S = tgt.shape[-1]
    out = []
    for x in idx.tolist():
        d, k = divmod(x, R)
        f = (tok[d].float() - shift)
        u, v, w = f[:, :S], f[:, S:2 * S], f[:, 2 * S:]
        t = tgt[d].float()
        for j in range(k + 1, R):
            t = t - u[j][:, None, None] * v[j][None, :, None] * w[j][None, None, :]
        frames = [t] + [u[j][:, None, None] * v[j][None, :, None] * w[j][None, None, :]
                        for j in reversed(range(k + 1, min(k + T, R)))]
        frames += [torch.zeros_like(t)] * (T - len(frames))
        out.append((torch.stack(frames), torch.tensor([float(R - k)]), tok[d][k], torch.tensor([float(-(k + 1))])))
    return out


def model(S, R, idx, T, esize):
    k = (idx % R).double()
    K = (R - 1 - k)
    N = idx.shape[0]
    n3 = S ** 3
    b_target = N * n3
    b_tokens = float((K + 1).sum()) * 3 * S + N * 8
    b_frames = N * T * n3 * esize + N * (3 * S + 8)
    macs = float(K.sum()) * n3
    t_mem = (b_target + b_tokens + b_frames) / HBM_BPS * 1e6
    t_mfma = 2 * macs / MFMA_I8_OPS * 1e6
    return {"bytes_target_gather": b_target, "bytes_token_reads": b_tokens, "bytes_frame_writes": b_frames,
            "macs": macs, "ideal_us_hbm": t_mem, "ideal_us_mfma": t_mfma,
            "bound": "memory" if t_mem >= t_mfma else "compute"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--grouped-reps", type=int, default=5)
    args = ap.parse_args()
    torch.set_num_threads(16)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "configs": []}
    for name, S, R, n_demos, rb in CONFIGS:
        demos = SyntheticDemos.generate(n_demos, S, R, DEV, dim_t=2, seed=1, random_basis=rb)
        gen = torch.Generator(device=DEV).manual_seed(7)
        for N in (256, 4096):
            idx = torch.randint(0, len(demos), (N,), generator=gen, device=DEV)
            for T in (1, 2):
                for dtype in (torch.int8, torch.float32):
                    esize = 1 if dtype == torch.int8 else 4
                    out = torch.empty((N, T, S, S, S), dtype=dtype, device=DEV)
                    sc = torch.empty((N, 1), device=DEV)
                    ac = torch.empty((N, 3 * S), dtype=torch.int8, device=DEV)
                    rw = torch.empty((N, 1), device=DEV)

                    def call():
                        ops.demo_items(demos.action_seq, demos.target_tensor, idx, T, dtype=dtype, out=out,
                                       scalars=sc, actions=ac, rewards=rw, shift=demos.shift)

                    t_items = event_times(call, args.reps, args.warmup)
                    t_grouped = event_times(lambda: grouped(demos, idx, T, dtype), args.grouped_reps, 1)
                    assert torch.equal(out.to(torch.int8), grouped(demos, idx, T, torch.int8)), (name, N, T)
                    row = {"config": name, "S": S, "R": R, "n_demos": n_demos, "random_basis": rb, "N": N, "T": T,
                           "dtype": str(dtype).replace("torch.", ""), "demo_items": t_items, "grouped_path": t_grouped,
                           "speedup_vs_grouped": t_grouped["median_us"] / t_items["median_us"],
                           "model": model(S, R, idx.cpu(), T, esize)}
                    row["model"]["achieved_GBps"] = (row["model"]["bytes_target_gather"] + row["model"]["bytes_token_reads"]
                                                     + row["model"]["bytes_frame_writes"]) / t_items["median_us"] / 1e3
                    res["configs"].append(row)
                    print(json.dumps({k: row[k] for k in ("config", "N", "T", "dtype")} |
                                     {"items_us": round(t_items["median_us"], 1),
                                      "grouped_us": round(t_grouped["median_us"], 1),
                                      "bound": row["model"]["bound"]}), flush=True)
        # the reference's per-item arithmetic on the CPU, N = 256, T = 2
        idx = torch.randint(0, len(demos), (256,), generator=gen, device=DEV).cpu()
        tok, tgt = demos.action_seq.cpu(), demos.target_tensor.cpu()
        t0 = time.perf_counter()
        cpu_reference(tok, tgt, idx, R, 2, demos.shift)
        dt = (time.perf_counter() - t0) * 1e6
        res["configs"].append({"config": name, "cpu_reference_float32_16_threads": {"N": 256, "T": 2, "us": dt}})
        print(json.dumps({"config": name, "cpu_reference_us_N256_T2": round(dt)}), flush=True)
        del demos
        torch.cuda.empty_cache()
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "r05_items.json").write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
