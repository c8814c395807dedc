"""tg_solution_canon (include/tensor_game_solutions.h) against a restatement of the same steps in torch ops on the same
GPU: verification, sign normalisation, lexicographic order, run merge, canonical tokens and the key.

    python tools/solutions_bench.py OUT_DIR [--reps 20] [--warmup 3] [--shapes 4096,4,8 4096,25,64]

One process, one GPU.  Per shape M,S,K: seeded lists with planted duplicates, negated duplicates, sign variants and null
terms (tests/solutions_ref.random_lists), targets exact / one entry off / random by thirds; ``ops.solution_canon`` and
the torch restatement are each timed with HIP events around the call after warm-up (median, p10, p90 in microseconds),
and their outputs are compared bit for bit before anything is timed; ``kernel_no_targets`` is the call without
verification (targets=None): the canonical form and the key alone.  The restatement covers good rows only (the
seeded lists have no bad row); it verifies in float64, which is exact below 2^53, and orders the terms by stable sorts
over 9-bit digits packed seven to an int64.  Writes OUT_DIR/solutions_bench.json.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from mat_mul_amd import ops  # noqa: E402
import solutions_ref as SR  # noqa: E402

DEV = "cuda:0"


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


def _i64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


C1, C2, GOLD, LEN = (_i64(c) for c in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53, 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F))


def fmix64(k):
    """MurmurHash3's finaliser on int64 tensors holding the 64 bits (the shifts made logical by a mask)."""
    m = (1 << 31) - 1
    k = k ^ ((k >> 33) & m)
    k = k * C1
    k = k ^ ((k >> 33) & m)
    k = k * C2
    return k ^ ((k >> 33) & m)


def torch_canon(targets, tokens, lengths, shift):
    """(canon, rank, key, residual_nnz) of good rows, in batched torch ops."""
    M, K, A3 = tokens.shape
    S = A3 // 3
    dev = tokens.device
    used = torch.arange(K, device=dev)[None, :] < lengths[:, None]                        # (M,K)
    f = (tokens.to(torch.int32) - shift) * used[:, :, None]
    # verification: exact in float64 (every partial sum is below 2^31)
    u, v, w = (f[:, :, x * S:(x + 1) * S].to(torch.float64) for x in range(3))
    uv = (u[:, :, :, None] * v[:, :, None, :]).reshape(M, K, S * S)
    total = torch.bmm(uv.transpose(1, 2), w).reshape(M, S, S, S)
    res = (targets.to(torch.float64) != total).sum(dim=(1, 2, 3)).to(torch.int32)
    # null terms, first non-zero positive
    g = f.reshape(M, K, 3, S)
    nz = g != 0
    live = nz.any(dim=3).all(dim=2) & used                                                # (M,K)
    first = torch.gather(g, 3, nz.to(torch.int32).argmax(dim=3, keepdim=True)).squeeze(3)  # (M,K,3)
    neg = first < 0
    g = torch.where(neg[:, :, :, None], -g, g)
    sigma = 1 - 2 * (neg.sum(dim=2) & 1)                                                  # (M,K)
    g = g.reshape(M, K, A3)
    # lexicographic order: least significant digits first, stable; the dead terms go last
    order = torch.arange(K, device=dev)[None, :].expand(M, K)
    digits = (g + 192).to(torch.int64)                                                    # 0 .. 384: nine bits
    for hi in range(A3, 0, -7):
        lo = max(0, hi - 7)
        packed = torch.zeros((M, K), dtype=torch.int64, device=dev)
        for e in range(lo, hi):
            packed = (packed << 9) | digits[:, :, e]
        order = torch.gather(order, 1, torch.sort(torch.gather(packed, 1, order), dim=1, stable=True).indices)
    order = torch.gather(order, 1, torch.sort((~torch.gather(live, 1, order)).to(torch.uint8), dim=1, stable=True).indices)
    g = torch.gather(g, 1, order[:, :, None].expand(M, K, A3))
    sigma = torch.gather(sigma, 1, order) * torch.gather(live, 1, order)
    # runs of equal terms: c = sum of sigma, |c| copies kept, w negated where c < 0
    start = torch.ones((M, K), dtype=torch.bool, device=dev)
    start[:, 1:] = (g[:, 1:] != g[:, :-1]).any(dim=2)
    run = torch.cumsum(start, 1) - 1                                                      # (M,K) run index
    c = torch.zeros((M, K), dtype=torch.int64, device=dev).scatter_add_(1, run, sigma.to(torch.int64))
    c = torch.gather(c, 1, run)
    pos = torch.arange(K, device=dev)[None, :]
    in_run = pos - torch.cummax(torch.where(start, pos, 0), 1).values
    kept = in_run < c.abs()
    rank = kept.sum(dim=1).to(torch.int32)
    g[:, :, 2 * S:] = torch.where((c < 0)[:, :, None], -g[:, :, 2 * S:], g[:, :, 2 * S:])
    at = torch.where(kept, torch.cumsum(kept, 1) - 1, K)                                  # row K: the sink
    canon = torch.zeros((M, K + 1, A3), dtype=torch.int8, device=dev)
    canon.scatter_(1, at[:, :, None].expand(M, K, A3), (g + shift).to(torch.int8))
    canon = canon[:, :K].contiguous()
    # the key over the rank * 3S canonical bytes
    n = rank.to(torch.int64) * A3
    pad = -(K * A3) % 8
    words = torch.nn.functional.pad(canon.reshape(M, K * A3), (0, pad)).view(torch.int64)  # (M,W), little endian
    k = torch.arange(words.shape[1], device=dev, dtype=torch.int64)[None, :]
    part = fmix64(words + (k + 1) * GOLD) * (8 * k < n[:, None])
    key = fmix64(part.sum(dim=1) ^ (n * LEN))
    return canon, rank, key, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["4096,4,8", "4096,25,64"], help="M,S,K")
    args = ap.parse_args()
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "rows": []}
    for shape in args.shapes:
        M, S, K = (int(x) for x in shape.split(","))
        rng = np.random.default_rng(M + 1000 * S + K)
        base = min(M, 256)                                          # distinct lists; the batch tiles them
        tokens, lengths = SR.random_lists(rng, base, K, S, 1)
        targets = SR.targets_for(rng, tokens, lengths, S, 1)
        reps = -(-M // base)
        tok, lens, tgt = (torch.from_numpy(np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:M].copy()).to(DEV)
                          for x in (tokens, lengths, targets))
        got, want = ops.solution_canon(tgt, tok, lens, shift=1), torch_canon(tgt, tok, lens, 1)
        for name, a, b in zip(("canon", "rank", "key", "residual_nnz"), got, want):
            assert torch.equal(a, b), f"{shape}: the restatement's {name} differs from the kernel's"
        row = {"M": M, "S": S, "K": K, "mean_rank": float(got[1].float().mean())}
        row["kernel"] = timed(lambda: ops.solution_canon(tgt, tok, lens, shift=1), args.reps, args.warmup)
        row["kernel_no_targets"] = timed(lambda: ops.solution_canon(None, tok, lens, shift=1), args.reps, args.warmup)
        row["torch_ops"] = timed(lambda: torch_canon(tgt, tok, lens, 1), args.reps, args.warmup)
        row["speedup"] = row["torch_ops"]["median_us"] / row["kernel"]["median_us"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    out = Path(args.out) / "solutions_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
