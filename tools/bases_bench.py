"""tg_solution_rebase and tg_basis_inverse_i32 (include/tensor_game_bases.h) against the same map in torch ops on the
same GPU.

    python tools/bases_bench.py OUT_DIR [--reps 20] [--warmup 3] [--shapes 4096,16,16 4096,25,64]

One process, one GPU.  Per shape M,S,K: 64 sampled bases (``BasisSet.sample``), seeded lists with factor values from
{-2..2} (tests/bases_ref.random_lists) and a random basis per row; ``ops.solution_rebase`` with the inverses and a torch
restatement (a float64 einsum, exact below 2^53, and a mask for the rows behind a list's end) are compared bit for bit and then each
timed with HIP events around the call after warm-up (median, p10, p90 in microseconds); ``inverse`` is
``ops.basis_inverse`` of M sampled factor pairs.  The restatement covers good rows only (the seeded lists have no bad
row).  Writes OUT_DIR/bases_bench.json.
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

from mat_mul_amd import BasisSet, ops  # noqa: E402
import bases_ref as BR  # noqa: E402
from solutions_bench import DEV, timed  # noqa: E402


def torch_rebase(tokens, lengths, mats, index, shift):
    M, K, A3 = tokens.shape
    S = A3 // 3
    f = (tokens.to(torch.float64) - shift).view(M, K, 3, S)   # float64 is exact here: every sum is below 2^44
    out = torch.einsum("mxab,mkxb->mkxa", mats[index].to(torch.float64), f).reshape(M, K, A3) + shift
    used = torch.arange(K, device=tokens.device)[None, :, None] < lengths[:, None, None]
    return (out * used).to(torch.int8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["4096,16,16", "4096,25,64"], help="M,S,K")
    args = ap.parse_args()
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "rows": []}
    for shape in args.shapes:
        M, S, K = (int(x) for x in shape.split(","))
        rng = np.random.default_rng(M + 1000 * S + K)
        base = min(M, 256)                                          # distinct lists; the batch tiles them
        tokens, lengths = BR.random_lists(rng, base, K, S, 1)
        reps = -(-M // base)
        tok, lens = (torch.from_numpy(np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:M].copy()).to(DEV)
                     for x in (tokens, lengths))
        bases = BasisSet.sample(64, S, DEV, seed=3)
        index = torch.from_numpy(rng.integers(0, 64, size=M)).to(DEV)
        got, glen, bad = ops.solution_rebase(tok, lens, bases.inverse, index=index)
        assert not bool(bad.any()) and torch.equal(glen, lens)
        assert torch.equal(got, torch_rebase(tok, lens, bases.inverse, index, 1)), f"{shape}: the restatement differs"
        _, L, U = ops.sample_basis(M, S, DEV, seed=5, want_factors=True)
        row = {"M": M, "S": S, "K": K, "mean_length": float(lens.float().mean())}
        row["kernel"] = timed(lambda: ops.solution_rebase(tok, lens, bases.inverse, index=index), args.reps, args.warmup)
        row["torch_ops"] = timed(lambda: torch_rebase(tok, lens, bases.inverse, index, 1), args.reps, args.warmup)
        row["speedup"] = row["torch_ops"]["median_us"] / row["kernel"]["median_us"]
        row["inverse"] = timed(lambda: ops.basis_inverse(L, U), args.reps, args.warmup)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    out = Path(args.out) / "bases_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
