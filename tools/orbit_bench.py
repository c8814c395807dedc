"""tg_orbit_canon (include/tensor_game_orbits.h) against the composition it replaces, on the same GPU: per group element
a torch gather of g.X, ``ops.solution_canon``, and a running lexicographic minimum in torch.

    python tools/orbit_bench.py OUT_DIR [--reps 10] [--warmup 2] [--comp-reps 3]
    python tools/orbit_bench.py OUT_DIR --resources      (no GPU: where the library was built, its objects are at hand)

One process, one GPU.  Shapes: S=4, K=8 with the 1 536 symmetries of <2,2,2> and their 384-element transversal, M = 16 and
4 096; S=9, K=27 with the 1 296 unsigned symmetries of <3,3,3>, M = 16 and 1 024.  Lists: seeded random lists
(tests/solutions_ref.random_lists) with the matmul tensor as target.  Each side is timed with HIP events around the whole
call after warm-up (median, p10, p90 in microseconds); the outputs of the two sides are compared bit for bit before
anything is timed.  ``kernel`` is the call as ``SolutionArchive`` makes it (workspace allocated by the wrapper: the group
is spread over workgroups when M is small), ``kernel_one_launch`` the call without workspace.  Also records the kernels'
VGPRs, LDS and scratch from the code object.  Writes OUT_DIR/orbit_bench.json.
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
sys.path.insert(0, str(ROOT / "tests"))

from mat_mul_amd import SymmetryGroup, build, ops  # noqa: E402
from mat_mul_amd.orbits import _flat  # noqa: E402
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


def composition(targets, tokens, lengths, p, s, shift):
    """The orbit form from existing pieces: per element a gather, tg_solution_canon and a lexicographic minimum."""
    M, K, A3 = tokens.shape
    vals = tokens.to(torch.int16) - shift
    best = rank = key = which = stab = None
    for g in range(p.shape[0]):
        moved = (vals[:, :, p[g]] * s[g] + shift).to(torch.int8)
        c, r, k, _ = ops.solution_canon(None, moved, lengths, shift=shift)
        order = (c.view(torch.uint8) ^ 0x80).reshape(M, K * A3)                  # unsigned order = the tokens' signed order
        if best is None:
            best, rank, key = order, r, k
            which = torch.zeros(M, dtype=torch.int32, device=tokens.device)
            stab = torch.ones(M, dtype=torch.int32, device=tokens.device)
            continue
        diff = order != best
        at = diff.to(torch.uint8).argmax(dim=1, keepdim=True)
        differs = diff.any(dim=1)
        less = differs & (order.gather(1, at) < best.gather(1, at)).squeeze(1)
        stab = torch.where(less, 1, stab + (~differs).to(torch.int32))
        which = torch.where(less, g, which)
        best = torch.where(less[:, None], order, best)
        rank, key = torch.where(less, r, rank), torch.where(less, k, key)
    canon = (best ^ 0x80).view(torch.int8).reshape(M, K, A3)
    res = ops.solution_canon(targets, tokens, lengths, shift=shift)[3]
    return canon, rank, key, res, which, stab


def kernel_resources():
    """VGPRs, LDS and scratch of the orbit kernels, from the metadata of the built object."""
    obj = build.OBJ_DIR / "tg_orbits.o"
    llvm = Path("/opt/rocm/llvm/bin")
    out = {}
    if not obj.exists():  # a tree that received the library without its objects
        return {"error": f"{obj.name} is not here: run `python tools/orbit_bench.py --resources` where the library was built"}
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
                                            "vgpr_spill_count")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--resources", action="store_true", help="only (re)write the kernels' resources into OUT_DIR/orbit_bench.json; no GPU")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--comp-reps", type=int, default=3)
    args = ap.parse_args()
    out = Path(args.out) / "orbit_bench.json"
    if args.resources:
        res = json.loads(out.read_text()) if out.exists() else {}
        res["resources"] = kernel_resources()
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["resources"], indent=1))
        return
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "resources": kernel_resources(), "rows": []}
    full2 = SymmetryGroup.matmul(2, DEV)
    cases = [(4, 8, "matmul(2)", full2, (16, 4096)), (4, 8, "matmul(2).modulo_term_signs()", full2.modulo_term_signs(), (16, 4096)),
             (9, 27, "matmul(3, signs=False)", SymmetryGroup.matmul(3, DEV, signs=False), (16, 1024))]
    for S, K, name, grp, Ms in cases:
        n = round(S ** 0.5)
        T = np.zeros((S, S, S), dtype=np.int8)
        for i in range(n):
            for j in range(n):
                for k in range(n):
                    T[i * n + j, j * n + k, i * n + k] = 1
        p, s = (torch.from_numpy(x).to(DEV) for x in _flat(grp.rows, S))
        s = s.to(torch.int16)
        for M in Ms:
            rng = np.random.default_rng(M + 1000 * S + K)
            base = min(M, 256)                                          # distinct lists; the batch tiles them
            tokens, lengths = SR.random_lists(rng, base, K, S, 1)
            reps = -(-M // base)
            tok, lens = (torch.from_numpy(np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:M].copy()).to(DEV)
                         for x in (tokens, lengths))
            tgt = torch.from_numpy(np.broadcast_to(T, (M, S, S, S)).copy()).to(DEV)
            got = ops.orbit_canon(tgt, tok, lens, grp.sym)
            one = ops.orbit_canon(tgt, tok, lens, grp.sym, workspace=False)
            want = composition(tgt, tok, lens, p, s, 1)
            for label, a, b, c in zip(("canon", "rank", "key", "residual_nnz", "which", "stab"), got, want, one):
                assert torch.equal(a, b), f"{name} M={M}: the composition's {label} differs from the kernel's"
                assert torch.equal(a, c), f"{name} M={M}: {label} depends on the workspace"
            row = {"S": S, "K": K, "group": name, "G": grp.order, "M": M, "mean_rank": float(got[1].float().mean()),
                   "workspace_bytes": ops.orbit_workspace_size(M, K, S, grp.order)}
            row["kernel"] = timed(lambda: ops.orbit_canon(tgt, tok, lens, grp.sym), args.reps, args.warmup)
            row["kernel_one_launch"] = timed(lambda: ops.orbit_canon(tgt, tok, lens, grp.sym, workspace=False), args.reps,
                                             args.warmup)
            row["composition"] = timed(lambda: composition(tgt, tok, lens, p, s, 1), args.comp_reps, 1)
            row["speedup"] = row["composition"]["median_us"] / row["kernel"]["median_us"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
