"""BilinearMatmul (mat_mul_amd/bilinear.py, include/tensor_game_bilinear.h) next to torch.matmul, and the two kernels
next to a copy.

    python tools/bilinear_bench.py OUT_DIR [--sizes 2048 4096 8192] [--reps 7] [--warmup 2]

One process, one GPU, float32 square matrices.  Algorithms: Strassen's list (tests/golden/strassen.npz) at levels 1, 2
and 3, and the standard list of <2,2,2> (8 products: the same arithmetic as the schoolbook method, so what it loses
against torch.matmul is the cost of the encodes, the decode and the smaller leaf products alone).  A size is skipped
when its temporaries would not fit in the free memory.

Rows "matmul": ``alg(A, B, out=C)`` and ``torch.matmul(A, B, out=D)``, alternating, each repetition between two device
events after warm-up of both; median, p10 and p90 in microseconds, the ratio of the medians, and the largest deviation of
the two results over the largest entry (the inputs are standard normal).

Rows "encode" and "decode": the first level of the same call alone, its bytes (every input byte read once, every output
byte written once: (N^2 + R (N/2)^2) * 4) over its time, alternating with a device copy of the same byte count (``copy_``
between two contiguous float32 tensors of half that many bytes each, which moves 16 bytes per lane), and the ratio of the
two rates.  Writes OUT_DIR/bilinear_bench.json.

    python tools/bilinear_bench.py OUT_DIR --rect [--sizes ...] [--reps 7] [--warmup 2]

The rectangular entries (include/tensor_game_rect.h) instead, with the same method; writes OUT_DIR/bilinear_rect_bench.json.
Rows "square": the standard list of <n,n,n>, n = 2..5, at N rounded down to a multiple of 4n (so that every call takes
16-byte packs), through the square entries and through the rectangular ones on the grid n x n, alternating in one loop,
five times over: five medians of each, the spread (lowest to highest median) of the square entry, and whether the median
of the rectangular entry's medians lies inside it.  Rows "footprint": the grids 4 x 5 and 5 x 6 (blocks of N/gr x N/gc,
the width rounded down to a multiple of 4; R = 2 gr gc terms with a third of the coefficients +-1), encode and decode,
next to ``copy_`` of the same byte count.  Every row gives its bytes (each read or written once) and the share of the
8 TB/s HBM peak they reach.

    python tools/bilinear_bench.py OUT_DIR --fused [--sizes ...] [--reps 7] [--warmup 2]

``FusedBilinearMatmul`` (include/tensor_game_products.h) on bfloat16 square matrices, with the same method; writes
OUT_DIR/bilinear_fused_bench.json.  Lists: Strassen's (7 products), the standard <2,2,2> (8), the 49-term Kronecker square
of Strassen's at n = 4, the standard <4,4,4> (64) and the standard <3,3,3> (27, at N rounded down to a multiple of 24 so
that its blocks take 16-byte loads too).  Per size one loop alternates every list's ``alg(A, B, out=C)``, every list's
products kernel alone (``ops.bilinear_products``) and ``torch.matmul`` on the same operands.  Rows "fused": the three
times, the products' share of the call, the ratio to torch.matmul and the deviation from it over the largest entry.
Rows "ratio": time(7) / time(8) and time(49) / time(64), of the whole call and of the products alone, next to 7/8 and
49/64: what encode-on-load lets the saved products show.
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

from mat_mul_amd import BilinearMatmul, FusedBilinearMatmul, ops, standard_rect  # noqa: E402

DEV = "cuda:0"
HBM_PEAK_TB_PER_S = 8.0


def standard_2x2(shift=1):
    rows = np.zeros((8, 12), dtype=np.int64)
    t = 0
    for i in range(2):
        for j in range(2):
            for k in range(2):
                rows[t, i * 2 + j] = rows[t, 4 + j * 2 + k] = rows[t, 8 + i * 2 + k] = 1
                t += 1
    return (rows + shift).astype(np.int8)


def stats(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median_us": statistics.median(ts), "p10_us": q(0.1), "p90_us": q(0.9), "reps": len(ts)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(fns, warmup, reps):
    """Each of ``fns`` warmed up, then timed in turn ``reps`` times; a list of stats, one per function."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(timed(fn))
    return [stats(t) for t in ts]


def temporaries_bytes(N, rank, levels):
    """float32 bytes ``alg(A, B)`` allocates at size N: both operands' encodes and every level's products."""
    total, side, count = 0, N, 1
    for _ in range(levels):
        side, count = side // 2, count * rank
        total += 3 * count * side * side * 4
    return total


def rate(nbytes, st):
    tb = nbytes / st["median_us"] * 1e-6
    return {"TB_per_s": tb, "share_of_hbm_peak": tb / HBM_PEAK_TB_PER_S}


def rect_rows(args):
    """The --rect rows (the module's text says what they are)."""
    out = Path(args.out) / "bilinear_rect_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "dtype": "float32",
           "hbm_peak_TB_per_s": HBM_PEAK_TB_PER_S, "rows": []}
    gen = torch.Generator(device=DEV).manual_seed(0)

    def emit(row):
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")

    for n in (2, 3, 4, 5):
        tok, R = standard_rect(n, n, n).to(DEV), n ** 3
        for N in args.sizes:
            N = N // (4 * n) * (4 * n)
            nbytes = (N * N + R * (N // n) ** 2) * 4
            if 3 * nbytes > torch.cuda.mem_get_info(0)[0]:
                emit({"kind": "square", "n": n, "N": N, "skipped": "memory"})
                continue
            X = torch.randn((1, N, N), device=DEV, generator=gen)
            Y = torch.empty((1, R, N // n, N // n), device=DEV)
            C = torch.empty_like(X)
            fns = [lambda: ops.bilinear_encode(X, tok, R, n, 0, out=Y), lambda: ops.bilinear_rect_encode(X, tok, R, n, n, 0, out=Y),
                   lambda: ops.bilinear_decode(Y, tok, R, n, out=C), lambda: ops.bilinear_rect_decode(Y, tok, R, n, n, out=C)]
            rounds = [alternate(fns, args.warmup, args.reps) for _ in range(5)]
            for half, (sq, re) in (("encode", (0, 1)), ("decode", (2, 3))):
                sq_med = [r[sq]["median_us"] for r in rounds]
                re_med = [r[re]["median_us"] for r in rounds]
                mid = statistics.median(re_med)
                emit({"kind": "square", "half": half, "n": n, "N": N, "R": R, "bytes": nbytes, "square_medians_us": sq_med,
                      "rect_medians_us": re_med, "square_spread_us": [min(sq_med), max(sq_med)], "rect_median_us": mid,
                      "rect_inside_square_spread": min(sq_med) <= mid <= max(sq_med),
                      "rect_over_square": mid / statistics.median(sq_med),
                      "square": rate(nbytes, {"median_us": statistics.median(sq_med)}), "rect": rate(nbytes, {"median_us": mid})})
            del X, Y, C
            torch.cuda.empty_cache()
    for gr, gc in ((4, 5), (5, 6)):
        S, R = gr * gc, 2 * gr * gc
        f = torch.randint(0, 6, (R, 3 * S), generator=torch.Generator().manual_seed(gr))
        tok = (torch.where(f == 0, 1, 0) - torch.where(f == 1, 1, 0) + 1).to(torch.int8).to(DEV)   # a third +-1
        for N in args.sizes:
            h, w = N // gr, N // gc // 4 * 4
            nbytes = (gr * h * gc * w + R * h * w) * 4
            if 3 * nbytes > torch.cuda.mem_get_info(0)[0]:
                emit({"kind": "footprint", "grid": [gr, gc], "N": N, "skipped": "memory"})
                continue
            X = torch.randn((1, gr * h, gc * w), device=DEV, generator=gen)
            Y = torch.empty((1, R, h, w), device=DEV)
            C = torch.empty_like(X)
            src, dst = (torch.empty(nbytes // 8, dtype=torch.float32, device=DEV) for _ in range(2))
            src.normal_(generator=gen)
            ops.bilinear_rect_encode(X, tok, R, gr, gc, 0, out=Y)
            enc, cp1, dec, cp2 = alternate([lambda: ops.bilinear_rect_encode(X, tok, R, gr, gc, 0, out=Y), lambda: dst.copy_(src),
                                            lambda: ops.bilinear_rect_decode(Y, tok, R, gr, gc, out=C), lambda: dst.copy_(src)],
                                           args.warmup, args.reps)
            for half, mine, copy in (("encode", enc, cp1), ("decode", dec, cp2)):
                emit({"kind": "footprint", "half": half, "grid": [gr, gc], "rows": gr * h, "cols": gc * w, "R": R,
                      "bytes": nbytes, **mine, **rate(nbytes, mine), "copy": copy, "copy_TB_per_s": rate(nbytes, copy)["TB_per_s"],
                      "share_of_copy": copy["median_us"] / mine["median_us"]})
            del X, Y, C, src, dst
            torch.cuda.empty_cache()


def kron_square(f, n):
    """The Kronecker square of the coefficients f (R,3n^2) of an algorithm for <n,n,n>: one for <n^2,n^2,n^2>, term
    r1*R + r2 with u[(i1*n+i2)*n^2 + (j1*n+j2)] = u1[i1*n+j1] * u2[i2*n+j2], likewise v and w."""
    S, N = n * n, n * n
    out = np.zeros((len(f) ** 2, 3 * N * N), dtype=np.int64)
    for r1 in range(len(f)):
        for r2 in range(len(f)):
            for d in range(3):
                x1, x2 = (g[d * S:(d + 1) * S].reshape(n, n) for g in (f[r1], f[r2]))
                out[r1 * len(f) + r2, d * N * N:(d + 1) * N * N] = np.einsum("ij,kl->ikjl", x1, x2).reshape(N * N)
    return out


def fused_rows(args):
    """The --fused rows (the module's text says what they are)."""
    out = Path(args.out) / "bilinear_fused_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "rows": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    strassen = np.load(ROOT / "tests" / "golden" / "strassen.npz")["tokens"].astype(np.int64)[:7] - 1
    lists = [("strassen", torch.from_numpy((strassen + 1).astype(np.int8)), 2), ("standard2", standard_rect(2, 2, 2), 2),
             ("kron49", torch.from_numpy((kron_square(strassen, 2) + 1).astype(np.int8)), 4), ("standard4", standard_rect(4, 4, 4), 4),
             ("standard3", standard_rect(3, 3, 3), 3)]
    algs = [(name, FusedBilinearMatmul(tok.to(DEV), tok.shape[0], n), n) for name, tok, n in lists]

    def emit(row):
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")

    for N in args.sizes:
        A = torch.randn((N, N), device=DEV, generator=gen).bfloat16()
        B = torch.randn((N, N), device=DEV, generator=gen).bfloat16()
        C, D = torch.empty((N, N), device=DEV), torch.empty_like(A)
        fns, side = [], {}
        for name, alg, n in algs:
            side[name] = M = N if n != 3 else N // 24 * 24
            a, b, c = A[:M, :M], B[:M, :M], C[:M, :M]
            prod = torch.empty((1, alg.rank, M // n, M // n), device=DEV)
            fns.append(lambda alg=alg, a=a, b=b, c=c: alg(a, b, out=c))
            fns.append(lambda alg=alg, a=a, b=b, n=n, prod=prod: ops.bilinear_products(a[None], b[None], alg.tokens, alg.rank, n, n, n,
                                                                                       alg.shift, out=prod))
        fns.append(lambda: torch.matmul(A, B, out=D))
        times = alternate(fns, args.warmup, args.reps)
        theirs = times[-1]
        whole, alone = {}, {}
        for i, (name, alg, n) in enumerate(algs):
            whole[name], alone[name] = times[2 * i], times[2 * i + 1]
            M = side[name]
            alg(A[:M, :M], B[:M, :M], out=C[:M, :M])
            ref = torch.matmul(A[:M, :M].float(), B[:M, :M].float())
            emit({"kind": "fused", "list": name, "n": n, "N": M, "products": alg.products, "schoolbook_products": n ** 3,
                  "fused": whole[name], "products_alone": alone[name], "torch_matmul_bf16_at_N": N, "torch_matmul": theirs,
                  "products_share_of_call": alone[name]["median_us"] / whole[name]["median_us"],
                  "ratio_to_torch_matmul": whole[name]["median_us"] / theirs["median_us"],
                  "TFLOP_per_s_of_the_product": 2.0 * M ** 3 / whole[name]["median_us"] * 1e-6,
                  "max_deviation_from_float32_matmul": float((C[:M, :M] - ref).abs().max() / ref.abs().max())})
            del ref
        for few, many, ideal in (("strassen", "standard2", 7 / 8), ("kron49", "standard4", 49 / 64)):
            spread = lambda t: [t[few]["p10_us"] / t[many]["p90_us"], t[few]["p90_us"] / t[many]["p10_us"]]  # noqa: E731
            emit({"kind": "ratio", "of": [few, many], "N": N, "ideal": ideal,
                  "fused": whole[few]["median_us"] / whole[many]["median_us"], "fused_p10_p90": spread(whole),
                  "products_alone": alone[few]["median_us"] / alone[many]["median_us"], "products_alone_p10_p90": spread(alone)})
        del A, B, C, D, fns
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 4096, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rect", action="store_true", help="the rectangular entries instead (bilinear_rect_bench.json)")
    ap.add_argument("--fused", action="store_true", help="FusedBilinearMatmul in bfloat16 instead (bilinear_fused_bench.json)")
    args = ap.parse_args()
    if args.rect:
        return rect_rows(args)
    if args.fused:
        return fused_rows(args)
    out = Path(args.out) / "bilinear_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    strassen = np.load(ROOT / "tests" / "golden" / "strassen.npz")["tokens"].astype(np.int8)
    lists = [("strassen", strassen, 7, (1, 2, 3)), ("standard2", standard_2x2(), 8, (1,))]
    res = {"torch": torch.__version__, "device": torch.cuda.get_device_name(0), "dtype": "float32", "rows": []}
    gen = torch.Generator(device=DEV).manual_seed(0)
    for N in args.sizes:
        A = torch.randn((N, N), device=DEV, generator=gen)
        B = torch.randn((N, N), device=DEV, generator=gen)
        C, D = torch.empty_like(A), torch.empty_like(A)
        for name, tokens, rank, all_levels in lists:
            tok = torch.from_numpy(tokens).to(DEV)
            for levels in all_levels:
                free = torch.cuda.mem_get_info(0)[0]
                if N % 2 ** levels or 2 * temporaries_bytes(N, rank, levels) > free:
                    print(json.dumps({"kind": "matmul", "list": name, "levels": levels, "N": N, "skipped": "memory or size"}))
                    continue
                alg = BilinearMatmul(tok, rank, n=2, shift=1, levels=levels)
                ours, theirs = alternate([lambda: alg(A, B, out=C), lambda: torch.matmul(A, B, out=D)], args.warmup, args.reps)
                row = {"kind": "matmul", "list": name, "levels": levels, "N": N, "products": alg.products,
                       "bilinear": ours, "torch_matmul": theirs, "ratio": ours["median_us"] / theirs["median_us"],
                       "max_deviation": float((C - D).abs().max() / D.abs().max())}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
            # the kernels alone: the first level of this list at this size
            nbytes = (N * N + rank * (N // 2) ** 2) * 4
            src, dst = (torch.empty(nbytes // 8, dtype=torch.float32, device=DEV) for _ in range(2))
            src.normal_(generator=gen)
            Y = torch.empty((1, rank, N // 2, N // 2), device=DEV)
            ops.bilinear_encode(A[None], tok, rank, 2, 0, out=Y)
            enc, cp1, dec, cp2 = alternate([lambda: ops.bilinear_encode(A[None], tok, rank, 2, 0, out=Y), lambda: dst.copy_(src),
                                            lambda: ops.bilinear_decode(Y, tok, rank, 2, out=C[None]), lambda: dst.copy_(src)],
                                           args.warmup, args.reps)
            for kind, mine, copy in (("encode", enc, cp1), ("decode", dec, cp2)):
                row = {"kind": kind, "list": name, "N": N, "R": rank, "bytes": nbytes, **mine,
                       "TB_per_s": nbytes / mine["median_us"] * 1e-6, "copy": copy,
                       "copy_TB_per_s": nbytes / copy["median_us"] * 1e-6, "share_of_copy": copy["median_us"] / mine["median_us"]}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del src, dst, Y
            torch.cuda.empty_cache()
        out.write_text(json.dumps(res, indent=1) + "\n")
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
