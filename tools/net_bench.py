"""The fused network (include/tensor_game_net.h) against the float32 restatement run eagerly, at the training app's
configuration (tests/net_ref.CONFIGS["a"]: S 4, T 2, c 8, W 32, 8 + 2 layers, n_steps 12), k = 8.

    python tools/net_bench.py OUT_DIR [--config a] [--reps 20] [--warmup 3] [--fused-only] [--masked] [--kernel-stats CSV]

One process, one GPU.  Per B in {256, 1024, 4096}: FusedAlphaTensor.fwd_infer and the eager Ref.fwd_infer (the
reference's op structure: the whole prefix rerun at every token step, torch's Categorical) alternate call by call;
HIP events around each call after warm-up; median, p10 and p90 in microseconds.  FLOPs are counted from shapes for the
fused algorithm (the decoder with its cache).  Then one self-play figure: microseconds per simulation of
search.actor_prediction with net.policy at S = 4, B = 4096.  --fused-only runs the fused calls alone (for a kernel-trace
run); --kernel-stats merges a rocprofv3 --stats CSV into an existing OUT_DIR/r08_net.json.  Writes OUT_DIR/r08_net.json.
--config picks another configuration of net_ref.CONFIGS, tests/net_s9_ref.CONFIGS (a9, b9: S = 9) or
tests/net_s16_ref.CONFIGS (a16, b16: S = 16); the file is then OUT_DIR/r08_net_<config>.json.  At S = 9 the self-play
figure is skipped; at S = 16 the sizes are B = 16, 256 and 1024 and the self-play figure is at B = 256, n_sim = 4.
--torso-only times tg_net_torso alone at B = 16 and 256 and writes OUT_DIR/r08_torso_<config>[_slices].json; with
TG_LIB_VARIANT=ab, TG_NET_TORSO_SLICES=1 forces net_torso_slice_kernel at any size (the A/B library's switch).
--masked times torso + sample through the row mask (tg_net_torso_masked, tg_net_sample_masked) with a share f = 1, 0.75,
0.5, 0.25 and 1/B of the rows active (seeded random flags) next to the plain call, the calls alternating in one process,
at B = 256 and 4096 (B = 16 and 256 at S = 16); it merges its result into OUT_DIR/r13_masked.json under net_<config>.
At S = 25 (tests/net_s25_ref.CONFIGS: a25, b25, c25; FusedAlphaTensor25, include/tensor_game_net_s25.h) the sizes are
B = 16 and 256, each with the torso alone, sample on its output at k = 1 and at k = n_samples, and fwd_infer next to the
eager restatement (which is timed max(2, reps / 8) times there: a call takes seconds); no self-play figure.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from mat_mul_amd import FusedAlphaTensor, FusedAlphaTensor25, search  # noqa: E402
from net_ref import CONFIGS, Ref, dims, make_inputs, make_weights  # noqa: E402
from net_s9_ref import CONFIGS as CONFIGS_S9  # noqa: E402
from net_s16_ref import CONFIGS as CONFIGS_S16  # noqa: E402
from net_s25_ref import CONFIGS as CONFIGS_S25  # noqa: E402

CONFIGS = {**CONFIGS, **CONFIGS_S9, **CONFIGS_S16, **CONFIGS_S25}

DEV = "cuda:0"
FP32_PEAK = 157.3e12  # MI355X vector FP32, FLOP/s (FMA = 2)


def flops(m, B, k):
    """Multiply-adds x 2 of the fused algorithm, from shapes."""
    S2, T2 = m["S"] ** 2, 2 * m["S"] ** 2
    c, hd, ff = m["c"], m["torso_heads"] * m["torso_d"], m["torso_ff"]
    L2 = 2 * m["S"]
    pair = T2 * c * hd * 3 + m["S"] * L2 * L2 * hd * 2 + T2 * hd * c + T2 * c * ff * 2
    torso = 3 * S2 * (m["S"] * m["T"] + 1) * c + m["torso_layers"] * 3 * pair
    W, H, d, J, n = m["W"], m["heads"], m["d"], 3 * S2, m["n_steps"]
    hd, ff = H * d, m["ff"]
    mlp = W * hd + W * ff * 2  # li1, li2, li3
    dec = 0
    for t in range(n):
        self_att = W * hd + hd * W + H * (t + 1) * W * 2 + W * hd + mlp
        cross = W * hd + hd * c + H * J * c * 2 + c * hd + mlp
        dec += m["blocks"] * (self_att + cross) + W * m["n_logits"]
    nh = m["n_hidden"]
    value = W * nh + 2 * nh * nh + nh * m["n_quantile"]
    return 2 * (B * torso + B * k * dec + B * value)


def stats(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median_us": statistics.median(ts), "p10_us": q(0.1), "p90_us": q(0.9), "n": len(ts)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--torso-only", action="store_true")
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--config", default="a", choices=sorted(CONFIGS))
    args = ap.parse_args()
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    path = out / ("r08_net.json" if args.config == "a" else f"r08_net_{args.config}.json")
    if args.kernel_stats:
        res = json.loads(path.read_text())
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "net_" in r.get("Name", "")]
        res["kernel_stats"] = rows
        path.write_text(json.dumps(res, indent=1))
        print(json.dumps(rows))
        return
    cfg = CONFIGS[args.config]
    m = dims(cfg)
    k = cfg["n_samples"]
    sd = make_weights(cfg, 11)
    wide25 = m["S"] == 25
    net = (FusedAlphaTensor25 if wide25 else FusedAlphaTensor).from_state_dict(sd, k, device=DEV)
    ref = Ref(sd, cfg, device=DEV, dtype=torch.float32)
    res = {"config": m, "k": k, "fp32_peak_flops": FP32_PEAK, "sizes": []}
    if args.torso_only:
        slices = os.environ.get("TG_LIB_VARIANT") == "ab" and "TG_NET_TORSO_SLICES" in os.environ
        res = {"config": m, "kernel": "net_torso_slice_kernel" if slices or m["S"] in (16, 25) else "net_torso_kernel",
               "sizes": []}
        for B in (16, 256):
            xx, ss = make_inputs(cfg, B, B)
            xx, ss = torch.from_numpy(xx).to(DEV).float(), torch.from_numpy(ss).to(DEV)
            for _ in range(args.warmup):
                net.torso(xx, ss)
            torch.cuda.synchronize()
            row = {"B": B, "torso": stats([timed(lambda: net.torso(xx, ss)) for _ in range(args.reps)])}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
        res["command"] = " ".join(sys.argv)
        path = out / f"r08_torso_{args.config}{'_slices' if slices else ''}.json"
        path.write_text(json.dumps(res, indent=1))
        print(f"wrote {path}")
        return
    wide16 = m["S"] == 16
    if args.masked:
        res = {"config": m, "k": k, "need": 129, "sizes": [], "command": " ".join(sys.argv)}
        for B in ((16, 256) if wide16 or wide25 else (256, 4096)):
            xx, ss = make_inputs(cfg, B, B)
            xx, ss = torch.from_numpy(xx).to(DEV).float(), torch.from_numpy(ss).to(DEV)
            rows = torch.arange(B, device=DEV, dtype=torch.int64)
            ee = torch.zeros((B, 3 * m["S"] ** 2, m["c"]), dtype=torch.float32, device=DEV)
            tokens = torch.zeros((B, k, m["n_steps"]), dtype=torch.int8, device=DEV)
            probs, q = torch.zeros((B, k), device=DEV), torch.zeros((B,), device=DEV)
            rng = np.random.default_rng(B)
            variants = {}
            for name, n_act in (("1", B), ("0.75", 3 * B // 4), ("0.5", B // 2), ("0.25", B // 4), ("1/B", 1)):
                fl = np.full(B, 128, np.uint8)  # PENDING alone: inactive under need = EXPAND | PENDING
                fl[rng.permutation(B)[:n_act]] = 129
                variants[name] = (n_act, torch.from_numpy(fl).to(DEV))

            def call(fl):
                net.torso(xx, ss, out=ee, flags=fl, need=129)
                net.sample(ee, rows, seed=1, tokens=tokens, probs=probs, q=q, flags=fl, need=129)

            calls = {"plain": lambda: call(None), **{f: (lambda fl=fl: call(fl)) for f, (_, fl) in variants.items()}}
            with torch.no_grad():
                for _ in range(args.warmup):
                    for fn in calls.values():
                        fn()
                torch.cuda.synchronize()
                ts = {name: [] for name in calls}
                for _ in range(args.reps):
                    for name, fn in calls.items():
                        ts[name].append(timed(fn))
            row = {"B": B, "plain": stats(ts["plain"]), "masked": {}}
            for f, (n_act, _) in variants.items():
                st = stats(ts[f])
                row["masked"][f] = {**st, "active_rows": n_act, "active_share": n_act / B,
                                    "time_over_plain": st["median_us"] / row["plain"]["median_us"]}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
        res["device"] = torch.cuda.get_device_name(0)
        path = out / "r13_masked.json"
        whole = json.loads(path.read_text()) if path.exists() else {}
        whole[f"net_{args.config}"] = res
        path.write_text(json.dumps(whole, indent=1) + "\n")
        print(f"wrote {path}")
        return
    eager_reps = max(2, args.reps // 8) if wide25 else args.reps
    for B in ((16, 256) if wide25 else (16, 256, 1024) if wide16 else (256, 1024, 4096)):
        xx, ss = make_inputs(cfg, B, B)
        xx = torch.from_numpy(xx).to(DEV).float()
        ss = torch.from_numpy(ss).to(DEV)
        fused = lambda: net.fwd_infer(xx, ss, seed=1)  # noqa: E731
        eager = lambda: ref.fwd_infer(xx, ss, k)  # noqa: E731
        with torch.no_grad():
            for i in range(args.warmup):
                fused()
                if not args.fused_only and i < eager_reps:
                    eager()
            torch.cuda.synchronize()
            tf, te = [], []
            for i in range(args.reps):
                tf.append(timed(fused))
                if not args.fused_only and i < eager_reps:
                    te.append(timed(eager))
        f = flops(m, B, k)
        row = {"B": B, "fused": stats(tf), "flops": f,
               "fused_share_of_fp32_peak": f / (statistics.median(tf) * 1e-6) / FP32_PEAK}
        if wide25:  # the two launches of fwd_infer apart, and the decoder with one sample per game
            ee = net.torso(xx, ss)
            parts = {"torso": lambda: net.torso(xx, ss), "sample_k1": lambda: net.sample(ee, seed=1, k=1),
                     f"sample_k{k}": lambda: net.sample(ee, seed=1)}
            for fn in parts.values():
                fn()
            torch.cuda.synchronize()
            ts = {name: [] for name in parts}
            for _ in range(args.reps):
                for name, fn in parts.items():
                    ts[name].append(timed(fn))
            row.update({name: stats(t) for name, t in ts.items()})
        if te:
            row["eager_restatement_fp32"] = stats(te)
            row["eager_over_fused"] = statistics.median(te) / statistics.median(tf)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    if not args.fused_only and (args.config == "a" or wide16):
        B, S, T = (256, 16, cfg["dim_t"]) if wide16 else (4096, 4, cfg["dim_t"])
        start = torch.from_numpy(np.random.default_rng(0).integers(-1, 2, size=(B, T, S, S, S)).astype(np.int8)).to(DEV)
        n_sim, max_actions = (4, 2) if wide16 else (16, 4)
        pol = net.policy(seed=3)
        first = [0]

        def counted(frames, scalars, games):
            first[0] += int(games.shape[0] == B)
            return pol(frames, scalars, games)

        search.actor_prediction(counted, start, 1, n_sim=2, n_bar=100, n_logits=3, k=k)  # warm-up
        first[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        search.actor_prediction(counted, start, max_actions, n_sim=n_sim, n_bar=100, n_logits=3, k=k)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        res["self_play"] = {"B": B, "S": S, "k": k, "n_sim": n_sim, "max_actions": max_actions,
                            "simulations": first[0], "us_per_simulation": wall * 1e6 / max(1, first[0]),
                            **({} if wide16 else {"search_only_us_per_simulation_r06": 122})}
        print(json.dumps(res["self_play"]), flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    res["command"] = " ".join(sys.argv)
    if not args.fused_only:
        path.write_text(json.dumps(res, indent=1))
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
