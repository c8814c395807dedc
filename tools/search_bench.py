#!/usr/bin/env python3
"""Per-simulation cost of the batched search (tg_search_select + tg_search_commit), HIP events around the two launches
of every simulation, with the device stand-in ``search.keyed_policy`` between them (not timed: a zero-cost network).

    python tools/search_bench.py [--out profiles/r06_search.json]                       (GPU)
    python tools/search_bench.py --reference DIR [--out profiles/r06_search.json]       (CPU: adds the reference)

Shapes: S=4 B=4096 T=2 n_sim=16; S=16 B=256 T=2 n_sim=16; S=25 B=64 T=1 n_sim=16 (k=8, max_actions=6).  Reported per
shape: us per simulation for all B games (median, p10, p90 over the simulations of a whole self-play run) and the
bytes one simulation moves per game by construction (index probes, node rows, frames, children) -- the kernels are
latency-bound (dependent probes per descent level), so no bandwidth figure is claimed.  ``--reference DIR`` times the
reference's extend_tree (act.py:115-216) on the CPU, one game, with the host form of the same stand-in, and records its
simulations per second next to the device's.

    python tools/search_bench.py --masked [--out profiles/r13_masked.json]              (GPU)

times whole ``search.actor_prediction`` runs with the fused network (FusedAlphaTensor of tests/net_ref's configurations
a and a16, rank-2 start states), ``net.policy(seed)`` against ``net.policy(seed, masked=True)`` alternating, at S = 4,
B = 4096, k = 8, n_sim = 16, max_actions = 8 and at S = 16, B = 256, n_sim = 4, max_actions = 2.  Besides the wall time
it reports the active share: over the policy calls of the masked run, the rows whose flags hold the needed bits divided
by B x calls (read from ``forest.flags`` here only; that read is inside the timed run, the same for every repetition).
The result is merged into the file under ``self_play``.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
SHAPES = [(4, 4096, 2), (16, 256, 2), (25, 64, 1)]
K, N_SIM, MAX_ACTIONS = 8, 16, 6


def shape_name(S, B, T):
    return f"S{S}_B{B}_T{T}"


def start_and_pool(S, B, T):
    rng = np.random.default_rng(S)
    st = np.zeros((B, T, S, S, S), np.int8)
    st[:, 0] = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(B, S, S, S))
    pool = rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2], size=(24, 3 * S)).astype(np.int8)
    return st, pool


def bytes_per_sim(S, T, k, depth, index_capacity):
    """Bytes one game's simulation reads + writes, by construction of the kernels (64 index slots per probe round)."""
    FB = (S ** 3 + 15) // 16 * 16
    probe = 64 * 8 + 4
    level = probe + 4 + k * 4 + 8 + 8        # nchild, Q row, chosen key, path entry
    select = (depth + 1) * probe + depth * level + 2 * T * FB + 3 * S + 32
    commit = k * (3 * S + FB) + k * probe + 2 * T * FB + k * (3 * S + 16) + depth * 16 + 32
    return select + commit


def bench_device():
    import torch

    from mat_mul_amd import search

    dev = "cuda:0"
    out = {}
    for S, B, T in SHAPES:
        st, pool = start_and_pool(S, B, T)
        forest = search.SearchForest(B, S, T, k=K, max_actions=MAX_ACTIONS, n_sim=N_SIM, device=dev)
        pol = search.keyed_policy(forest, torch.from_numpy(pool), seed=1)
        games = torch.arange(B, device=dev)
        times, depths = [], []
        for rep in range(2):  # the first run warms up (code objects, allocator); the second is measured
            forest.reset(torch.from_numpy(st).to(dev), N_SIM)
            times.clear()
            depths.clear()
            for _ in range(MAX_ACTIONS):
                for _ in range(N_SIM):
                    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    e0.record()
                    frames, scalars = forest.select()
                    e1.record()
                    tok, _, q = pol(frames, scalars, games)
                    e2.record()
                    forest.commit(tok, q)
                    e3 = torch.cuda.Event(enable_timing=True)
                    e3.record()
                    retry = forest.flags & search.RETRY
                    while bool(retry.any()):
                        sel = retry.nonzero()[:, 0]
                        t2, _, q2 = pol(frames[sel], scalars[sel], sel)
                        tok[sel], q[sel] = t2, q2
                        forest.commit(tok, q, mask=(retry != 0).to(torch.uint8))
                        retry = forest.flags & search.RETRY
                    torch.cuda.synchronize()
                    times.append((e0.elapsed_time(e1) + e2.elapsed_time(e3)) * 1e3)
                    depths.append(float(forest.depth.float().mean()))
                forest.advance(N_SIM)
                if bool(forest.done.all()):
                    break
        t = np.array(times)
        d = float(np.mean(depths))
        out[shape_name(S, B, T)] = dict(
            S=S, B=B, T=T, k=K, n_sim=N_SIM, max_actions=MAX_ACTIONS, simulations=len(t),
            us_per_sim_median=round(float(np.median(t)), 2), us_per_sim_p10=round(float(np.percentile(t, 10)), 2),
            us_per_sim_p90=round(float(np.percentile(t, 90)), 2),
            games_per_second=round(B / (float(np.median(t)) * 1e-6)), mean_depth=round(d, 2),
            bytes_per_game_sim=round(bytes_per_sim(S, T, K, d, forest.index_capacity)),
            status_nonzero=int((forest.status != 0).sum()))
        print(shape_name(S, B, T), out[shape_name(S, B, T)], flush=True)
    return dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shapes=out)


MASKED_RUNS = [("a", 4096, 16, 8), ("a16", 256, 4, 2)]  # configuration, B, n_sim, max_actions


def bench_masked(reps=3):
    import torch

    from mat_mul_amd import FusedAlphaTensor, SyntheticDemos, search
    from net_ref import CONFIGS, make_weights
    from net_s16_ref import CONFIGS as CONFIGS_S16

    dev = "cuda:0"
    out = {}
    for name, B, n_sim, max_actions in MASKED_RUNS:
        cfg = {**CONFIGS, **CONFIGS_S16}[name]
        S, T, k = cfg["dim_3d"], cfg["dim_t"], cfg["n_samples"]
        sd = make_weights(cfg, 11)
        start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=dev)
        start[:, 0] = SyntheticDemos(2, B, 1, S, device=dev, seed=3).target_tensor.reshape(B, S, S, S)
        count = {}

        def run(masked):
            net = FusedAlphaTensor.from_state_dict(sd, k, device=dev)
            forest = search.SearchForest(B, S, T, k=k, max_actions=max_actions, n_sim=n_sim, device=dev)
            inner = net.policy(seed=3, masked=masked)
            count.update(calls=0, rows=0, first=0)

            def plain(frames, scalars, games):
                count["calls"] += 1
                count["first"] += int(games.shape[0] == B)
                return inner(frames, scalars, games)

            def flagged(frames, scalars, games, flags, need, out):
                count["calls"] += 1
                count["first"] += int(need != search.RETRY)
                count["rows"] += int(((flags & need) == need).sum())
                return inner(frames, scalars, games, flags=flags, need=need, out=out)

            flagged.takes_flags = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = search.actor_prediction(flagged if masked else plain, start, max_actions, n_sim=n_sim, n_bar=100,
                                          n_logits=3, k=k, forest=forest)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, [t.cpu() for t in res], dict(count)

        run(False), run(True)  # warm-up
        wall = {False: [], True: []}
        for _ in range(reps):
            for masked in (False, True):
                dt, res, c = run(masked)
                wall[masked].append(dt)
                if masked:
                    counted, got = c, res
                else:
                    sims, want = c["first"], res
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "the two policies played different games"
        med = {m: float(np.median(v)) for m, v in wall.items()}
        out[f"{name}_B{B}"] = dict(
            config=name, S=S, B=B, T=T, k=k, n_sim=n_sim, max_actions=max_actions, reps=reps, simulations=sims,
            policy_calls=counted["calls"], active_share=round(counted["rows"] / (B * counted["calls"]), 4),
            mean_length=round(float(want[3].float().mean()), 3),
            plain_seconds=[round(x, 4) for x in wall[False]], masked_seconds=[round(x, 4) for x in wall[True]],
            plain_us_per_simulation=round(med[False] * 1e6 / sims, 1),
            masked_us_per_simulation=round(med[True] * 1e6 / sims, 1),
            masked_over_plain=round(med[True] / med[False], 4))
        print(name, out[f"{name}_B{B}"], flush=True)
    return dict(device=torch.cuda.get_device_name(0), command=" ".join(sys.argv), runs=out)


def bench_reference(ref_dir):
    """The reference's extend_tree on the CPU, one game per shape, with the host form of the stand-in."""
    import torch

    sys.path.insert(0, str(ref_dir))
    import act  # noqa: E402  (reference)
    import search_ref as R

    out = {}
    for S, B, T in SHAPES:
        st, pool = start_and_pool(S, 1, T)
        fn = R.keyed_policy(pool, K, seed=1)

        class StandIn:
            device = "cpu"

            def __init__(self):
                self.attempts = {}

            def fwd_infer(self, state, scalars):
                head = state[0, 0].numpy().astype(np.int8)
                key = R.head_key(head)
                a = self.attempts.get(key, 0)
                self.attempts[key] = a + 1
                tok, q = fn(head, None, 0, a, key)
                return torch.from_numpy(tok.astype(np.int64))[None], None, torch.tensor([q])

        model = StandIn()
        state = torch.from_numpy(st[0].astype(np.float32))[None]
        tree, info = {}, {}
        n = 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 5.0 and n < N_SIM * MAX_ACTIONS:
            tree, info = act.extend_tree(model, state, 0, MAX_ACTIONS, tree, info)
            n += 1
        dt = time.perf_counter() - t0
        out[shape_name(S, B, T)] = dict(simulations=n, seconds=round(dt, 3), sims_per_second=round(n / dt, 1))
        print("reference", shape_name(S, B, T), out[shape_name(S, B, T)], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/r06_search.json (profiles/r13_masked.json with --masked)")
    ap.add_argument("--masked", action="store_true", help="self-play with the fused network, plain against masked policy")
    ap.add_argument("--reference", default=None, help="directory of the reference (CPU run; adds its rate)")
    args = ap.parse_args()
    path = Path(args.out or ROOT / "profiles" / ("r13_masked.json" if args.masked else "r06_search.json"))
    res = json.loads(path.read_text()) if path.exists() else {}
    if args.masked:
        res["self_play"] = bench_masked()
    elif args.reference:
        res["reference_extend_tree_cpu"] = bench_reference(args.reference)
        for name, r in res["reference_extend_tree_cpu"].items():
            dev = res.get("device_search", {}).get("shapes", {}).get(name)
            if dev:
                r["device_game_sims_per_second"] = dev["games_per_second"]
    else:
        res["device_search"] = bench_device()
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
