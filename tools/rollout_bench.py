"""Sampled policy rollouts (include/tensor_game_rollout.h, mat_mul_amd/rollout.py) on one MI355X.

    python tools/rollout_bench.py OUT_DIR [--parts a,b,c] [--configs a,a9,a16] [--reps 20] [--warmup 3]
    python tools/rollout_bench.py OUT_DIR --masked [--configs a,a16] [--fractions 1,0.5,0.1,0] [--repeats 5]
    python tools/rollout_bench.py OUT_DIR --stream [--configs a,a16] [--parent DIR] [--reps 7]

Writes (and, part by part, merges into) OUT_DIR/r12_rollout.json.  HIP events around each call after warm-up; median,
p10 and p90 in microseconds; two variants of one figure alternate call by call in one process.

 (a) tg_rollout_advance alone against the composition that existed before it for the same work
     (functional.take_action + the scalar increment + the running minimum and hit count in torch), at S = 4 / 9 / 16,
     T = 2, n = 8, 2 048 and 65 536 rows, random frames in {-2..2} and random tokens.  Bytes are counted from shapes
     (T frames read and written per row, the tokens) for the advance.
 (b) a full rollout with the fused network at configurations a, a9, a16 (tests/net_ref.py and its S = 9 / 16 files),
     G = 256 start states x n = 8 samples, max_actions = 7 / 12 / 8: sample_rollouts eager and graph=True (capture
     excluded: the replay of a captured loop is timed), the same loop from the pieces that existed before (net.torso,
     net.sample, functional.take_action, statistics in torch), and -- at configuration a only -- the loop on the eager
     float32 restatement of the network (tests/net_ref.Ref).  From 30 s per rollout on the number of runs drops below
     20 (the "n" of each figure says how many).
 (c) the feature in use, a report and not a test: FusedTrainer at configuration a on SyntheticDemos of 2 actions at
     S = 4, a solution search on 256 held-out targets (n = 8, max_actions = 4) every 50 training steps for 400 steps;
     num_solved, num_hits and lowest_rank per search.

--masked writes OUT_DIR/r14_rollout_masked.json instead: ONE step of the solution search (policy + advance) at
G = 256 x n = 8 rows with a share f of the groups still active (solved_step < 0 for them, every f-th group; the rows'
mask to match), for each f: the plain step (rollout_policy + tg_rollout_advance, which does not look at the records:
the same work at every f) next to the masked step (rollout_policy(masked=True) + tg_rollout_advance_masked), alternating
call by call in one process.  The records are put back before every call (both variants pay the same four small
copies), so every call sees the same share.  The whole measurement is made --repeats times; the spread of the plain
step's medians over the repeats is reported beside the figures.

--stream writes OUT_DIR/r15_rollout_stream.json instead: the solution search over a dataset of start states with
continuous refill (``solve_stream(slots=R)``, include/tensor_game_rollout_slots.h) against the chunked search
(``solve_states(chunk_groups=R)``), wall time per dataset, alternating run by run in one process.  With --parent DIR the
chunked side is the package of ANOTHER checkout (the parent commit, built there), loaded beside this one under its own
name with its own library; without it, this tree's solve_states (same Python, same code objects of the masked step).
N = 4 096 start states at configuration a, 512 at a16, n = 8, R = 256 and 1 024, the fused policy with the bias towards
the null action of the tests' ``fused_setup``, and three shares of start states that are solved at once (zero states):
0, 1/3 and 2/3; the others hold random entries and are practically never solved, so they take all max_actions steps.
Then ``rollout_refill`` (every slot takes a new state / every slot is kept) and ``rollout_advance_slots`` alone at
2 048 and 65 536 rows (S = 4, T = 2, n = 8) next to the masked advance, HIP events, the slot words put back before
every call on both sides.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from mat_mul_amd import FusedAlphaTensor, FusedTrainer, SyntheticDemos, functional, ops, rollout  # noqa: E402
from net_ref import CONFIGS, P, Ref, make_weights  # noqa: E402
from net_s9_ref import CONFIGS as CONFIGS_S9  # noqa: E402
from net_s16_ref import CONFIGS as CONFIGS_S16  # noqa: E402

CONFIGS = {**CONFIGS, **CONFIGS_S9, **CONFIGS_S16}
HORIZON = {"a": 7, "a9": 12, "a16": 8}
DEV = "cuda:0"


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


def alternate(fns, reps, warmup, budget_s=30.0):
    """{name: stats}: the variants alternate call by call; fewer than ``reps`` runs once a variant takes ``budget_s``."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    spent = {k: 0.0 for k in fns}
    for r in range(reps):
        for k, fn in fns.items():
            if r >= 5 and spent[k] > budget_s:
                continue
            t = timed(fn)
            ts[k].append(t)
            spent[k] += t * 1e-6
    return {k: stats(v) for k, v in ts.items()}


def part_a(reps, warmup):
    rows_out = []
    T, n = 2, 8
    for S in (4, 9, 16):
        for B in (2048, 65536):
            G = B // n
            rng = np.random.default_rng(S + B)
            frames = torch.from_numpy(rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)).to(DEV)
            tokens = torch.from_numpy(rng.integers(0, 3, size=(B, 3 * S)).astype(np.int8)).to(DEV)
            scal = torch.zeros((B, 1), device=DEV)
            rec = ops.rollout_records(G, S, DEV)
            nnz = torch.empty((B,), dtype=torch.int32, device=DEV)
            ovf = torch.zeros((B,), dtype=torch.uint8, device=DEV)
            actions = torch.zeros((B, 1, 3 * S), dtype=torch.int8, device=DEV)
            state = {"frames": frames.clone()}
            scal2 = torch.zeros((B, 1), device=DEV)
            best = torch.full((G,), S ** 3, dtype=torch.int32, device=DEV)
            hits = torch.zeros((G,), dtype=torch.int32, device=DEV)

            def advance():
                ops.rollout_advance(frames, tokens, n, 0, rec, scalars=scal, nnz=nnz, overflow=ovf, actions=actions)

            def composition():
                new, rank_ubs, m = functional.take_action(state["frames"], tokens, n, shift=1)
                state["frames"] = new
                scal2.add_(1)
                torch.minimum(best, m.values, out=best)
                hits.add_((m.values == 0).to(torch.int32))

            res = alternate({"advance": advance, "composition": composition}, reps, warmup)
            moved = B * (2 * T * S ** 3 + 2 * 3 * S + 4 + 4 + 4) + G * 16
            row = {"S": S, "T": T, "n": n, "rows": B, **res, "advance_bytes": moved,
                   "advance_bytes_per_s": moved / (res["advance"]["median_us"] * 1e-6),
                   "composition_over_advance": res["composition"]["median_us"] / res["advance"]["median_us"]}
            rows_out.append(row)
            print(json.dumps(row), flush=True)
            del frames, state
            torch.cuda.empty_cache()
    return rows_out


def unfused_loop(net_torso, net_sample, states, scalars, n, K, seed):
    """The rollout from the pieces that existed before tg_rollout_advance."""
    frames, scal = states.repeat_interleave(n, 0).contiguous(), scalars.repeat_interleave(n, 0).contiguous()
    B, G = frames.shape[0], states.shape[0]
    rows = torch.arange(B, device=DEV)
    best = torch.full((G,), states.shape[2] ** 3, dtype=torch.int32, device=DEV)
    hits = torch.zeros((G,), dtype=torch.int32, device=DEV)
    for step in range(K):
        tok = net_sample(net_torso(frames, scal), rows, seed, step).view(B, -1)
        frames, _, m = functional.take_action(frames, tok, n, shift=1)
        scal = scal + 1
        best = torch.minimum(best, m.values)
        hits += (m.values == 0).to(torch.int32)
    return best.min(), hits.sum()


def part_b(configs, reps, warmup):
    out = []
    G, n = 256, 8
    for name in configs:
        cfg = CONFIGS[name]
        S, T, K = cfg["dim_3d"], cfg["dim_t"], HORIZON[name]
        sd = make_weights(cfg, 11)
        net = FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)
        rng = np.random.default_rng(S)
        st = np.zeros((G, T, S, S, S), np.int8)
        st[:, 0] = rng.integers(-1, 2, size=(G, S, S, S))
        states, scalars = torch.from_numpy(st).to(DEV), torch.zeros((G, cfg["dim_s"]), device=DEV)
        pol = net.rollout_policy(seed=5)
        captured = rollout.sample_rollouts(pol, states, scalars, n, K, graph=True)
        torch.cuda.synchronize()
        # a replay continues from the captured buffers' current contents: the same launches on other data
        fns = {
            "eager": lambda: rollout.sample_rollouts(pol, states, scalars, n, K),
            "graph_replay": captured.graph.replay,
            "unfused_loop": lambda: unfused_loop(net.torso, lambda ee, rows, seed, step: net.sample(
                ee, rows, seed, call=step, k=1)[0], states, scalars, n, K, 5),
        }
        if name == "a":
            ref = Ref(sd, cfg, device=DEV, dtype=torch.float32)

            def ref_policy(frames, scal, rows, step):
                with torch.no_grad():
                    aa = ref.fwd_infer(frames.float(), scal, 1)[0]
                return aa.reshape(frames.shape[0], -1).to(torch.int8)

            fns["eager_float32_restatement"] = lambda: rollout.sample_rollouts(ref_policy, states, scalars, n, K)
        res = alternate(fns, reps, min(warmup, 1 if name == "a16" else warmup))
        eager = rollout.sample_rollouts(pol, states, scalars, n, K)
        row = {"config": name, "S": S, "T": T, "G": G, "n": n, "max_actions": K, **res,
               "lowest_rank": int(eager.lowest_rank.item()), "num_solved": int(eager.num_solved.item()),
               "unfused_over_eager": res["unfused_loop"]["median_us"] / res["eager"]["median_us"],
               "eager_over_graph": res["eager"]["median_us"] / res["graph_replay"]["median_us"]}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def part_c():
    cfg = CONFIGS["a"]
    S, T, R, n, K = cfg["dim_3d"], cfg["dim_t"], 2, 8, 4
    n_train, n_held = 8192, 256
    demos = SyntheticDemos(R, n_train + n_held, T, S, device=DEV, seed=21)
    tr = FusedTrainer.from_state_dict(make_weights(cfg, 11), dropout_p=0.1, n_samples=cfg["n_samples"], seed=3, device=DEV)
    opt = torch.optim.AdamW([tr.params], lr=1e-3)
    train_idx = torch.arange(n_train * R, device=DEV)
    held = torch.arange(n_train, n_train + n_held, device=DEV) * R + (R - 1)  # the whole target: R actions to go
    h_state, h_scalar, _, _ = demos.items(held, dtype=torch.int8)
    gen = torch.Generator(device=DEV).manual_seed(0)
    net = tr.net()
    searches, step, t0 = [], 0, time.perf_counter()

    def search():
        res = rollout.sample_rollouts(net.rollout_policy(seed=step), h_state, h_scalar, n, K)
        groups, tokens, lengths = res.solutions()
        ok = 0
        for g, tok, L in zip(groups.tolist(), tokens, lengths.tolist()):  # every returned solution replays to zero
            ok += int(not bool(functional.take_actions(tok[:L], h_state[g, 0], shift=1).any()))
        searches.append({"train_step": step, "num_solved": int(res.num_solved.item()), "of": n_held,
                         "num_hits": int(res.num_hits.item()), "lowest_rank": int(res.lowest_rank.item()),
                         "solutions_replayed_to_zero": ok, "l_pol": None, "l_val": None})
        print(json.dumps(searches[-1]), flush=True)

    search()
    while step < 400:
        for batch in demos.batches(256, generator=gen, indices=train_idx, dtype=torch.int8):
            l_pol, l_val = tr.train_step(batch, opt)
            step += 1
            if step % 50 == 0:
                search()
                searches[-1]["l_pol"], searches[-1]["l_val"] = float(l_pol.item()), float(l_val.item())
            if step >= 400:
                break
    torch.cuda.synchronize()
    return {"config": "a", "S": S, "demo_actions": R, "train_demos": n_train, "held_out": n_held, "n": n,
            "max_actions": K, "batch": 256, "lr": 1e-3, "dropout_p": 0.1, "searches": searches,
            "wall_s": time.perf_counter() - t0}


def part_masked(configs, fractions, reps, warmup, repeats):
    out = []
    G, n = 256, 8
    B = G * n
    for name in configs:
        cfg = CONFIGS[name]
        S, T = cfg["dim_3d"], cfg["dim_t"]
        net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 11), cfg["n_samples"], device=DEV)
        rng = np.random.default_rng(S)
        frames = torch.from_numpy(rng.integers(-1, 2, size=(B, T, S, S, S)).astype(np.int8)).to(DEV)
        scal = torch.zeros((B, cfg["dim_s"]), device=DEV)
        rows = torch.arange(B, device=DEV)
        plain_pol, masked_pol = net.rollout_policy(seed=5), net.rollout_policy(seed=5, masked=True)
        tokens = torch.ones((B, 3 * S), dtype=torch.int8, device=DEV)
        nnz = torch.zeros((B,), dtype=torch.int32, device=DEV)
        rec = ops.rollout_records(G, S, DEV)
        active = torch.ones((B,), dtype=torch.uint8, device=DEV)
        for f in fractions:
            k = int(round(f * G))
            on = torch.zeros((G,), dtype=torch.bool, device=DEV)
            if k:
                on[torch.linspace(0, G - 1, k, device=DEV).round().long()] = True
            fresh = list(ops.rollout_records(G, S, DEV))
            fresh[2] = torch.where(on, -1, 0).to(torch.int32)
            fresh[3] = fresh[2].clone()
            mask = on.repeat_interleave(n).to(torch.uint8)

            def restore():
                for r, x in zip(rec, fresh):
                    r.copy_(x)
                active.copy_(mask)

            def plain():
                restore()
                tok = plain_pol(frames, scal, rows, 0)
                ops.rollout_advance(frames, tok, n, 0, rec, scalars=scal, nnz=nnz)

            def masked():
                restore()
                masked_pol(frames, scal, rows, 0, active=active, out=tokens)
                ops.rollout_advance(frames, tokens, n, 0, rec, scalars=scal, nnz=nnz, active=active, stop_solved=True)

            runs = [alternate({"plain": plain, "masked": masked}, reps, warmup) for _ in range(repeats)]
            med = {v: [r[v]["median_us"] for r in runs] for v in ("plain", "masked")}
            row = {"config": name, "S": S, "T": T, "G": G, "n": n, "active_fraction": k / G,
                   "plain_median_us": statistics.median(med["plain"]), "masked_median_us": statistics.median(med["masked"]),
                   "plain_medians_us": med["plain"], "masked_medians_us": med["masked"],
                   "plain_spread_us": max(med["plain"]) - min(med["plain"]),
                   "masked_over_plain": statistics.median(med["masked"]) / statistics.median(med["plain"]),
                   "calls_per_median": runs[0]["plain"]["n"], "repeats": repeats}
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def load_parent(path):
    """The package of another checkout under the name mat_mul_amd_parent (its own _lib loads its own library)."""
    import importlib.util
    pkg = Path(path).resolve() / "mat_mul_amd"
    spec = importlib.util.spec_from_file_location("mat_mul_amd_parent", pkg / "__init__.py",
                                                  submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mat_mul_amd_parent"] = mod
    spec.loader.exec_module(mod)
    assert Path(mod._lib.LIB_PATH).resolve().parent.parent == pkg, mod._lib.LIB_PATH
    return mod


def null_biased(cfg, seed=77):
    """The weights of the tests' fused_setup: the last policy layer scaled down, its bias favouring the token of 0."""
    sd = make_weights(cfg, seed)
    sd[P + "li1.weight"] = sd[P + "li1.weight"] * 0.25
    assert cfg["n_logits"] == 3
    sd[P + "li1.bias"] = np.array([0.0, 3.0, 0.0], np.float32)
    return sd


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def part_stream(configs, parent, reps, warmup):
    out = []
    n = 8
    for name in configs:
        cfg = CONFIGS[name]
        S, T, K = cfg["dim_3d"], cfg["dim_t"], HORIZON[name]
        N = {"a": 4096, "a16": 512}.get(name, 512)
        sd = null_biased(cfg)
        net = FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)
        chunk_pkg = parent if parent is not None else sys.modules["mat_mul_amd"]
        net_c = chunk_pkg.FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV) if parent is not None else net
        rng = np.random.default_rng(S)
        base = np.zeros((N, T, S, S, S), np.int8)
        base[:, 0] = rng.integers(-1, 2, size=(N, S, S, S))
        scalars = torch.zeros((N, cfg["dim_s"]), device=DEV)
        for share, zero in (("0", np.zeros(N, bool)), ("1/3", np.arange(N) % 3 == 0), ("2/3", np.arange(N) % 3 != 2)):
            st = base.copy()
            st[zero] = 0
            states = torch.from_numpy(st).to(DEV)
            for R in (256, 1024):
                res = {}

                def stream():
                    res["stream"] = rollout.solve_stream(net.slot_policy(5), states, scalars, n, K, slots=R, check_every=4)

                def chunked():
                    res["chunked"] = chunk_pkg.rollout.solve_states(net_c.rollout_policy(5, masked=True), states, scalars,
                                                                    n, K, chunk_groups=R, check_every=1)

                fns = {"solve_states_chunked": chunked, "solve_stream": stream}
                for _ in range(warmup):
                    for fn in fns.values():
                        fn()
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, fn in fns.items():
                        ts[k].append(wall(fn))
                a, b = res["stream"], res["chunked"]
                equal = all(torch.equal(getattr(a, f), getattr(b, f)) for f in
                            ("best_nnz", "hits", "solved_step", "solved_sample", "groups", "tokens", "lengths"))
                row = {"config": name, "S": S, "N": N, "n": n, "R": R, "max_actions": K, "zero_share": share,
                       "solved": int((a.solved_step >= 0).sum().item()), "stream_ticks": a.ticks,
                       "chunked_steps": int(sum(b.steps_run)), "results_equal": equal,
                       "chunked_is_parent_checkout": parent is not None, **{k: stats(v) for k, v in ts.items()}}
                row["stream_over_chunked"] = row["solve_stream"]["median_us"] / row["solve_states_chunked"]["median_us"]
                out.append(row)
                print(json.dumps(row), flush=True)
    return out


def part_slot_entries(reps, warmup):
    out = []
    S, T, n, K, dim_s = 4, 2, 8, 7, 1
    for B in (2048, 65536):
        R = B // n
        rng = np.random.default_rng(B)
        N = 4 * R
        q_states = torch.from_numpy(rng.integers(-2, 3, size=(N, T, S, S, S)).astype(np.int8)).to(DEV)
        q_scal = torch.zeros((N, dim_s), device=DEV)
        sl = ops.rollout_slots(R, n, S, T, dim_s, K, DEV)
        outs = (*ops.rollout_records(N, S, DEV), torch.zeros((N,), dtype=torch.uint8, device=DEV),
                torch.zeros((N, K, 3 * S), dtype=torch.int8, device=DEV))
        ops.rollout_refill(sl, q_states, q_scal, outs, seed=1)
        tokens = torch.from_numpy(rng.integers(0, 3, size=(B, 3 * S)).astype(np.int8)).to(DEV)
        frames0 = sl.frames.clone()
        step0, stepK = torch.zeros_like(sl.slot_step), torch.full_like(sl.slot_step, K)
        head0 = torch.zeros_like(sl.head)
        rec = ops.rollout_records(R, S, DEV)
        fresh = ops.rollout_records(R, S, DEV)
        nnz = torch.zeros((B,), dtype=torch.int32, device=DEV)
        active = torch.ones((B,), dtype=torch.uint8, device=DEV)

        def put_back(step):
            sl.slot_step.copy_(step)
            sl.records[2].copy_(fresh[2])
            rec[2].copy_(fresh[2])
            sl.head.copy_(head0)

        def advance_slots():
            put_back(step0)
            ops.rollout_advance_slots(sl, tokens)

        def advance_masked():
            put_back(step0)
            ops.rollout_advance(frames0, tokens, n, 0, rec, scalars=sl.scalars, nnz=nnz, overflow=sl.overflow,
                                actions=sl.actions, active=active, stop_solved=True)

        def refill_all_take():
            put_back(stepK)
            ops.rollout_refill(sl, q_states, q_scal, outs, seed=1)

        def refill_all_kept():
            put_back(step0)
            ops.rollout_refill(sl, q_states, q_scal, outs, seed=1)

        def put_back_alone():
            put_back(step0)

        res = alternate({"advance_slots": advance_slots, "advance_masked": advance_masked,
                         "refill_all_take": refill_all_take, "refill_all_kept": refill_all_kept,
                         "put_back_alone": put_back_alone}, reps, warmup)
        row = {"S": S, "T": T, "n": n, "rows": B, "slots": R, "max_actions": K, **res}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--configs", default="a,a9,a16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--masked", action="store_true", help="time the step that stops solved groups (see above)")
    ap.add_argument("--fractions", default="1,0.5,0.1,0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stream", action="store_true", help="time solve_stream against solve_states (see above)")
    ap.add_argument("--parent", default=None, help="--stream: another checkout whose solve_states is the chunked side")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rollout_bench.py measures on the GPU; there is no CPU path"
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    if args.stream:
        path = out / "r15_rollout_stream.json"
        res = json.loads(path.read_text()) if path.exists() else {}
        configs = ["a", "a16"] if args.configs == "a,a9,a16" else args.configs.split(",")
        parent = load_parent(args.parent) if args.parent else None
        reps = 7 if args.reps == 20 else args.reps
        done = {(r["config"], r["zero_share"], r["R"]): r for r in res.get("dataset", [])}
        for r in part_stream(configs, parent, reps, min(args.warmup, 1)):
            done[(r["config"], r["zero_share"], r["R"])] = r
        res["dataset"] = [done[k] for k in sorted(done)]
        res["entries"] = part_slot_entries(50, 5)
        res["device"] = torch.cuda.get_device_name(0)
        res.setdefault("commands", []).append(" ".join(sys.argv))
        path.write_text(json.dumps(res, indent=1))
        print(f"wrote {path}")
        return
    if args.masked:
        path = out / "r14_rollout_masked.json"
        res = json.loads(path.read_text()) if path.exists() else {}
        configs = [c for c in args.configs.split(",") if c != "a9"] if args.configs == "a,a9,a16" else args.configs.split(",")
        done = {(r["config"], r["active_fraction"]): r for r in res.get("masked_step", [])}
        for r in part_masked(configs, [float(x) for x in args.fractions.split(",")], args.reps, args.warmup, args.repeats):
            done[(r["config"], r["active_fraction"])] = r
        res["masked_step"] = [done[k] for k in sorted(done, key=lambda k: (k[0], -k[1]))]
        res["device"] = torch.cuda.get_device_name(0)
        res.setdefault("commands", []).append(" ".join(sys.argv))
        path.write_text(json.dumps(res, indent=1))
        print(f"wrote {path}")
        return
    path = out / "r12_rollout.json"
    res = json.loads(path.read_text()) if path.exists() else {}
    parts = args.parts.split(",")
    if "a" in parts:
        res["advance_vs_composition"] = part_a(args.reps, args.warmup)
    if "b" in parts:
        done = {r["config"]: r for r in res.get("full_rollout", [])}
        for r in part_b(args.configs.split(","), args.reps, args.warmup):
            done[r["config"]] = r
        res["full_rollout"] = [done[k] for k in sorted(done)]
    if "c" in parts:
        res["in_use"] = part_c()
    res["device"] = torch.cuda.get_device_name(0)
    res.setdefault("commands", []).append(" ".join(sys.argv))
    path.write_text(json.dumps(res, indent=1))
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
