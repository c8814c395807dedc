#!/usr/bin/env python3
"""Golden fixture for the batched search (include/tensor_game_search.h), recorded by RUNNING THE REFERENCE's
``act.actor_prediction`` (/root/reference/act.py:8-64) with a stand-in for the network.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_search.py      (build container only)

The stand-in's ``fwd_infer`` returns k candidate tokens and a q value that are a seeded function of (case, head bytes,
attempt) -- attempt = how many times this game has already asked about this head -- drawn from a small per-case pool
of actions (null actions included) or, with some probability, fresh; so transpositions, null and duplicate candidates
and retries all happen.  Everything else is the reference's own code: mc_ts, extend_tree, backward_pass,
select_next_state, get_improved_policy and the rewards.  Stored per case ``<c>_``:
    meta       int64 [S, T, k, n_sim, max_actions, n_bar, n_logits, horizon, games, skipped]
    start      int8 (G,T,S,S,S)             the initial states
    states     int8 (G,max_actions,T,S,S,S) state_seq, zero past the length
    policy     f32  (G,max_actions,3S,n_logits)
    rewards    int64 (G,max_actions), lengths int64 (G,)
    root_n / root_q  f32 (G,max_actions,k)  the root's visit counts / Q values after each move's simulations
    root_nc    int32 (G,max_actions)        its number of children;  choice int32 (G,max_actions) the chosen index
    call_*     every fwd_infer call: game, head int8 (S,S,S), attempt, scalar (idx), tokens int8 (k,3S), q f32
Games whose run raises (a terminal leaf inside the horizon: UnboundLocalError) or does not finish within 60 s (a
retry or descent loop) are skipped; ``skipped`` counts them.  The archive is written deterministically (fixed member
order and time stamps), so a rerun reproduces it byte for byte.  Nothing of the reference is copied.
"""
import io
import os
import signal
import sys
import tempfile
import zipfile
import zlib
from pathlib import Path

import numpy as np

REF = "/root/reference"
OUT = Path(__file__).resolve().parent / "search_games.npz"

# name, S, T, k, n_sim, max_actions, n_bar, games, seed, start kind
CASES = [
    ("S4_T1", 4, 1, 6, 4, 4, 100, 4, 101, "strassen"),
    ("S4_T2", 4, 2, 6, 16, 8, 2, 4, 102, "strassen"),
    ("S4_T2_lowrank", 4, 2, 5, 16, 4, 100, 4, 103, "rank3"),
    ("S3_T1", 3, 1, 6, 16, 8, 100, 4, 104, "random"),
    ("S5_T2", 5, 2, 4, 4, 8, 2, 3, 105, "random"),
    ("S16_T1", 16, 1, 4, 4, 4, 2, 2, 106, "random"),
]
N_LOGITS, HORIZON = 3, 5


class Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise Timeout()


def make_pool(rng, S, n=5):
    pool = []
    while len(pool) < n:
        a = rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2], size=3 * S).astype(np.int64)
        if all((a[x * S:(x + 1) * S] != 1).any() for x in range(3)):
            pool.append(a)
    pool.append(np.ones(3 * S, np.int64))          # a null action (u = v = w = 0)
    z = pool[0].copy()
    z[S:2 * S] = 1                                  # null through v = 0 only
    pool.append(z)
    return pool


class StandIn:
    """The network: fwd_infer(state, scalars) -> (tokens (1,k,3S), None, q (1,)), a seeded function of
    (case seed, head bytes, attempt)."""

    device = "cpu"

    def __init__(self, torch, S, k, seed, pool):
        self.torch, self.S, self.k, self.seed, self.pool = torch, S, k, seed, pool
        self.n_steps, self.n_logits = 3 * S, N_LOGITS
        self.attempts, self.calls = {}, []

    def fwd_infer(self, state, scalars):
        head = state[0, 0].numpy().astype(np.int8)
        hb = head.tobytes()
        a = self.attempts.get(hb, 0)
        self.attempts[hb] = a + 1
        rng = np.random.default_rng([self.seed, a, zlib.crc32(hb)])
        pick = rng.integers(0, len(self.pool), size=self.k)
        fresh = rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2], size=(self.k, 3 * self.S))
        use_fresh = rng.random(self.k) < (0.2 if a == 0 else 0.6)
        acts = np.where(use_fresh[:, None], fresh, np.stack([self.pool[i] for i in pick])).astype(np.int64)
        q = np.float32(rng.uniform(-3.0, 1.0))
        self.calls.append((head.copy(), a, float(scalars[0, 0]), acts.astype(np.int8), q))
        return (self.torch.from_numpy(acts).view(1, self.k, 3 * self.S), None,
                self.torch.tensor([q], dtype=self.torch.float32))


def start_state(kind, rng, S, T, utils, datasets):
    st = np.zeros((T, S, S, S), np.int8)
    if kind == "strassen":
        st[0] = datasets.get_strassen_tensor("cpu")[0].numpy().astype(np.int8)
    elif kind == "rank3":
        for _ in range(3):
            u, v, w = (rng.choice([-1, 0, 1], size=S) for _ in range(3))
            st[0] += np.einsum("i,j,k->ijk", u, v, w).astype(np.int8)
    else:
        st[0] = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(S, S, S)).astype(np.int8)
    return st


def run_case(torch, act, utils, datasets, name, S, T, k, n_sim, max_actions, n_bar, games, seed, kind):
    rng = np.random.default_rng(seed)
    pool = make_pool(rng, S)
    orig_mc_ts = act.mc_ts
    out = {key: [] for key in ("start", "states", "policy", "rewards", "lengths", "root_n", "root_q", "root_nc", "choice")}
    calls = []
    skipped = 0
    tries = 0
    while len(out["start"]) < games:
        tries += 1
        assert tries < 50 * games, f"{name}: too many skipped games"
        start = start_state(kind, rng, S, T, utils, datasets)
        model = StandIn(torch, S, k, seed, pool)
        roots = []

        def mc_ts(model_, root_state, *args):
            res = orig_mc_ts(model_, root_state, *args)
            info = res[2][utils.state_to_str(utils.get_head_state(root_state))]
            n, q = info[3][0].numpy().copy(), info[4][0].numpy().copy()
            roots.append((n, q, int(torch.from_numpy(q).argmax())))
            return res

        act.mc_ts = mc_ts
        signal.signal(signal.SIGALRM, _alarm)
        signal.alarm(60)
        try:
            st_seq, pol_seq, rew_seq = act.actor_prediction(model, torch.from_numpy(start.astype(np.float32)),
                                                            max_actions, n_sim, n_bar)
        except (UnboundLocalError, Timeout):
            skipped += 1
            continue
        finally:
            signal.alarm(0)
            act.mc_ts = orig_mc_ts
        L = len(st_seq)
        g = len(out["start"])
        st = np.zeros((max_actions, T, S, S, S), np.int8)
        st[:L] = np.stack([s.numpy() for s in st_seq]).astype(np.int8)
        pol = np.zeros((max_actions, 3 * S, N_LOGITS), np.float32)
        pol[:L] = pol_seq.numpy()
        rew = np.zeros(max_actions, np.int64)
        rew[:L] = rew_seq.numpy()
        rn = np.zeros((max_actions, k), np.float32)
        rq = np.zeros((max_actions, k), np.float32)
        nc = np.zeros(max_actions, np.int32)
        ch = np.full(max_actions, -1, np.int32)
        assert len(roots) == L
        for m, (n, q, j) in enumerate(roots):
            rn[m, :len(n)], rq[m, :len(q)], nc[m], ch[m] = n, q, len(n), j
        for key, val in (("start", start), ("states", st), ("policy", pol), ("rewards", rew), ("lengths", L),
                         ("root_n", rn), ("root_q", rq), ("root_nc", nc), ("choice", ch)):
            out[key].append(val)
        calls += [(g, *c) for c in model.calls]
    arrays = {f"{name}_{key}": np.array(val) for key, val in out.items()}
    arrays[f"{name}_lengths"] = arrays[f"{name}_lengths"].astype(np.int64)
    arrays[f"{name}_meta"] = np.array([S, T, k, n_sim, max_actions, n_bar, N_LOGITS, HORIZON, games, skipped], np.int64)
    arrays[f"{name}_call_game"] = np.array([c[0] for c in calls], np.int32)
    arrays[f"{name}_call_head"] = np.stack([c[1] for c in calls])
    arrays[f"{name}_call_attempt"] = np.array([c[2] for c in calls], np.int32)
    arrays[f"{name}_call_scalar"] = np.array([c[3] for c in calls], np.float32)
    arrays[f"{name}_call_tokens"] = np.stack([c[4] for c in calls])
    arrays[f"{name}_call_q"] = np.array([c[5] for c in calls], np.float32)
    print(f"{name}: {games} games (skipped {skipped}), lengths {arrays[f'{name}_lengths'].tolist()}, "
          f"{len(calls)} model calls ({int((arrays[f'{name}_call_attempt'] > 0).sum())} retries)")
    return arrays


def write_npz(path, arrays):
    """np.savez_compressed with fixed member order and time stamps: reruns are byte-identical."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, member.getvalue())
    Path(path).write_bytes(buf.getvalue())


def main(out_path=OUT):
    sys.dont_write_bytecode = True
    os.chdir(tempfile.mkdtemp(prefix="golden_search_"))
    sys.path.insert(0, REF)
    import torch

    torch.manual_seed(0)
    import act  # noqa: E402  (reference)
    import datasets  # noqa: E402  (reference)
    import utils  # noqa: E402  (reference)

    arrays = {}
    for case in CASES:
        arrays.update(run_case(torch, act, utils, datasets, *case))
    write_npz(out_path, arrays)
    print(f"wrote {out_path} ({Path(out_path).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
