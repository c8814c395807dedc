"""numpy restatement of the sampled policy rollout (mat_mul_amd/rollout.py, include/tensor_game_rollout.h) on
oracle.tensor_game: one step (``advance``), the loop (``rollout``) and ``solutions``.  Shared by test_rollout_cpu.py and
test_gpu_rollout.py; reads nothing outside the repository."""
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import tensor_game as O  # noqa: E402


def fresh_records(G, S):
    """(best_nnz, hits, solved_step, solved_sample), int32 (G,) each, as a rollout starts."""
    return (np.full(G, S ** 3, np.int32), np.zeros(G, np.int32), np.full(G, -1, np.int32), np.full(G, -1, np.int32))


def advance(frames, tokens, n, step, records, scalars=None, overflow=None, actions=None, shift=1):
    """One step of every row (reference training.py:253-268 + :343-346).  frames int8 (B,T,S,S,S) newest first, tokens
    int8 (B,3S), rows group-major.  Returns (new frames, nnz int32 (B,), new records, new scalars, new overflow, new
    actions); no input is modified."""
    frames = np.asarray(frames)
    assert frames.dtype == np.int8
    B, T = frames.shape[:2]
    assert B % n == 0
    head, _, ovf = O.step_i8(frames[:, 0], np.asarray(tokens, np.int8), shift)      # :253-255, narrowed as the build does
    new = np.concatenate([head[:, None], frames], axis=1)[:, :-1]                  # :256-258
    nnz = O.nnz_per_game(head)                                                     # :266
    best, hits, sstep, ssample = (r.copy() for r in records)
    grouped = nnz.reshape(-1, n)
    m = grouped.min(axis=1)                                                        # :267
    best = np.minimum(best, m).astype(np.int32)                                    # :343-345, per group
    hit = m == 0
    hits = (hits + hit).astype(np.int32)                                           # :346
    first = np.argmax(grouped == 0, axis=1).astype(np.int32)                       # the LOWEST sample index at zero
    newly = hit & (sstep < 0)
    sstep = np.where(newly, np.int32(step), sstep).astype(np.int32)
    ssample = np.where(newly, first, ssample).astype(np.int32)
    if scalars is not None:
        scalars = (np.asarray(scalars, np.float32) + np.float32(1)).astype(np.float32)  # :268
    if overflow is not None:
        overflow = (np.asarray(overflow) | ovf).astype(np.uint8)
    if actions is not None:
        actions = np.array(actions, np.int8)
        actions[:, step] = tokens
    return new, nnz, (best, hits, sstep, ssample), scalars, overflow, actions


class Result:
    pass


def rollout(policy, states, scalars, n, max_actions, shift=1):
    """The loop of mat_mul_amd.rollout.sample_rollouts: policy(frames, scalars, rows, step) -> tokens int8 (B,3S)."""
    states = np.asarray(states, np.int8)
    G, T, S = states.shape[:3]
    frames = np.repeat(states, n, axis=0)
    scal = np.repeat(np.asarray(scalars, np.float32), n, axis=0)
    B = G * n
    rows = np.arange(B, dtype=np.int64)
    rec = fresh_records(G, S)
    overflow = np.zeros(B, np.uint8)
    actions = np.zeros((B, max_actions, 3 * S), np.int8)
    nnz = np.zeros(B, np.int32)
    r = Result()
    r.trace = []
    for step in range(max_actions):
        tokens = np.asarray(policy(frames, scal, rows, step), np.int8)
        frames, nnz, rec, scal, overflow, actions = advance(frames, tokens, n, step, rec, scal, overflow, actions, shift)
        r.trace.append(tuple(x.copy() for x in rec))
    r.n_samples, r.max_actions, r.shift = n, max_actions, shift
    r.best_nnz, r.hits, r.solved_step, r.solved_sample = rec
    r.frames, r.scalars, r.nnz, r.overflow, r.actions = frames, scal, nnz, overflow, actions
    r.lowest_rank = int(r.best_nnz.min()) if G else S ** 3
    r.num_hits = int(r.hits.sum())
    r.num_solved = int((r.solved_step >= 0).sum())
    return r


def solutions(r):
    """RolloutResult.solutions(): (groups, tokens (M,max_actions,3S) zero beyond the length, lengths)."""
    groups = np.nonzero(r.solved_step >= 0)[0].astype(np.int64)
    rows = groups * r.n_samples + r.solved_sample[groups]
    lengths = r.solved_step[groups].astype(np.int64) + 1
    tokens = r.actions[rows].copy()
    for m, L in enumerate(lengths):
        tokens[m, L:] = 0
    return groups, tokens, lengths


# ---- scripted policies on the recorded factorisations ---------------------------------------------------------------
def unused_factors(state, tokens, shift=1):
    """The unique subset of the rank-1 terms ``tokens`` (R,3S) that sums to ``state`` (S,S,S): indices, ascending."""
    terms = O.action_to_tensor(np.asarray(tokens), shift)  # (R,S,S,S) int64
    R = len(terms)
    bits = (np.arange(1 << R)[:, None] >> np.arange(R)[None, :]) & 1          # every subset
    sums = bits @ terms.reshape(R, -1)
    found = np.nonzero((sums == np.asarray(state, np.int64).reshape(1, -1)).all(axis=1))[0]
    assert len(found) == 1, found
    return [i for i in range(R) if bits[found[0], i]]


def null_action(S, shift):
    """Tokens of the zero rank-1 term (u = v = w = 0): the state does not change."""
    return np.full(3 * S, shift, np.int8)


def scripted_policy(scripts, S, n, slot, shift, seed=0, values=3):
    """Rows of sample ``slot`` play their group's script (a list of token rows), then the null action; the other
    samples play seeded random tokens in [0, values)."""
    G = len(scripts)
    rng = np.random.default_rng(seed)

    def policy(frames, scalars, rows, step):
        tok = rng.integers(0, values, size=(G * n, 3 * S)).astype(np.int8) + np.int8(shift - 1)
        for g, sc in enumerate(scripts):
            tok[g * n + slot] = sc[step] if step < len(sc) else null_action(S, shift)
        return tok

    return policy


# ---- the recorded factorisations (tests/golden; ``golden`` is conftest's loader) --------------------------------------
def strassen_scripts(golden, shift):
    """(states (448,1,4,4,4), scripts, rewards): for every dataset state the Strassen factors not yet used, as tokens of
    the vocabulary ``shift`` (1: the recorded ``tokens``; 2: tokens + 1, the vocabulary of ``ds_actions``)."""
    g = golden("strassen")
    tok = g["tokens"].astype(np.int8) + np.int8(shift - 1)
    scripts = []
    for state, reward in zip(g["ds_states"], g["ds_rewards"]):
        idx = unused_factors(state, g["tokens"], 1)
        assert len(idx) == -int(reward)
        scripts.append([tok[i] for i in idx])
    return g["ds_states"][:, None].astype(np.int8), scripts, -g["ds_rewards"].astype(np.int64)


def demo_cases(golden, sizes=(4, 9)):
    """(name, target (1,1,S,S,S), script) of the recorded fn_* demonstrations (shift 1) at the given sizes."""
    g = golden("synthetic_demos")
    out = []
    for key in g.files:
        m = re.fullmatch(r"(fn_S(\d+)_R\d+_\d+)_tokens", key)
        if m and int(m.group(2)) in sizes:
            out.append((m.group(1), g[m.group(1) + "_target"][None, None].astype(np.int8), list(g[key].astype(np.int8))))
    assert len(out) >= 2
    return out
