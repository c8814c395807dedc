"""Host restatement of include/tensor_game_flips_plus.h, straight from its text: ``advance`` with the choice between a
flip step and a plus step, and the plus itself.  Everything the header takes over from tensor_game_flips.h comes from
flips_ref.py unchanged: the terms, ``reduce``, ``matches``, the flip of ``step``, the removal of a slot and Philox.
Nothing here calls the library.

``advance`` takes an optional ``events`` (a ``collections.Counter``) and counts in it, besides the events of flips_ref,
the events the plus rule defines (PLUS_EVENTS below): which branch of the rule a step took."""
import functools
from collections import Counter
from itertools import permutations

import numpy as np

from oracle import tensor_game as O

import flips_ref as FR

STATE_NAMES = FR.STATE_NAMES + ("since", "pluses")
INT32_MAX = 2 ** 31 - 1
PERMS = sorted(permutations(range(3)))      # lexicographic: 012, 021, 102, 120, 201, 210

PLUS_EVENTS = ("plus_accepted", "plus_refused",                  # a plus step's outcome
               "plus_forced", "plus_timed",                       # why it was taken: C == 0; since >= plus_after (C > 0)
               "perm0", "perm1", "perm2", "perm3", "perm4", "perm5",   # the drawn (p, q, r)
               "plus_null_t1", "plus_null_t2", "plus_null_t3",    # an accepted plus leaves t1; t2; t3 null
               "plus_then_merge",                                 # the reduce of an accepted plus merges or cancels
               "stuck_at_cap",                                    # C == 0 with L >= 2 and L >= cap: stuck although plus exists
               "append_slot_ge64", "append_slot_64", "append_slot_Km1",   # an accepted plus's new slot L: >= 64; 64; K - 1
               "pair_i_ge64", "pair_straddle")                    # the drawn pair has i >= 64; has i < 64 <= j


def draws3_of_walks(seed, gs, step0, n):
    """uint32 (len(gs), n, 3): o.x, o.y, o.z for steps step0 .. step0 + n - 1 of the walks with the global ids ``gs``."""
    t = np.tile((np.arange(n, dtype=np.uint64) + np.uint64(step0)).astype(np.uint32), len(gs))
    lo = np.repeat(np.array([g & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    hi = np.repeat(np.array([(g >> 32) & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    ctr = np.stack([lo, hi, t, np.full(len(t), FR.DOMAIN, np.uint32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return O.philox4x32_10(ctr, np.broadcast_to(key, (len(t), 2)))[:, :3].reshape(len(gs), n, 3)


def plus(terms, oy, oz, bound, K, events=None):
    """Step 4 on a list with L >= 2 terms.  True if the plus was accepted."""
    L = len(terms)
    P = L * (L - 1) // 2
    c = (oy * P) >> 32
    i, j = [(i, j) for i in range(L) for j in range(i + 1, L)][c]
    v = (oz * 24) >> 32
    a, b = (j, i) if v & 1 else (i, j)
    eps = -1 if v & 2 else 1
    p, q, r = PERMS[v >> 2]
    if events is not None:
        events["perm%d" % (v >> 2)] += 1
        if i >= 64:
            events["pair_i_ge64"] += 1
        elif j >= 64:
            events["pair_straddle"] += 1
    ta, tb = terms[a], terms[b]
    A = {p: ta[p], q: ta[q], r: tuple(ta[3] * x for x in ta[r])}
    B = {p: tuple(eps * x for x in tb[p]), q: tb[q], r: tuple(eps * tb[3] * x for x in tb[r])}
    d1 = tuple(x - y for x, y in zip(A[p], B[p]))
    d2 = tuple(x + y for x, y in zip(A[r], B[r]))
    d3 = tuple(y - x for x, y in zip(A[q], B[q]))
    if any(abs(x) > bound for x in d1 + d2 + d3):
        if events is not None:
            events["plus_refused"] += 1
        return False
    raw1, raw2, raw3 = [None] * 3, [None] * 3, [None] * 3
    raw1[p], raw1[q], raw1[r] = d1, A[q], A[r]
    raw2[p], raw2[q], raw2[r] = B[p], A[q], d2
    raw3[p], raw3[q], raw3[r] = B[p], d3, B[r]
    t1, t2, t3 = FR.term_from_raw(raw1), FR.term_from_raw(raw2), FR.term_from_raw(raw3)
    if events is not None:
        events["plus_accepted"] += 1
        for name, t in (("plus_null_t1", t1), ("plus_null_t2", t2), ("plus_null_t3", t3)):
            events[name] += t is None
        if t2 is not None:
            events["append_slot_ge64"] += L >= 64
            events["append_slot_64"] += L == 64
            events["append_slot_Km1"] += L == K - 1
    terms[a] = t1
    terms.append(t2)                                   # slot L; L += 1
    terms[b] = t3
    for s in sorted((s for s, t in ((a, t1), (L, t2), (b, t3)) if t is None), reverse=True):   # the highest slot first
        FR._remove(terms, s, events)
    before = len(terms)
    FR.reduce(terms, bound, events)
    if events is not None and len(terms) < before:
        events["plus_then_merge"] += 1
    return True


def advance(st, seed, walk0, step0, n_steps, bound, shift, plus_after, plus_slack, on_step=None, events=None):
    """``tg_flip_advance_plus`` in place on the state dict (the seven of flips_ref and ``since``, ``pluses``).
    ``on_step(w, t, terms, cap)`` sees every list after its step, with the cap that step had."""
    W, K, A3 = st["cur"].shape
    S = A3 // 3
    walking = [w for w in range(W) if st["state"][w] == 0 and 0 <= st["cur_rank"][w] <= K]
    all_o = draws3_of_walks(seed, [(walk0 + w) & (2 ** 64 - 1) for w in walking], step0, n_steps).tolist()
    for w, o in zip(walking, all_o):
        terms = FR.from_rows(st["cur"][w], int(st["cur_rank"][w]), S, shift)
        since = int(st["since"][w])
        for k in range(n_steps):
            t = step0 + k
            ox, oy, oz = o[k]
            L = len(terms)
            C = len(FR.matches(terms))
            cap = min(K, int(st["best_rank"][w]) + plus_slack)
            want = C == 0 or since >= plus_after
            can = L >= 2 and L < cap
            if want and can:
                if events is not None:
                    events["plus_forced" if C == 0 else "plus_timed"] += 1
                if plus(terms, oy, oz, bound, K, events):
                    st["pluses"][w] += 1
                    since = 0
                else:
                    since = min(since + 1, INT32_MAX)
            elif C == 0:
                if events is not None and L >= 2:
                    events["stuck_at_cap"] += 1
                st["state"][w] = 1
                break
            else:
                res = FR.step(terms, ox, bound, events)
                st["flips"][w] += int(res[1])
                since = 0 if len(terms) < L else min(since + 1, INT32_MAX)
            if on_step is not None:
                on_step(w, t, terms, cap)
            if len(terms) < st["best_rank"][w]:
                st["best"][w] = FR.to_rows(terms, K, S, shift)
                st["best_rank"][w] = len(terms)
                st["best_step"][w] = t + 1
        st["cur"][w] = FR.to_rows(terms, K, S, shift)
        st["cur_rank"][w] = len(terms)
        st["since"][w] = since
    return st


def with_plus(st):
    """The state dict ``st`` of flips_ref with zeroed ``since`` and ``pluses`` (a fresh walk)."""
    W = len(st["state"])
    return {**st, "since": np.zeros(W, np.int32), "pluses": np.zeros(W, np.int64)}


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


# ---- the cases both test files run -----------------------------------------------------------------------------------
# name: (list, S, K, L, bound = shift, W, n_steps, plus_after, plus_slack, seed, the events the restatement must show)
@functools.lru_cache(maxsize=None)
def _reduced_pool(S):
    """A long reduced list in stored form: 200 pool terms with values in {-1, 0, 1} as ``begin`` at bound 2 leaves them
    (every pair that shares two modes merges there).  Any prefix of it is a reduced list too, and matches are plentiful."""
    rows, n = FR.pool_list(np.random.default_rng(7), S, 200, 200, 40, 2)
    terms = [t for t in FR.from_rows(rows, n, S, 2)]
    FR.reduce(terms, 2)
    assert len(terms) >= 120
    return terms


def _list(kind, S, K, L):
    if kind == "2x2":
        return FR.standard_matmul(2, K=K)
    if kind == "3x3":
        return FR.standard_matmul(3, K=K)
    if kind == "inert":
        rows = FR._inert_rows(np.random.default_rng(3), S, K, L, 1, set(), ())     # values in {-1, 0, 1}: room under bound 2
        rows[:L] += 2
        return rows.astype(np.int8), L
    if kind == "pool":                                    # begin keeps all L terms in their slots
        return FR.to_rows(_reduced_pool(S)[:L], K, S, 2), L
    raise KeyError(kind)


# The table of events: which of PLUS_EVENTS the restatement's counts must show (>= MIN_EVENTS) per case; together the
# cases reach every event (test_flips_plus_cpu.py checks both).  Seeds and plus_after were chosen on the CPU, with the
# restatement alone.  The short cap cases take too few pluses for all six permutations; the long ones show them.
PERM = ("perm0", "perm1", "perm2", "perm3", "perm4", "perm5")
TIMED = ("plus_accepted", "plus_refused", "plus_timed") + PERM
CASES = {
    "2x2": ("2x2", 4, 9, 8, 1, 64, 512, 16, 2, 0, TIMED + ("plus_forced", "plus_then_merge", "plus_null_t1", "plus_null_t2", "plus_null_t3")),
    "3x3": ("3x3", 9, 30, 27, 1, 16, 256, 8, 3, 0, TIMED),
    "inert": ("inert", 5, 8, 4, 2, 32, 32, 1000, 1, 0, ("plus_accepted", "plus_forced") + PERM),
    "inert full": ("inert", 5, 4, 4, 2, 8, 2, 1000, 1, 0, ("stuck_at_cap",)),      # L = K: no plus, stuck at once
    "cap K64": ("pool", 5, 64, 62, 2, 8, 128, 2, 64, 0, TIMED[:3] + ("append_slot_Km1",)),
    "slot64 K65": ("pool", 5, 65, 62, 2, 8, 128, 2, 64, 0, TIMED[:3] + ("append_slot_64", "append_slot_ge64", "append_slot_Km1")),
    "slot64 K128": ("pool", 5, 128, 62, 2, 8, 128, 2, 64, 0, TIMED + ("append_slot_64", "append_slot_ge64", "pair_straddle")),
    "last K128": ("pool", 5, 128, 120, 2, 4, 64, 1, 128, 0, TIMED + ("append_slot_ge64", "pair_i_ge64", "pair_straddle")),
}
MIN_EVENTS = FR.MIN_EVENTS


def start_state(name):
    """(tokens (K,3S), L, the restatement's begin state with zeroed since and pluses) of a case."""
    kind, S, K, L, bound, W = CASES[name][:6]
    tokens, L = _list(kind, S, K, L)
    st, status = FR.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), bound, bound)
    assert status == 0
    return tokens, L, with_plus(st)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(tokens, L, the begin state, the restatement's state after n_steps, its event counts) -- computed once; the
    states are shared, so nobody changes them."""
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = CASES[name]
    tokens, L, st = start_state(name)
    want, events = copy_state(st), Counter()
    advance(want, seed, 0, 0, n_steps, bound, bound, plus_after, plus_slack, events=events)
    return tokens, L, st, want, events
