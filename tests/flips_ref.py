"""Host restatement of include/tensor_game_flips.h, straight from its text (numpy and Python integers, the oracle's
Philox): ``begin`` and ``advance`` with a full-scan reduce and a full match enumeration, no shortcuts; the standard
matmul lists and the planted lists both test files use.  Nothing here calls the library.

A walk's list is held as the header names it: per term the normalised vectors n_0, n_1, n_2 and the sign s, so that
the term is s * n_0 (x) n_1 (x) n_2 and its stored form is (n_0, n_1, s * n_2).

``step``, ``reduce`` and ``advance`` take an optional ``events`` (a ``collections.Counter``) and count in it the events
the header's rules define (EVENTS below): which branch of a rule a step took, not how a kernel implements it.  The
gadget lists at the end place the few terms that can match at chosen slots, so that the slots decide the branch."""
import functools
from collections import Counter

import numpy as np

from oracle import tensor_game as O

BAD_LENGTH, BAD_RANGE, BAD_SRC = 1, 2, 4
MAX_K, MAX_STEPS, DOMAIN = 128, 65536, 0x46000000
STATE_NAMES = ("cur", "cur_rank", "best", "best_rank", "best_step", "flips", "state")


def _norm(vec):
    """(vec or -vec with its first non-zero value positive, that value's sign; sign 0 for the zero vector)."""
    for x in vec:
        if x:
            return (vec, 1) if x > 0 else (tuple(-y for y in vec), -1)
    return vec, 0


def term_from_raw(raw3):
    """[n_0, n_1, n_2, s] of a term given by three integer vectors, or None for a null term."""
    ns, s = [], 1
    for v in raw3:
        n, sg = _norm(tuple(int(x) for x in v))
        if sg == 0:
            return None
        ns.append(n)
        s *= sg
    return [ns[0], ns[1], ns[2], s]


# What ``events`` counts, per step of ``advance`` (never inside ``begin``):
EVENTS = ("accepted", "refused", "m0", "m1", "m2",      # the step's outcome; the drawn match's mode
          "match_i_ge64", "match_straddle",               # the drawn match has i >= 64; has i < 64 <= j
          "null_a", "null_b", "null_both",                # the flip leaves a' null; b' null; both
          "null_lo_hi_last",                              # only the lower slot is null and the higher one is slot L-1
          "null_hi_not_last",                             # the higher slot is null and is not slot L-1: the last moves in
          "move_ge64_to_lt64",                            # a removal moves the term of a slot >= 64 into a slot < 64
          "merge_d0", "merge_d1", "merge_d2", "cancel",   # a reduce merges in mode d; removes a pair with z = 0
          "cancel_with_third",                            # ... a pair that is not the two terms the flip just wrote
          "passed_over", "share3",                        # a scan passes a pair over for the bound; visits a pair that
          "multi_merge")                                  #   shares all three modes; a reduce merges or cancels twice


def _remove(terms, p, events=None):
    """Removing slot p moves the last live term into p and decrements L."""
    last = terms.pop()
    if p < len(terms):
        terms[p] = last
        if events is not None and len(terms) >= 64 > p:
            events["move_ge64_to_lt64"] += 1


def reduce(terms, bound, events=None, flipped=()):
    """The full scan: pairs i < j in ascending (i, j) order; after a merge the scan restarts.  ``flipped``: the two term
    objects the step's flip wrote (for the event cancel_with_third)."""
    n_merged = 0
    while True:
        merged = False
        L = len(terms)
        for i in range(L):
            ti = terms[i]
            for j in range(i + 1, L):
                tj = terms[j]
                shared = [ti[m] == tj[m] for m in range(3)]
                if sum(shared) < 2:
                    continue
                d = 2 if all(shared) else shared.index(False)
                z = tuple(ti[3] * a + tj[3] * b for a, b in zip(ti[d], tj[d]))
                if events is not None and all(shared):
                    events["share3"] += 1
                if any(abs(x) > bound for x in z):
                    if events is not None:
                        events["passed_over"] += 1
                    continue                       # skipped: z stays what it is while neither term changes
                if not any(z):
                    if events is not None:
                        events["cancel"] += 1
                        if not (len(flipped) == 2 and {id(ti), id(tj)} == {id(flipped[0]), id(flipped[1])}):
                            events["cancel_with_third"] += 1
                    _remove(terms, j, events)
                    _remove(terms, i, events)
                else:
                    if events is not None:
                        events["merge_d%d" % d] += 1
                    n, sg = _norm(z)
                    new = list(ti)
                    new[d], new[3] = n, sg
                    terms[i] = new
                    _remove(terms, j, events)
                merged = True
                n_merged += 1
                break
            if merged:
                break
        if not merged:
            if events is not None and n_merged >= 2:
                events["multi_merge"] += 1
            return


def matches(terms):
    """All (i, j, m) with i < j < L and n_m(i) == n_m(j), in ascending (i, j, m) order."""
    L = len(terms)
    return [(i, j, m) for i in range(L) for j in range(i + 1, L) for m in range(3) if terms[i][m] == terms[j][m]]


def to_rows(terms, K, S, shift):
    """The stored form as tokens: int8 (K,3S), zero bytes at and beyond L."""
    out = np.zeros((K, 3 * S), dtype=np.int8)
    for t, (n0, n1, n2, s) in enumerate(terms):
        out[t] = np.array(n0 + n1 + tuple(s * x for x in n2), dtype=np.int64) + shift
    return out


def from_rows(rows, L, S, shift):
    f = np.asarray(rows[:L], dtype=np.int64) - shift
    return [term_from_raw((r[:S], r[S:2 * S], r[2 * S:])) for r in f]


def begin(tokens, lengths, src, bound, shift):
    """(state dict of numpy arrays, status bits) of ``tg_flip_begin``."""
    tokens = np.asarray(tokens)
    M, K, A3 = tokens.shape
    S = A3 // 3
    W = M if src is None else len(src)
    st = {"cur": np.zeros((W, K, A3), np.int8), "cur_rank": np.zeros(W, np.int32), "best": np.zeros((W, K, A3), np.int8),
          "best_rank": np.zeros(W, np.int32), "best_step": np.zeros(W, np.int64), "flips": np.zeros(W, np.int64),
          "state": np.zeros(W, np.int32)}
    status = 0
    for w in range(W):
        m = w if src is None else int(src[w])
        bad = 0
        if m < 0 or m >= M:
            bad = BAD_SRC
        elif lengths[m] < 0 or lengths[m] > K:
            bad = BAD_LENGTH
        else:
            L = int(lengths[m])
            f = tokens[m, :L].astype(np.int64) - shift
            if (np.abs(f) > bound).any():
                bad = BAD_RANGE
        if bad:
            status |= bad
            st["state"][w] = -1
            continue
        terms = [t for t in (term_from_raw((r[:S], r[S:2 * S], r[2 * S:])) for r in f) if t is not None]
        reduce(terms, bound)
        st["cur"][w] = st["best"][w] = to_rows(terms, K, S, shift)
        st["cur_rank"][w] = st["best_rank"][w] = len(terms)
    return st, status


def draws(seed, g, step0, n):
    """o.x of Philox-4x32-10 for steps step0 .. step0 + n - 1 of walk g."""
    return [int(x) for x in draws_of_walks(seed, [g], step0, n)[0]]


def draws_of_walks(seed, gs, step0, n):
    """uint32 (len(gs), n): o.x for steps step0 .. step0 + n - 1 of the walks with the global ids ``gs`` (Python
    integers below 2^64), in one Philox call."""
    t = np.tile((np.arange(n, dtype=np.uint64) + np.uint64(step0)).astype(np.uint32), len(gs))
    lo = np.repeat(np.array([g & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    hi = np.repeat(np.array([(g >> 32) & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    ctr = np.stack([lo, hi, t, np.full(len(t), DOMAIN, np.uint32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return O.philox4x32_10(ctr, np.broadcast_to(key, (len(t), 2)))[:, 0].reshape(len(gs), n)


def step(terms, ox, bound, events=None):
    """One step on a walking list.  Returns None when there is no match (stuck), else (variant, accepted)."""
    ms = matches(terms)
    C = len(ms)
    if C == 0:
        return None
    c = (ox * 8 * C) >> 32
    i, j, m = ms[c >> 3]
    variant = c & 7
    if events is not None:
        events["m%d" % m] += 1
        if i >= 64:
            events["match_i_ge64"] += 1
        elif j >= 64:
            events["match_straddle"] += 1
    eps = -1 if variant & 1 else 1
    q, r = [x for x in range(3) if x != m]
    if variant & 2:
        q, r = r, q
    a, b = (j, i) if variant & 4 else (i, j)
    ta, tb = terms[a], terms[b]
    new_q = tuple(x + eps * y for x, y in zip(ta[q], tb[q]))
    new_r = tuple(tb[3] * y - eps * ta[3] * x for x, y in zip(ta[r], tb[r]))
    if any(abs(x) > bound for x in new_q + new_r):
        if events is not None:
            events["refused"] += 1
        return variant, False
    raw_a, raw_b = [None] * 3, [None] * 3
    raw_a[m], raw_a[q], raw_a[r] = ta[m], new_q, tuple(ta[3] * x for x in ta[r])
    raw_b[m], raw_b[q], raw_b[r] = tb[m], tb[q], new_r
    na, nb = term_from_raw(raw_a), term_from_raw(raw_b)
    if events is not None:
        events["accepted"] += 1
        for name, hit in (("null_a", na is None), ("null_b", nb is None), ("null_both", na is None and nb is None)):
            events[name] += hit
        null_hi, null_lo = (na, nb)[a < b] is None, (na, nb)[a > b] is None
        events["null_lo_hi_last"] += null_lo and not null_hi and max(a, b) == len(terms) - 1
        events["null_hi_not_last"] += null_hi and max(a, b) != len(terms) - 1
    if na is not None:
        terms[a] = na
    if nb is not None:
        terms[b] = nb
    for p in sorted((p for p, t in ((a, na), (b, nb)) if t is None), reverse=True):   # the higher slot first
        _remove(terms, p, events)
    reduce(terms, bound, events, tuple(t for t in (na, nb) if t is not None))
    return variant, True


def advance(st, seed, walk0, step0, n_steps, bound, shift, trace=None, on_step=None, events=None):
    """``tg_flip_advance`` in place on the state dict.  ``trace`` (a list) receives (w, t, variant, accepted) per step
    that drew; ``on_step(w, t, terms)`` sees every list after its step; ``events`` (a Counter) counts EVENTS."""
    W, K, A3 = st["cur"].shape
    S = A3 // 3
    walking = [w for w in range(W) if st["state"][w] == 0 and 0 <= st["cur_rank"][w] <= K]
    all_ox = draws_of_walks(seed, [(walk0 + w) & (2 ** 64 - 1) for w in walking], step0, n_steps).tolist()
    for w, ox in zip(walking, all_ox):
        terms = from_rows(st["cur"][w], int(st["cur_rank"][w]), S, shift)
        for k in range(n_steps):
            t = step0 + k
            res = step(terms, ox[k], bound, events)
            if res is None:
                st["state"][w] = 1
                break
            if trace is not None:
                trace.append((w, t, res[0], res[1]))
            st["flips"][w] += int(res[1])
            if on_step is not None:
                on_step(w, t, terms)
            if len(terms) < st["best_rank"][w]:
                st["best"][w] = to_rows(terms, K, S, shift)
                st["best_rank"][w] = len(terms)
                st["best_step"][w] = t + 1
        st["cur"][w] = to_rows(terms, K, S, shift)
        st["cur_rank"][w] = len(terms)
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def term_sum(rows, L, S, shift):
    f = np.asarray(rows[:L], dtype=np.int64) - shift
    return np.einsum("ti,tj,tl->ijl", f[:, :S], f[:, S:2 * S], f[:, 2 * S:])


# ---- the lists the tests start from ----------------------------------------------------------------------------------
def standard_matmul(n, shift=1, K=None):
    """The standard algorithm of <n,n,n>: n^3 terms a_ij (x) b_jk (x) c_ik in the layout of the matmul tensor
    (entry (i*n+j, j*n+k, i*n+k), as tg_reset_matmul_i8 writes it).  Returns (tokens int8 (K,3S), length)."""
    S = n * n
    K = n ** 3 if K is None else K
    rows = np.zeros((K, 3 * S), dtype=np.int64)
    t = 0
    for i in range(n):
        for j in range(n):
            for k in range(n):
                rows[t, i * n + j] = rows[t, S + j * n + k] = rows[t, 2 * S + i * n + k] = 1
                t += 1
    rows[:t] += shift
    return rows.astype(np.int8), t


def pool_list(rng, S, K, L, pool, shift, nnz=None):
    """L random terms whose factors come from a pool of ``pool`` vectors per mode with values in {-1, 0, 1}, so that
    matches are plentiful.  ``nnz``: at most that many values of a pool vector are non-zero (sums of two sparse vectors
    stay inside a bound of 1 often enough for flips to be accepted at large S)."""
    vecs = rng.integers(-1, 2, size=(3, pool, S))
    if nnz is not None:
        keep = np.zeros((3, pool, S), dtype=bool)
        for m in range(3):
            for p in range(pool):
                keep[m, p, rng.choice(S, size=nnz, replace=False)] = True
        vecs = np.where(keep, vecs, 0)
    vecs[:, :, 0] = np.where(vecs.any(axis=2), vecs[:, :, 0], 1)        # no zero vector in the pool
    rows = np.zeros((K, 3 * S), dtype=np.int64)
    for t in range(L):
        rows[t] = np.concatenate([vecs[m, rng.integers(pool)] for m in range(3)])
    rows[:L] += shift
    return rows.astype(np.int8), L


def planted_list(rng, S, K, bound, shift, rot=0):
    """A list of exactly K rows with the cases ``begin`` has to get right: null terms, unnormalised signs, a term split
    as w' + w'', a cancelling pair, three terms sharing (u, v), and a merge that leaves the bound.  The groups are
    rotated by ``rot`` before the list is cut to K rows (a short list holds only some of them), and the order is
    shuffled, so the cases land in every slot, the last lane and a lane's second slot included."""
    def vec():
        v = rng.integers(-1, 2, size=S)
        if not v.any():
            v[rng.integers(S)] = 1
        return v

    zero = np.zeros(S, np.int64)
    groups = []
    u, v, w = vec(), vec(), vec()
    groups.append([np.concatenate([u, v, zero]), np.concatenate([zero, v, w])])                        # null terms
    groups.append([np.concatenate([-vec(), -vec(), vec()])])                                            # signs
    w1 = vec()
    w2 = np.where(w1 == 0, rng.integers(-1, 2, size=S), 0)                                              # split: w1 + w2
    if not w2.any():
        w2 = -w1                                                                                        # (cancels)
    u, v = vec(), vec()
    groups.append([np.concatenate([u, v, w1]), np.concatenate([-u, v, -w2])])
    u, v, w = vec(), vec(), vec()
    groups.append([np.concatenate([u, v, w]), np.concatenate([u, -v, w])])                              # cancelling
    u, v = vec(), vec()
    e = np.zeros((3, S), np.int64)
    e[0, 0] = e[1, S - 1] = e[2, S // 2] = 1
    groups.append([np.concatenate([u, v, e[k]]) for k in range(3)])                                     # three share (u,v)
    u, v, w = vec(), vec(), vec() * bound
    groups.append([np.concatenate([u, v, w]), np.concatenate([u, v, w])])                               # 2w leaves the bound
    groups = groups[rot % len(groups):] + groups[:rot % len(groups)]
    rows = [r for g in groups for r in g][:K]
    while len(rows) < K:
        rows.append(np.concatenate([vec(), vec(), vec()]))
    rows = np.stack(rows)[rng.permutation(K)]
    return (rows + shift).astype(np.int8), K




# ---- gadget lists: the slots of the few terms that can match decide which branch of a rule a step takes --------------
def _sparse_free_vec(rng, S, hi):
    """A normalised vector with values in [-hi, hi], at least two of them non-zero (no multiple of a unit vector)."""
    while True:
        v = tuple(int(x) for x in rng.integers(-hi, hi + 1, size=S))
        if sum(1 for x in v if x) >= 2:
            return _norm(v)[0]


def _inert_rows(rng, S, K, L, bound, taken, skip):
    """int64 (K,3S) values: inert terms in stored form in the slots < L that are not in ``skip`` -- normalised vectors
    that are pairwise distinct in every mode and not in ``taken``."""
    rows = np.zeros((K, 3 * S), dtype=np.int64)
    used = [set(taken), set(taken), set(taken)]
    for t in range(L):
        if t in skip:
            continue
        for m in range(3):
            while True:
                n = _sparse_free_vec(rng, S, bound)
                if n not in used[m]:
                    break
            used[m].add(n)
            rows[t, m * S:(m + 1) * S] = n
        if rng.integers(2):
            rows[t, 2 * S:] *= -1                         # the stored form carries the term's sign in w
    return rows


def gadget_list(rng, S, K, L, bound, shift, dup, hidden, quad):
    """A list of L terms of which only eight can match, the *gadgets*; the others are *inert*: their normalised vectors
    are pairwise distinct in every mode and differ from every gadget's (and from the gadgets' doubles), so every match
    of the list as ``begin`` leaves it involves a gadget.  Needs S >= 5 and bound >= 2.  All gadget vectors have
    values in {-1, 0, 1} unless stated.
      dup = (p0, p1):    the duplicated term (u, v, w) in both slots, w with a value equal to ``bound``.  The pair
                         shares all three modes; its merge 2w leaves the bound, so every reduce passes it over.  A flip
                         on its match in mode 2 with eps = -1 leaves a' null, with eps = +1 b' null, the other term
                         doubled in a mode where the double stays inside the bound.
      hidden = (c0, c1): x (x) 2y (x) w in slot c0 and -(x (x) y (x) 2w) in slot c1.  They share mode 0 alone, so
                         ``begin`` keeps them; the flip with eps = -1, (q, r) = (1, 2) and a = c0 turns them into
                         x y w and -(x y w), which cancel in its reduce.
      quad = (d0, d1, t1, t2): x (x) 2y (x) wa in d0, x (x) y (x) wb in d1 (wa and wb with disjoint supports),
                         x' (x) y (x) wa in t1 and x (x) y' (x) (wa + wb) in t2.  No two of them share two modes.  The
                         same flip, with a = d0, makes x y wa and x y (wa + wb): the two merge in mode 2 if the scan
                         meets that pair first; if it meets (d0, t1) first, d0 and t1 merge in mode 0 and then d1
                         and t2 in mode 1 -- two merges in one reduce.  The slots decide.
    Nothing merges in ``begin``, so every term keeps its slot.  Returns (tokens int8 (K,3S), L)."""
    slots = (*dup, *hidden, *quad)
    assert S >= 5 and bound >= 2 and len(set(slots)) == 8 and max(slots) < L <= K

    while True:
        u, v, x, y, w2, qx, qy, wa, wb, qx1, qy1 = (_sparse_free_vec(rng, S, 1) for _ in range(11))
        w = u[:S - 1] + (bound,)                          # (u, v, w): w normalised, with a value equal to the bound
        wab = tuple(a + b for a, b in zip(wa, wb))
        taken = set()
        for g in (u, v, w, x, y, w2, qx, qy, wa, wb, qx1, qy1, wab):
            taken |= {g, tuple(2 * e for e in g)}
        if len(taken) == 26 and not any(a and b for a, b in zip(wa, wb)) and any(u[:S - 1]):
            break
    rows = _inert_rows(rng, S, K, L, bound, taken, slots)
    two = lambda g: tuple(2 * e for e in g)               # noqa: E731
    for p, term in zip(slots, ((u, v, w), (u, v, w), (x, two(y), w2), (x, y, two(tuple(-e for e in w2))),
                               (qx, two(qy), wa), (qx, qy, wb), (qx1, qy, wa), (qx, qy1, wab))):
        rows[p] = np.concatenate(term)
    rows[:L] += shift
    return rows.astype(np.int8), L


# name: (K, L, dup, hidden, quad, W, n_steps, the events its slots make the walks reach, beyond ALWAYS).  One term per
# lane at K <= 64, two at K = 128; at most 64 walks where L > 64 (the restatement's time).
# The merges do not hang on the slots alone: besides the quad's direct flip, longer paths reach every mode everywhere.
ALWAYS = ("accepted", "refused", "m0", "m1", "m2", "null_a", "null_b", "cancel", "passed_over", "share3",
          "merge_d0", "merge_d1", "merge_d2", "multi_merge")
GADGET_CASES = {
    "K8 dup 0,1": (8, 8, (0, 1), (5, 6), (2, 3, 4, 7), 256, 8, ("null_hi_not_last",)),
    "K8 dup 0,7": (8, 8, (0, 7), (2, 6), (1, 5, 3, 4), 256, 8, ("null_lo_hi_last",)),
    "K8 dup 6,7": (8, 8, (6, 7), (3, 0), (5, 4, 1, 2), 256, 8, ("null_lo_hi_last",)),
    "K64 dup 0,63": (64, 64, (0, 63), (62, 10), (20, 30, 40, 50), 256, 8, ("null_lo_hi_last",)),
    "K64 dup 62,63": (64, 64, (62, 63), (5, 61), (1, 60, 59, 2), 256, 8, ("null_lo_hi_last",)),
    "K128 dup 0,127 hidden 64,63": (128, 128, (0, 127), (64, 63), (62, 65, 66, 126), 64, 10,
                                    ("null_lo_hi_last", "move_ge64_to_lt64", "match_straddle")),
    "K128 dup 126,127 hidden 10,125": (128, 128, (126, 127), (10, 125), (70, 124, 3, 64), 64, 10,
                                       ("null_lo_hi_last", "match_i_ge64", "match_straddle")),
    "K128 dup 63,64 hidden 100,90": (128, 128, (63, 64), (100, 90), (65, 127, 126, 1), 64, 10,
                                     ("null_hi_not_last", "move_ge64_to_lt64", "match_i_ge64", "match_straddle")),
    "K128 dup 64,127 hidden 126,65": (128, 128, (64, 127), (126, 65), (66, 67, 125, 124), 64, 10,
                                      ("null_lo_hi_last", "match_i_ge64")),
    "K128 dup 62,127 hidden 10,126": (128, 128, (62, 127), (10, 126), (63, 64, 2, 125), 64, 10,
                                      ("null_lo_hi_last", "move_ge64_to_lt64", "match_straddle")),
    "K128 L100 dup 64,99 hidden 98,3": (128, 100, (64, 99), (98, 3), (63, 65, 97, 96), 64, 10,
                                        ("null_lo_hi_last", "move_ge64_to_lt64", "match_i_ge64", "match_straddle")),
    "K128 L100 dup 98,99 hidden 63,64": (128, 100, (98, 99), (63, 64), (97, 0, 96, 65), 64, 10,
                                         ("null_lo_hi_last", "move_ge64_to_lt64", "match_i_ge64", "match_straddle")),
}
GADGET_S, GADGET_BOUND, GADGET_SEED, MIN_EVENTS = 5, 2, 11, 8


@functools.lru_cache(maxsize=None)
def gadget_ref(name):
    """(tokens (K,3S), L, W, n_steps, the restatement's state after n_steps, its event counts) of a gadget case --
    computed once; the state is shared, so nobody changes it."""
    K, L, dup, hidden, quad, W, n_steps, _ = GADGET_CASES[name]
    rng = np.random.default_rng(sorted(GADGET_CASES).index(name))
    tokens, L = gadget_list(rng, GADGET_S, K, L, GADGET_BOUND, GADGET_BOUND, dup, hidden, quad)
    st, status = begin(tokens[None], [L], np.zeros(W, dtype=np.int64), GADGET_BOUND, GADGET_BOUND)
    assert status == 0 and (st["cur_rank"] == L).all() and np.array_equal(st["cur"][0], tokens)   # every term kept its slot
    events = Counter()
    advance(st, GADGET_SEED, 0, 0, n_steps, GADGET_BOUND, GADGET_BOUND, events=events)
    return tokens, L, W, n_steps, st, events


# An unreduced list, which only a hand-written state can hold: u (x) v (x) w in slot p0 and -(u (x) v (x) w) in slot p1.
# ``begin`` would cancel the pair; written into ``cur`` directly it is walked as it is, and every flip on it with
# eps = -1 leaves both a' and b' null -- the one event no walk reaches from a reduced list.  Both removals then move
# inert terms, so the order "the higher slot first" shows in the rows.
ANTIPAIR_CASES = {8: ((8, 0, 1), (8, 2, 7), (8, 3, 5), (7, 1, 4)),
                  128: ((128, 63, 64), (128, 10, 127), (128, 64, 126), (128, 0, 1), (100, 62, 99), (100, 70, 98))}
ANTIPAIR_WALKS, ANTIPAIR_STEPS = 16, 3


@functools.lru_cache(maxsize=None)
def antipair_ref(K):
    """(the hand-written state, the restatement's state after ANTIPAIR_STEPS steps, its event counts): ANTIPAIR_WALKS
    walks per (L, p0, p1) of ANTIPAIR_CASES[K] -- computed once, nobody changes it."""
    S, bound = GADGET_S, GADGET_BOUND
    rng = np.random.default_rng(K)
    W = ANTIPAIR_WALKS * len(ANTIPAIR_CASES[K])
    st = {"cur": np.zeros((W, K, 3 * S), np.int8), "cur_rank": np.zeros(W, np.int32), "best": None,
          "best_rank": None, "best_step": np.zeros(W, np.int64), "flips": np.zeros(W, np.int64), "state": np.zeros(W, np.int32)}
    for c, (L, p0, p1) in enumerate(ANTIPAIR_CASES[K]):
        u, v, w = (_sparse_free_vec(rng, S, 1) for _ in range(3))
        taken = {u, v, w} | {tuple(2 * e for e in g) for g in (u, v, w)}
        rows = _inert_rows(rng, S, K, L, bound, taken, (p0, p1))
        rows[p0] = np.concatenate([u, v, w])
        rows[p1] = np.concatenate([u, v, tuple(-e for e in w)])
        rows[:L] += bound
        st["cur"][c * ANTIPAIR_WALKS:(c + 1) * ANTIPAIR_WALKS] = rows.astype(np.int8)
        st["cur_rank"][c * ANTIPAIR_WALKS:(c + 1) * ANTIPAIR_WALKS] = L
    st["best"], st["best_rank"] = st["cur"].copy(), st["cur_rank"].copy()
    want, events = copy_state(st), Counter()
    advance(want, GADGET_SEED, 0, 0, ANTIPAIR_STEPS, bound, bound, events=events)
    return st, want, events
