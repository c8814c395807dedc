"""Host restatement of include/tensor_game_flips_mod2.h, straight from its text (numpy and Python integers, the oracle's
Philox): ``begin``, ``reduce`` with full scans, ``step``, ``advance`` with a trace, ``residual``.  No shortcuts: every
scan visits every pair, every step enumerates every match.  Nothing here calls the library.

A term is a list of three Python integers, the masks m_0, m_1, m_2; a walk's list is a list of terms.  The starting
lists come from flips_ref.py (``standard_matmul``, ``pool_list``, ``planted_list``)."""
import numpy as np

from oracle import tensor_game as O

BAD_LENGTH, BAD_SRC = 1, 4
MAX_K, MAX_STEPS, DOMAIN = 128, 65536, 0x46320000
INT32_MAX = 2 ** 31 - 1
STATE_NAMES = ("cur", "cur_rank", "best", "best_rank", "best_step", "flips", "state", "since", "pluses")
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def masks_of_row(row, S, shift):
    """The three masks of a token row: bit e of m_d = (row[d*S + e] - shift) & 1."""
    f = np.asarray(row, dtype=np.int64) - shift
    return [sum(int(f[d * S + e]) & 1 and 1 << e for e in range(S)) for d in range(3)]


def _remove(terms, p):
    """Removing slot p moves the last live term into p and decrements L."""
    last = terms.pop()
    if p < len(terms):
        terms[p] = last


def reduce(terms, events=None):
    """Full scans: pairs i < j in ascending (i, j) order; after a merge or a cancel the scan restarts at (0, 1)."""
    while True:
        acted = False
        L = len(terms)
        for i in range(L):
            for j in range(i + 1, L):
                a, b = terms[i], terms[j]
                shared = (a[0] == b[0], a[1] == b[1], a[2] == b[2])
                if shared[0] + shared[1] + shared[2] < 2:
                    continue
                if all(shared):
                    _remove(terms, j)
                    _remove(terms, i)
                    if events is not None:
                        events["cancel"] += 1
                else:
                    d = shared.index(False)
                    new = list(terms[i])
                    new[d] ^= terms[j][d]
                    terms[i] = new
                    _remove(terms, j)
                    if events is not None:
                        events["merge"] += 1
                acted = True
                break
            if acted:
                break
        if not acted:
            return


def matches(terms):
    """All (i, j, d) with i < j < L and m_d(i) == m_d(j), in ascending (i, j, d) order."""
    L = len(terms)
    return [(i, j, d) for i in range(L) for j in range(i + 1, L) for d in range(3) if terms[i][d] == terms[j][d]]


def to_rows(terms, K):
    """int32 (K,3): the masks as int32 bit patterns, zero at and beyond L."""
    out = np.zeros((K, 3), dtype=np.uint32)
    for t, term in enumerate(terms):
        out[t] = term
    return out.view(np.int32)


def from_rows(rows, L):
    return [[int(x) for x in r] for r in np.asarray(rows[:L]).view(np.uint32)]


def begin(tokens, lengths, src, shift):
    """(state dict of numpy arrays, status bits) of ``tg_flip2_begin``."""
    tokens = np.asarray(tokens)
    M, K, A3 = tokens.shape
    S = A3 // 3
    W = M if src is None else len(src)
    st = {"cur": np.zeros((W, K, 3), np.int32), "cur_rank": np.zeros(W, np.int32), "best": np.zeros((W, K, 3), np.int32),
          "best_rank": np.zeros(W, np.int32), "best_step": np.zeros(W, np.int64), "flips": np.zeros(W, np.int64),
          "state": np.zeros(W, np.int32), "since": np.zeros(W, np.int32), "pluses": np.zeros(W, np.int64)}
    status = 0
    for w in range(W):
        m = w if src is None else int(src[w])
        bad = 0
        if m < 0 or m >= M:
            bad = BAD_SRC
        elif lengths[m] < 0 or lengths[m] > K:
            bad = BAD_LENGTH
        if bad:
            status |= bad
            st["state"][w] = -1
            continue
        terms = [masks_of_row(tokens[m, t], S, shift) for t in range(int(lengths[m]))]
        terms = [t for t in terms if all(t)]
        reduce(terms)
        st["cur"][w] = st["best"][w] = to_rows(terms, K)
        st["cur_rank"][w] = st["best_rank"][w] = len(terms)
    return st, status


def draws_of_walks(seed, gs, step0, n):
    """uint32 (len(gs), n, 4): Philox-4x32-10 for steps step0 .. step0 + n - 1 of the walks with the global ids ``gs``
    (Python integers below 2^64)."""
    t = np.tile((np.arange(n, dtype=np.uint64) + np.uint64(step0)).astype(np.uint32), len(gs))
    lo = np.repeat(np.array([g & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    hi = np.repeat(np.array([(g >> 32) & 0xFFFFFFFF for g in gs], dtype=np.uint32), n)
    ctr = np.stack([lo, hi, t, np.full(len(t), DOMAIN, np.uint32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return O.philox4x32_10(ctr, np.broadcast_to(key, (len(t), 2))).reshape(len(gs), n, 4)


def flip(terms, ox, events=None):
    """Step 4 on a list with at least one match.  Returns the variant c & 3."""
    ms = matches(terms)
    c = (ox * 4 * len(ms)) >> 32
    i, j, d = ms[c >> 2]
    q, r = [x for x in range(3) if x != d]
    if c & 1:
        q, r = r, q
    a, b = (j, i) if c & 2 else (i, j)
    ta, tb = terms[a], terms[b]
    na, nb = list(ta), list(tb)
    na[q] = ta[q] ^ tb[q]
    nb[r] = tb[r] ^ ta[r]
    terms[a], terms[b] = na, nb
    nulls = sorted((p for p, t in ((a, na), (b, nb)) if not all(t)), reverse=True)    # the higher slot first
    if events is not None:
        events["null%d" % len(nulls)] += 1
    for p in nulls:
        _remove(terms, p)
    reduce(terms, events)
    return c & 3


def plus(terms, oy, oz, events=None):
    """Step 5 on a list with L >= 2.  Returns the variant v."""
    L = len(terms)
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    i, j = pairs[(oy * (L * (L - 1) // 2)) >> 32]
    v = (oz * 12) >> 32
    a, b = (j, i) if v & 1 else (i, j)
    p, q, r = PERMS[v >> 1]
    ta, tb = terms[a], terms[b]
    t1, t2, t3 = [0] * 3, [0] * 3, [0] * 3
    t1[p], t1[q], t1[r] = ta[p] ^ tb[p], ta[q], ta[r]
    t2[p], t2[q], t2[r] = tb[p], ta[q], ta[r] ^ tb[r]
    t3[p], t3[q], t3[r] = tb[p], tb[q] ^ ta[q], tb[r]
    terms[a], terms[b] = t1, t3
    terms.append(t2)
    nulls = sorted((s for s, t in ((a, t1), (b, t3), (L, t2)) if not all(t)), reverse=True)    # the highest slot first
    if events is not None:
        events["plus_null%d" % len(nulls)] += 1
    for s in nulls:
        _remove(terms, s)
    reduce(terms, events)
    return v


def advance(st, seed, walk0, step0, n_steps, plus_after=0, plus_slack=1, trace=None, on_step=None, events=None):
    """``tg_flip2_advance`` in place on the state dict.  ``trace`` (a list) receives (w, t, kind, variant) per step that
    acted, kind "flip" or "plus"; ``on_step(w, t, terms)`` sees every list after its step; ``events`` (a Counter) counts
    cancel, merge, null0..2 (null terms a flip left) and plus_null0..3."""
    W, K, _ = st["cur"].shape
    walking = [w for w in range(W) if st["state"][w] == 0 and 0 <= st["cur_rank"][w] <= K]
    if not walking:
        return st
    all_o = draws_of_walks(seed, [(walk0 + w) & (2 ** 64 - 1) for w in walking], step0, n_steps).tolist()
    for w, o in zip(walking, all_o):
        terms = from_rows(st["cur"][w], int(st["cur_rank"][w]))
        since = int(st["since"][w])
        for k in range(n_steps):
            t = step0 + k
            L = len(terms)
            C = len(matches(terms))
            cap = min(K, int(st["best_rank"][w]) + plus_slack)
            want = plus_after > 0 and (C == 0 or since >= plus_after)
            can = 2 <= L < cap
            if want and can:
                v = plus(terms, o[k][1], o[k][2], events)
                st["pluses"][w] += 1
                since = 0
                if trace is not None:
                    trace.append((w, t, "plus", v))
            elif C == 0:
                st["state"][w] = 1
                break
            else:
                v = flip(terms, o[k][0], events)
                st["flips"][w] += 1
                since = 0 if len(terms) < L else min(since + 1, INT32_MAX)
                if trace is not None:
                    trace.append((w, t, "flip", v))
            if on_step is not None:
                on_step(w, t, terms)
            if len(terms) < st["best_rank"][w]:
                st["best"][w] = to_rows(terms, K)
                st["best_rank"][w] = len(terms)
                st["best_step"][w] = t + 1
        st["cur"][w] = to_rows(terms, K)
        st["cur_rank"][w] = len(terms)
        st["since"][w] = since
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def xor_sum(terms, S):
    """uint8 (S,S,S): the tensor the list sums to over Z_2."""
    total = np.zeros((S, S, S), dtype=np.uint8)
    for m0, m1, m2 in terms:
        u, v, w = (np.array([(m >> e) & 1 for e in range(S)], dtype=np.uint8) for m in (m0, m1, m2))
        total ^= u[:, None, None] & v[None, :, None] & w[None, None, :]
    return total


def residual(targets, lists, ranks):
    """int32 (M,) of ``tg_flip2_residual``."""
    targets = np.asarray(targets)
    M, S = targets.shape[0], targets.shape[1]
    K = lists.shape[1]
    out = np.zeros(M, dtype=np.int32)
    for m in range(M):
        if ranks[m] < 0 or ranks[m] > K:
            out[m] = -1
        else:
            out[m] = int(((targets[m].astype(np.int64) & 1) != xor_sum(from_rows(lists[m], int(ranks[m])), S)).sum())
    return out


def target_of(tokens, L, S, shift):
    """int8 (S,S,S): the integer sum of a token list (``flips.term_sum`` on the host); its parity is the Z_2 target."""
    f = np.asarray(tokens[:L], dtype=np.int64) - shift
    return np.einsum("ti,tj,tl->ijl", f[:, :S], f[:, S:2 * S], f[:, 2 * S:]).astype(np.int8)
