"""Host restatement of include/tensor_game_flips.h, straight from its text (numpy and Python integers, the oracle's
Philox): ``begin`` and ``advance`` with a full-scan reduce and a full match enumeration, no shortcuts; the standard
matmul lists and the planted lists both test files use.  Nothing here calls the library.

A walk's list is held as the header names it: per term the normalised vectors n_0, n_1, n_2 and the sign s, so that
the term is s * n_0 (x) n_1 (x) n_2 and its stored form is (n_0, n_1, s * n_2)."""
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


def _remove(terms, p):
    """Removing slot p moves the last live term into p and decrements L."""
    last = terms.pop()
    if p < len(terms):
        terms[p] = last


def reduce(terms, bound):
    """The full scan: pairs i < j in ascending (i, j) order; after a merge the scan restarts."""
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
                if any(abs(x) > bound for x in z):
                    continue                       # skipped: z stays what it is while neither term changes
                if not any(z):
                    _remove(terms, j)
                    _remove(terms, i)
                else:
                    n, sg = _norm(z)
                    new = list(ti)
                    new[d], new[3] = n, sg
                    terms[i] = new
                    _remove(terms, j)
                merged = True
                break
            if merged:
                break
        if not merged:
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
    t = (np.arange(n, dtype=np.uint64) + np.uint64(step0)).astype(np.uint32)
    ctr = np.stack([np.full(n, g & 0xFFFFFFFF, np.uint32), np.full(n, (g >> 32) & 0xFFFFFFFF, np.uint32), t,
                    np.full(n, DOMAIN, np.uint32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return [int(x) for x in O.philox4x32_10(ctr, np.broadcast_to(key, (n, 2)))[:, 0]]


def step(terms, ox, bound):
    """One step on a walking list.  Returns None when there is no match (stuck), else (variant, accepted)."""
    ms = matches(terms)
    C = len(ms)
    if C == 0:
        return None
    c = (ox * 8 * C) >> 32
    i, j, m = ms[c >> 3]
    variant = c & 7
    eps = -1 if variant & 1 else 1
    q, r = [x for x in range(3) if x != m]
    if variant & 2:
        q, r = r, q
    a, b = (j, i) if variant & 4 else (i, j)
    ta, tb = terms[a], terms[b]
    new_q = tuple(x + eps * y for x, y in zip(ta[q], tb[q]))
    new_r = tuple(tb[3] * y - eps * ta[3] * x for x, y in zip(ta[r], tb[r]))
    if any(abs(x) > bound for x in new_q + new_r):
        return variant, False
    raw_a, raw_b = [None] * 3, [None] * 3
    raw_a[m], raw_a[q], raw_a[r] = ta[m], new_q, tuple(ta[3] * x for x in ta[r])
    raw_b[m], raw_b[q], raw_b[r] = tb[m], tb[q], new_r
    na, nb = term_from_raw(raw_a), term_from_raw(raw_b)
    if na is not None:
        terms[a] = na
    if nb is not None:
        terms[b] = nb
    for p in sorted((p for p, t in ((a, na), (b, nb)) if t is None), reverse=True):   # the higher slot first
        _remove(terms, p)
    reduce(terms, bound)
    return variant, True


def advance(st, seed, walk0, step0, n_steps, bound, shift, trace=None, on_step=None):
    """``tg_flip_advance`` in place on the state dict.  ``trace`` (a list) receives (w, t, variant, accepted) per step
    that drew; ``on_step(w, t, terms)`` sees every list after its step."""
    W, K, A3 = st["cur"].shape
    S = A3 // 3
    for w in range(W):
        if st["state"][w] != 0:
            continue
        g = walk0 + w
        terms = from_rows(st["cur"][w], int(st["cur_rank"][w]), S, shift)
        ox = draws(seed, g, step0, n_steps)
        for k in range(n_steps):
            t = step0 + k
            res = step(terms, ox[k], bound)
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


def pool_list(rng, S, K, L, pool, shift):
    """L random terms whose factors come from a pool of ``pool`` vectors per mode with values in {-1, 0, 1}, so that
    matches are plentiful."""
    vecs = rng.integers(-1, 2, size=(3, pool, S))
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
