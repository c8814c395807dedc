"""Host restatement of include/tensor_game_solutions.h, straight from its text (numpy and Python integers): the exact
verification, the canonical form, the key and the bad rows of ``tg_solution_canon``; ``Archive``, the add rule of
``mat_mul_amd.SolutionArchive``; and the seeded action lists both test files use.  Nothing here calls the library."""
import numpy as np

MASK = (1 << 64) - 1
BAD_LENGTH, BAD_NEGATION = 1, 2


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & MASK
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & MASK
    k ^= k >> 33
    return k


def stream_key(data: bytes) -> int:
    """tg_hash_u64's rule over a byte stream of n bytes, with n in place of S^3."""
    n = len(data)
    data = data + b"\0" * (-n % 8)
    total = 0
    for k in range(len(data) // 8):
        w = int.from_bytes(data[8 * k:8 * k + 8], "little")
        total = (total + fmix64((w + (k + 1) * 0x9E3779B97F4A7C15) & MASK)) & MASK
    return fmix64(total ^ ((n * 0xC2B2AE3D27D4EB4F) & MASK))


def term_sum(tokens, length, S, shift):
    """sum_{t < length} u (x) v (x) w of one list, in int64."""
    f = np.asarray(tokens[:length], dtype=np.int64) - shift
    return np.einsum("ti,tj,tl->ijl", f[:, :S], f[:, S:2 * S], f[:, 2 * S:])


def _fits(vec, shift):
    tok = vec + shift
    return bool((tok >= -128).all() and (tok <= 127).all())


def canon_row(target, tokens, length, S, shift):
    """(canon (K,3S) int8, rank, key, residual_nnz or None, status bits) of one list."""
    K = tokens.shape[0]
    zero = np.zeros((K, 3 * S), dtype=np.int8)
    bad_res = None if target is None else -1
    if length < 0 or length > K:
        return zero, 0, 0, bad_res, BAD_LENGTH
    res = None
    if target is not None:
        res = int(np.count_nonzero(np.asarray(target, dtype=np.int64) - term_sum(tokens, length, S, shift)))
    f = np.asarray(tokens[:length], dtype=np.int64) - shift
    terms = []
    for t in range(length):
        vecs = [f[t, :S], f[t, S:2 * S], f[t, 2 * S:]]
        if not all(v.any() for v in vecs):
            continue                                         # 1. a null term
        sigma, norm = 1, []
        for v in vecs:                                       # 2. first non-zero positive
            if v[np.flatnonzero(v)[0]] < 0:
                v, sigma = -v, -sigma
                if not _fits(v, shift):
                    return zero, 0, 0, bad_res, BAD_NEGATION
            norm.append(v)
        terms.append((tuple(int(x) for x in np.concatenate(norm)), sigma))
    terms.sort(key=lambda ts: ts[0])                         # 3. lexicographic, signed
    kept, i = [], 0
    while i < len(terms):                                    # 4. merge the runs
        j, c = i, 0
        while j < len(terms) and terms[j][0] == terms[i][0]:
            c += terms[j][1]
            j += 1
        row = np.array(terms[i][0], dtype=np.int64)
        if c < 0:
            row[2 * S:] = -row[2 * S:]
            if not _fits(row[2 * S:], shift):
                return zero, 0, 0, bad_res, BAD_NEGATION
        kept += [row] * abs(c)
        i = j
    rank = len(kept)                                         # 5.
    out = zero.copy()
    if rank:
        out[:rank] = (np.stack(kept) + shift).astype(np.int8)  # 6.
    return out, rank, stream_key(out[:rank].tobytes()), res, 0


def canon(targets, tokens, lengths, shift):
    """(canon int8 (M,K,3S), rank int32 (M), key uint64 (M), residual_nnz int32 (M) or None, status)."""
    tokens = np.asarray(tokens, dtype=np.int8)
    M, K, A3 = tokens.shape
    S = A3 // 3
    out = np.zeros((M, K, A3), dtype=np.int8)
    rank = np.zeros(M, dtype=np.int32)
    key = np.zeros(M, dtype=np.uint64)
    res = None if targets is None else np.zeros(M, dtype=np.int32)
    status = 0
    for m in range(M):
        out[m], rank[m], k, r, bits = canon_row(None if targets is None else targets[m], tokens[m], int(lengths[m]), S,
                                                shift)
        key[m] = np.uint64(k)
        if res is not None:
            res[m] = r
        status |= bits
    return out, rank, key, res, status


def state_key(state) -> int:
    """tg_hash_u64 of one (S,S,S) int8 state."""
    return stream_key(np.ascontiguousarray(state, dtype=np.int8).tobytes())


class Archive:
    """The add rule of ``SolutionArchive`` on the host: verify and canonicalise; a row is valid when its residual is
    zero and its rank is at most ``max_rank``; among valid rows with equal key only the lowest batch index counts; of
    those, the ones whose key was never offered before are new, and the new rows are appended in batch order while
    there is room (a row without room sets bit 0 of ``status``; its key still counts as offered)."""

    def __init__(self, S, max_rank, capacity, shift=1):
        self.S, self.max_rank, self.capacity, self.shift = S, max_rank, capacity, shift
        self.tokens, self.rank, self.key, self.target_key = [], [], [], []
        self.offered = set()
        self.status = 0

    @property
    def count(self):
        return len(self.key)

    @property
    def lowest_rank(self):
        return min(self.rank) if self.rank else self.max_rank + 1

    def add(self, targets, tokens, lengths):
        """(proven bool (M), rank, key, fresh bool (M): the rows stored by this call)."""
        cn, rank, key, res, _ = canon(targets, tokens, lengths, self.shift)
        M = len(rank)
        proven = res == 0
        fresh = np.zeros(M, dtype=bool)
        in_batch = set()
        for m in range(M):
            k = int(key[m])
            if not proven[m] or rank[m] > self.max_rank or k in in_batch:
                continue
            in_batch.add(k)
            if k in self.offered:
                continue
            self.offered.add(k)
            if self.count >= self.capacity:
                self.status |= 1
                continue
            fresh[m] = True
            row = np.zeros((self.max_rank, 3 * self.S), dtype=np.int8)
            n = min(self.max_rank, cn.shape[1])
            row[:n] = cn[m, :n]
            self.tokens.append(row)
            self.rank.append(int(rank[m]))
            self.key.append(k)
            self.target_key.append(state_key(targets[m]))
        return proven, rank, key, fresh

    def state_dict(self):
        return dict(S=self.S, max_rank=self.max_rank, capacity=self.capacity, shift=self.shift, status=self.status,
                    tokens=[t.copy() for t in self.tokens], rank=list(self.rank), key=list(self.key),
                    target_key=list(self.target_key))

    @classmethod
    def from_state_dict(cls, sd):
        a = cls(sd["S"], sd["max_rank"], sd["capacity"], sd["shift"])
        a.tokens, a.rank, a.key, a.target_key = ([t.copy() for t in sd["tokens"]], list(sd["rank"]), list(sd["key"]),
                                                 list(sd["target_key"]))
        a.offered = set(a.key)   # the stored keys only: a row that found no room is offered again, and finds none again
        a.status = sd["status"]
        return a


# ---- seeded action lists ---------------------------------------------------------------------------------------------
VALUES, PROBS = (-2, -1, 0, 1, 2), (0.05, 0.2, 0.5, 0.2, 0.05)


def _negate(f, S, which):
    f = f.copy()
    for x in which:
        f[x * S:(x + 1) * S] = -f[x * S:(x + 1) * S]
    return f


def random_lists(rng, M, K, S, shift, lengths=None):
    """(tokens int8 (M,K,3S), lengths int64 (M)): factor values from VALUES; lengths (unless given) from 0 to K, both
    ends present when M >= 2; about half of the terms planted from an earlier term of their list: a duplicate, a negated duplicate (one
    factor negated), a sign variant (two factors negated: the same term), or a null term (one factor zeroed).  The rows
    beyond a list's length hold arbitrary tokens, which nothing may read."""
    tokens = rng.integers(-128, 128, size=(M, K, 3 * S)).astype(np.int8)
    if lengths is None:
        lengths = rng.integers(0, K + 1, size=M)
        if M >= 2:
            lengths[0], lengths[-1] = 0, K
    lengths = np.asarray(lengths, dtype=np.int64)
    for m in range(M):
        L = int(lengths[m])
        f = rng.choice(VALUES, size=(L, 3 * S), p=PROBS).astype(np.int64)
        for t in range(1, L):
            r, src = rng.random(), f[rng.integers(t)]
            if r < 0.15:
                f[t] = src
            elif r < 0.30:
                f[t] = _negate(src, S, [rng.integers(3)])
            elif r < 0.40:
                f[t] = _negate(src, S, list(rng.choice(3, size=2, replace=False)))
            elif r < 0.50:
                x = rng.integers(3)
                f[t, x * S:(x + 1) * S] = 0
        tokens[m, :L] = (f + shift).astype(np.int8)
    return tokens, lengths


def targets_for(rng, tokens, lengths, S, shift):
    """int8 (M,S,S,S): row m is, by m mod 3, the exact sum of its list (clipped to int8, which small values never
    need), the sum with ONE entry changed, or random."""
    M = tokens.shape[0]
    out = np.zeros((M, S, S, S), dtype=np.int8)
    for m in range(M):
        total = np.clip(term_sum(tokens[m], int(lengths[m]), S, shift), -128, 127)
        if m % 3 == 1:
            i = tuple(rng.integers(S, size=3))
            total[i] += 1 if total[i] < 127 else -1
        elif m % 3 == 2:
            total = rng.integers(-2, 3, size=(S, S, S))
        out[m] = total.astype(np.int8)
    return out


def variant(rng, tokens, length, K, S, shift, pairs=1, nulls=1):
    """The same factorisation written differently, as (tokens (K,3S), length): the terms permuted, two factors negated
    in random terms, and ``pairs`` random terms inserted together with their negatives and ``nulls`` null terms, at
    random places.  Needs length + 2*pairs + nulls <= K."""
    f = np.asarray(tokens[:length], dtype=np.int64) - shift
    f = f[rng.permutation(length)] if length else f
    rows = []
    for t in range(length):
        row = f[t]
        if rng.random() < 0.5:
            row = _negate(row, S, list(rng.choice(3, size=2, replace=False)))
        rows.append(row)
    for _ in range(pairs):
        extra = rng.choice((-1, 1), size=3 * S) * rng.integers(0, 2, size=3 * S)
        for x in range(3):                                   # not a null term: it has to cancel, not to be dropped
            if not extra[x * S:(x + 1) * S].any():
                extra[x * S + rng.integers(S)] = 1
        for row in (extra, _negate(extra, S, [rng.integers(3)])):
            rows.insert(rng.integers(len(rows) + 1), row)
    for _ in range(nulls):
        null = rng.choice((-1, 0, 1), size=3 * S)
        x = rng.integers(3)
        null[x * S:(x + 1) * S] = 0
        rows.insert(rng.integers(len(rows) + 1), null)
    assert len(rows) <= K
    out = np.zeros((K, 3 * S), dtype=np.int8)
    if rows:
        out[:len(rows)] = (np.stack(rows) + shift).astype(np.int8)
    return out, len(rows)
