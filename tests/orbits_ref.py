"""Host restatement of include/tensor_game_orbits.h, straight from its text (numpy and Python integers), on top of
``solutions_ref.canon_row`` (the canonical form of one list) and ``symmetry_ref`` (the encoding of a group element):
the action of an element on a list, the smallest canonical form over a set with ``which`` and ``stab``, the three bad
bits, and ``fixes``.  Nothing here calls the library."""
import numpy as np

import solutions_ref as SR
import symmetry_ref as SY

BAD_LENGTH, BAD_NEGATION, BAD_GROUP = 1, 2, 4


def act(tokens, length, g, S, shift):
    """g.X as VALUES int64 (length,3S), not narrowed: f^g[m*S + a] = s_m[a] * f[rho[m]*S + pi_m[a]]."""
    rho, pi, sign = g
    f = np.asarray(tokens[:length], dtype=np.int64) - shift
    out = np.empty_like(f)
    for m in range(3):
        out[:, m * S:(m + 1) * S] = sign[m][None] * f[:, rho[m] * S + pi[m]]
    return out


def act_tokens(tokens, length, g, S, shift):
    """g.X as an int8 token list (K,3S) like ``tokens`` (the values must fit), rows beyond ``length`` zero."""
    out = np.zeros_like(np.asarray(tokens, dtype=np.int8))
    vals = act(tokens, length, g, S, shift) + shift
    assert (vals >= -128).all() and (vals <= 127).all()
    out[:length] = vals.astype(np.int8)
    return out


def form_of(values, K, S, shift):
    """(canon (K,3S) int8, rank, bits) of a list of VALUES: steps 1-5 of tensor_game_solutions.h; bit 1 when a normalised
    value of a term that step 1 keeps, or a negated w that is kept, has its token outside int8."""
    length = values.shape[0]
    for t in range(length):
        vecs = [values[t, x * S:(x + 1) * S] for x in range(3)]
        if not all(v.any() for v in vecs):
            continue
        for v in vecs:
            norm = -v if v[np.flatnonzero(v)[0]] < 0 else v
            if (norm + shift < -128).any() or (norm + shift > 127).any():
                return None, 0, BAD_NEGATION
    wide = np.zeros((K, 3 * S), dtype=np.int64)   # as "tokens" of 64 bits: canon_row only ever subtracts the shift again
    wide[:length] = values + shift
    cn, rank, _, _, bits = SR.canon_row(None, wide, length, S, shift)
    return (None, 0, bits) if bits else (cn, rank, 0)


def order_key(cn):
    """A row's place in the order: its bytes as signed tokens, lexicographically."""
    return (cn.reshape(-1).view(np.uint8) ^ 0x80).tobytes()


def orbit_row(target, tokens, length, S, shift, elems, want_forms=False):
    """(canon, rank, key, residual_nnz or None, which, stab, bits) of one list over the good elements ``elems`` (None
    entries are bad rows and are skipped); with ``want_forms`` also the list of every (order key, rank) over g."""
    K = tokens.shape[0]
    zero = np.zeros((K, 3 * S), dtype=np.int8)
    bad_res = None if target is None else -1
    if length < 0 or length > K:
        return (zero, 0, 0, bad_res, -1, 0, BAD_LENGTH) + (([],) if want_forms else ())
    res = SR.canon_row(target, tokens, length, S, shift)[3]
    best, which, stab, forms = None, -1, 0, []
    for gi, g in enumerate(elems):
        if g is None:
            continue
        cn, rank, bits = form_of(act(tokens, length, g, S, shift), K, S, shift)
        if bits:
            return (zero, 0, 0, bad_res, -1, 0, BAD_NEGATION) + (([],) if want_forms else ())
        k = order_key(cn)
        forms.append((k, rank))
        if best is None or k < best[0]:
            best, which, stab = (k, cn, rank), gi, 1
        elif k == best[0]:
            stab += 1
    if best is None:                                            # every row of the set is bad
        return (zero, 0, 0, bad_res, -1, 0, 0) + (([],) if want_forms else ())
    _, cn, rank = best
    out = (cn, rank, SR.stream_key(cn[:rank].tobytes()), res, which, stab, 0)
    return out + ((forms,) if want_forms else ())


def orbit_canon(targets, tokens, lengths, shift, sym):
    """(canon int8 (M,K,3S), rank int32, key uint64, residual_nnz int32 or None, which int32, stab int32, status)."""
    tokens = np.asarray(tokens, dtype=np.int8)
    M, K, A3 = tokens.shape
    S = A3 // 3
    elems = [SY.decode(row, S) for row in np.asarray(sym, np.uint8)]
    group_bad = any(g is None for g in elems)
    out = np.zeros((M, K, A3), dtype=np.int8)
    rank, which, stab = (np.zeros(M, dtype=np.int32) for _ in range(3))
    key = np.zeros(M, dtype=np.uint64)
    res = None if targets is None else np.zeros(M, dtype=np.int32)
    status = BAD_GROUP if group_bad else 0
    for m in range(M):
        cn, r, k, n, w, s, bits = orbit_row(None if targets is None else targets[m], tokens[m], int(lengths[m]), S, shift,
                                            elems)
        status |= bits
        if group_bad and not bits:                              # every list is bad
            cn, r, k, n, w, s = np.zeros((K, A3), np.int8), 0, 0, (None if targets is None else -1), -1, 0
        out[m], rank[m], key[m], which[m], stab[m] = cn, r, np.uint64(k), w, s
        if res is not None:
            res[m] = n
    return out, rank, key, res, which, stab, status


def fixes(targets, sym):
    """(uint8 (M,), status): 1 where every row fixes the target, compared in int64; a bad row: all 0, status bit 0."""
    targets = np.asarray(targets, np.int64)
    M, S = targets.shape[:2]
    out = np.ones(M, dtype=np.uint8)
    for row in np.asarray(sym, np.uint8):
        g = SY.decode(row, S)
        if g is None:
            return np.zeros(M, dtype=np.uint8), 1
        rho, pi, sign = g
        ix = [None] * 3
        for m in range(3):
            shape = [1, 1, 1]
            shape[m] = S
            ix[rho[m]] = pi[m].reshape(shape)
        s3 = sign[0][:, None, None] * sign[1][None, :, None] * sign[2][None, None, :]
        for n in range(M):
            if not np.array_equal(s3 * targets[n][ix[0], ix[1], ix[2]], targets[n]):
                out[n] = 0
    return out, 0


def proven_lists(rng, M, K, S, shift, max_terms):
    """(targets int8 (M,S,S,S), tokens, lengths): random lists with their exact sums as targets."""
    lengths = rng.integers(1, max_terms + 1, size=M)
    tokens, lengths = SR.random_lists(rng, M, K, S, shift, lengths)
    targets = np.stack([SR.term_sum(tokens[m], int(lengths[m]), S, shift) for m in range(M)])
    assert np.abs(targets).max() <= 127
    return targets.astype(np.int8), tokens, lengths
