"""Host restatement of include/tensor_game_symmetry.h, straight from its formulas (numpy): the group action on frames
and tokens, the inverse element, the env step it commutes with, and the sampler's rule on the oracle's Philox."""
import numpy as np

from oracle.tensor_game import philox4x32_10

RHO = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # code -> (rho[0], rho[1], rho[2])
MODES, PERMS, SIGNS = 1, 2, 4
STREAM = 0x53000000


def decode(row, S):
    """(rho, pi (3,S), sign (3,S) of +-1) of one uint8 row, or None for a bad row."""
    row = np.asarray(row, np.uint8)
    idx = (row[1:] & 0x7F).astype(np.int64).reshape(3, S)
    if row[0] > 5 or (idx >= S).any():
        return None
    sign = np.where(row[1:] & 0x80, -1, 1).astype(np.int64).reshape(3, S)
    return RHO[int(row[0])], idx, sign


def encode(rho, pi, sign):
    pi, sign = np.asarray(pi), np.asarray(sign)
    return np.concatenate([[RHO.index(tuple(rho))], (pi | np.where(sign < 0, 0x80, 0)).reshape(-1)]).astype(np.uint8)


def identity(N, S):
    return np.tile(encode((0, 1, 2), np.tile(np.arange(S), (3, 1)), np.ones((3, S), np.int64)), (N, 1))


def apply(frames, tokens, sym, shift=1):
    """frames int8 (N,T,S,S,S) (or (N,S,S,S): one frame), tokens int8 (N,3S) or None, sym uint8 (N,3S+1) ->
    (frames, tokens, overflow uint8 (N,), status): values wrapped to int8, overflow where one left it, a bad row all zero
    with bit 0 of status."""
    frames = np.asarray(frames, np.int8)
    single = frames.ndim == 4
    if single:
        frames = frames[:, None]
    N, T, S = frames.shape[:3]
    out = np.zeros(frames.shape, np.int64)
    tok = None if tokens is None else np.zeros((N, 3 * S), np.int64)
    status = 0
    for n in range(N):
        g = decode(sym[n], S)
        if g is None:
            status |= 1
            continue
        rho, pi, sign = g
        ix = [None] * 3
        for m in range(3):  # b_{rho[m]} = pi_m[a_m]: along output axis m
            shape = [1, 1, 1]
            shape[m] = S
            ix[rho[m]] = pi[m].reshape(shape)
        s3 = sign[0][:, None, None] * sign[1][None, :, None] * sign[2][None, None, :]
        for f in range(T):
            out[n, f] = s3 * frames[n, f].astype(np.int64)[ix[0], ix[1], ix[2]]
        if tok is not None:
            t = np.asarray(tokens[n], np.int64)
            for m in range(3):
                tok[n, m * S:(m + 1) * S] = sign[m] * (t[rho[m] * S + pi[m]] - shift) + shift
    over = (np.abs(out.reshape(N, -1) + 0.5) > 128).any(1)
    if tok is not None:
        over |= (np.abs(tok + 0.5) > 128).any(1)
        tok = tok.astype(np.int8)
    out = out.astype(np.int8)
    return (out[:, 0] if single else out), tok, over.astype(np.uint8), status


def inverse(sym, S):
    """The rows of the inverse elements: x = apply(apply(x, g), inverse(g))."""
    out = []
    for row in sym:
        rho, pi, sign = decode(row, S)
        irho, ipi, isign = [0] * 3, np.zeros((3, S), np.int64), np.zeros((3, S), np.int64)
        for m in range(3):
            k = rho[m]
            irho[k] = m
            ipi[k][pi[m]] = np.arange(S)   # pi'_k = pi_m^-1
            isign[k][pi[m]] = sign[m]      # s'_k[b] = s_m[pi_m^-1[b]]
        out.append(encode(irho, ipi, isign))
    return np.stack(out)


def step(state, tokens, shift=1):
    """state (N,S,S,S) - u (x) v (x) w in int64 (no narrowing), done (N,)."""
    state = np.asarray(state, np.int64)
    S = state.shape[1]
    f = np.asarray(tokens, np.int64) - shift
    u, v, w = f[:, :S], f[:, S:2 * S], f[:, 2 * S:]
    out = state - u[:, :, None, None] * v[:, None, :, None] * w[:, None, None, :]
    return out, ~out.reshape(len(out), -1).any(1)


def words(N, S, seed, item_offset=0):
    """uint64 (N, 4*ceil((3S+1)/4)): the stream w[...] of the ids item_offset .. item_offset+N-1."""
    nblk = (3 * S + 1 + 3) // 4
    ids = (np.arange(N, dtype=np.uint64) + np.uint64(item_offset & (2 ** 64 - 1)))
    ctr = np.zeros((N, nblk, 4), np.uint32)
    ctr[..., 0] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[..., 1] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[..., 2] = np.arange(nblk, dtype=np.uint32)[None]
    ctr[..., 3] = STREAM
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    return philox4x32_10(ctr, np.broadcast_to(key, (N, nblk, 2))).reshape(N, nblk * 4).astype(np.uint64)


def sample(N, S, seed, item_offset=0, flags=MODES | PERMS | SIGNS):
    """uint8 (N,3S+1): the header's rule."""
    w = words(N, S, seed, item_offset)
    rows = np.zeros((N, 3 * S + 1), np.uint8)
    code = (w[:, 0] * np.uint64(6)) >> np.uint64(32)
    rows[:, 0] = code if flags & MODES else 0
    r = np.arange(N)
    for m in range(3):
        pi = np.tile(np.arange(S, dtype=np.int64), (N, 1))
        for a in range(S - 1, 0, -1):
            j = ((w[:, 1 + m * S + (S - 1 - a)] * np.uint64(a + 1)) >> np.uint64(32)).astype(np.int64)
            pa, pj = pi[r, a].copy(), pi[r, j].copy()
            pi[r, a], pi[r, j] = pj, pa
        if not flags & PERMS:
            pi = np.tile(np.arange(S, dtype=np.int64), (N, 1))
        sw = w[:, 1 + m * S + (S - 1)]
        neg = ((sw[:, None] >> np.arange(S, dtype=np.uint64)[None]) & np.uint64(1)).astype(np.int64)
        if not flags & SIGNS:
            neg[:] = 0
        rows[:, 1 + m * S:1 + (m + 1) * S] = pi | (neg << 7)
    return rows
