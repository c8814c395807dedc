"""Oracle of tg_demo_items / ops.demo_items (not a test module): oracle.tensor_game.demo_getitem -- the arithmetic of
the reference's SyntheticDemoDataset.__getitem__ (datasets.py:78-122) -- batched over flat item indices, with the frames
narrowed to int8 and the per-item overflow flag of _narrow_i8."""
import numpy as np

from oracle import tensor_game as O


def ref_items(tokens, targets, idx, T, shift=1):
    """tokens int8 (n_demos,R,3S), targets int8 (n_demos,S,S,S), idx (N,) flat indices.  Returns (frames int8
    (N,T,S,S,S), scalars f32 (N,1), actions int8 (N,3S), rewards f32 (N,1), overflow uint8 (N,), status uint32 (1,)):
    an index outside [0, n_demos*R) gives an all-zero item and sets bit 0 of status."""
    tokens, targets = np.asarray(tokens), np.asarray(targets)
    n_demos, R, A3 = tokens.shape
    S = A3 // 3
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    N = idx.shape[0]
    frames = np.zeros((N, T, S, S, S), np.int8)
    scalars = np.zeros((N, 1), np.float32)
    actions = np.zeros((N, A3), np.int8)
    rewards = np.zeros((N, 1), np.float32)
    overflow = np.zeros((N,), np.uint8)
    status = np.zeros((1,), np.uint32)
    for n, x in enumerate(idx.tolist()):
        if not 0 <= x < n_demos * R:
            status[0] |= 1
            continue
        d, k = divmod(x, R)
        f64, sc, a, rw = O.demo_getitem(list(tokens[d].astype(np.int64)), targets[d], k, T, shift)
        f8, ovf = O._narrow_i8(f64[None])
        frames[n], overflow[n] = f8[0], ovf[0]
        scalars[n, 0], actions[n], rewards[n, 0] = sc, a, rw
    return frames, scalars, actions, rewards, overflow, status
