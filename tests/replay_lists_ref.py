"""Host restatement of tg_replay_add_lists (not a test module), written from the text of
include/tensor_game_replay_lists.h: the 32-bit replay of a move list, its four validity conditions, the stored game
(frames by the head_{t-f} / starts[g][f-t] rule, the list's tokens, rewards -(t+1)) and the two select rules, on the ring
of replay_ref.  tests/test_replay_lists_cpu.py checks it against tests/golden/replay_lists_cases.npz (recorded from the
reference itself) and against replay_ref's tg_replay_add on the padded form; tests/test_gpu_replay_lists.py checks the
device against it.  ``composed_add`` is the device-side path a user had before the entry (env steps, stacked frames, a
one-hot policy, ops.replay_add): the GPU test and tools/replay_lists_bench.py compare the entry with it."""
import numpy as np

BAD_LENGTH, BAD_GROUP, BAD_RANGE, NOT_ZERO = 1, 4, 8, 16


def heads_of(start0, tokens, L, shift):
    """head_0 .. head_L (int32 (L+1,S,S,S), wrapping as 32-bit integers do): head_{t+1} = head_t - u (x) v (x) w."""
    S = start0.shape[0]
    heads = [np.asarray(start0, np.int32)]
    for t in range(L):
        u, v, w = (np.asarray(tokens[t], np.int32) - np.int32(shift)).reshape(3, S)
        with np.errstate(over="ignore"):
            heads.append(heads[-1] - u[:, None, None] * v[None, :, None] * w[None, None, :])
    return np.stack(heads)


def list_flags(starts, tokens_m, L, g, K, ring_L, shift):
    """(status bits of one list, its heads or None): the length and the group first, each on its own; only a list that
    passes both is replayed."""
    flags = 0
    if not 1 <= L <= min(K, ring_L):
        flags |= BAD_LENGTH
    if not 0 <= g < len(starts):
        flags |= BAD_GROUP
    if flags:
        return flags, None
    heads = heads_of(starts[g][0], tokens_m, L, shift)
    if (heads[1:] < -128).any() or (heads[1:] > 127).any():
        flags |= BAD_RANGE
    if heads[L].any():
        flags |= NOT_ZERO
    return flags, heads


def game_of(start, heads, tokens_m, L):
    """The stored game of a valid list: (frames int8 (L,T,S,S,S), tokens int8 (L,3S), rewards f32 (L,))."""
    T = start.shape[0]
    frames = np.zeros((L,) + start.shape, np.int8)
    for t in range(L):
        for f in range(T):
            frames[t, f] = heads[t - f] if f <= t else start[f - t]
    return frames, np.asarray(tokens_m[:L], np.int8).copy(), -np.arange(1, L + 1, dtype=np.float32)


def add_lists(ring, starts, tokens, lengths, groups=None, shift=1, select=False):
    """One tg_replay_add_lists call on a replay_ref.Ring: returns (stored uint8 (M,), the status bits)."""
    starts, tokens = np.asarray(starts, np.int8), np.asarray(tokens, np.int8)
    M, K = tokens.shape[0], tokens.shape[1]
    stored, status, games = np.zeros(M, np.uint8), 0, {}
    for m in range(M):
        L, g = int(lengths[m]), int(m if groups is None else groups[m])
        flags, heads = list_flags(starts, tokens[m], L, g, K, ring.L, shift)
        status |= flags
        if flags == 0:
            games[m] = game_of(starts[g], heads, tokens[m], L)
    if select:
        if games:
            least = min(len(v[2]) for v in games.values())
            games = dict([next((m, v) for m, v in games.items() if len(v[2]) == least)])  # dicts keep list order
    for m, game in games.items():
        ring.slots[ring.pointer] = game
        ring.pointer = (ring.pointer + 1) % ring.C
        ring.added += 1
        stored[m] = 1
    return stored, status


def padded_form(starts, tokens, lengths, groups, ring_L, shift, n_logits):
    """What tg_replay_add takes for the same lists, built the way a user had to before: a state stepped move by move
    with the history shifted down by hand (get_child_states), a one-hot float policy, the reference's reward rule for
    an end state of rank 0.  Lists must be valid.  (states (M,L,T,S,S,S) int8, policy f32, rewards f32, lengths)."""
    starts, tokens = np.asarray(starts, np.int8), np.asarray(tokens, np.int8)
    M, A3 = tokens.shape[0], tokens.shape[2]
    S = A3 // 3
    states = np.zeros((M, ring_L) + starts.shape[1:], np.int8)
    policy = np.zeros((M, ring_L, A3, n_logits), np.float32)
    rewards = np.zeros((M, ring_L), np.float32)
    for m in range(M):
        n = int(lengths[m])
        state = starts[int(m if groups is None else groups[m])].astype(np.int32)
        for t in range(n):
            states[m, t] = state
            u, v, w = (tokens[m, t].astype(np.int32) - shift).reshape(3, S)
            head = state[0] - np.einsum("i,j,k->ijk", u, v, w)
            state = np.concatenate([head[None], state[:-1]])
        policy[m, :n] = np.eye(n_logits, dtype=np.float32)[tokens[m, :n]]
        rewards[m, :n] = np.cumsum(np.full(n, -1.0, np.float32))
    return states, policy, rewards, np.asarray(lengths, np.int64)


def composed_add(buf, starts, tokens, lengths, groups=None, shift=1, select=False, n_logits=None):
    """The same lists into a ``GameBuffer`` by the composed path, on the device: K ``TensorGameEnv.step`` calls, the frames
    stacked with the history shift, a one-hot float policy and ``ops.replay_add``.  Lists must be valid and at most
    ``buf.L`` moves long (K <= buf.L).  Returns the tensors handed to ``ops.replay_add``."""
    import torch

    from mat_mul_amd import TensorGameEnv, ops

    M, K, A3 = tokens.shape
    S, T, dev = A3 // 3, starts.shape[1], tokens.device
    begin = starts if groups is None else starts[groups]
    env = TensorGameEnv(M, S, device=dev, shift=shift, track_nnz=False)
    env.reset(begin[:M, 0].contiguous())
    line = [begin[:M, f] for f in range(T - 1, 0, -1)]  # oldest first: the history, then head_0, head_1, ...
    for t in range(K):
        line.append(env.state.clone())
        env.step(tokens[:, t].contiguous())
    windows = torch.stack(line, 1).unfold(1, T, 1)       # (M,K,S,S,S,T): move t sees line[t : t + T], oldest first
    states = torch.zeros((M, buf.L, T, S, S, S), dtype=torch.int8, device=dev)
    states[:, :K] = windows.permute(0, 1, 5, 2, 3, 4).flip(2)
    n_logits = int(n_logits or 3 + shift)
    policy = torch.zeros((M, buf.L, A3, n_logits), dtype=torch.float32, device=dev)
    policy[:, :K] = torch.nn.functional.one_hot(tokens.to(torch.int64), n_logits).to(torch.float32)
    rewards = torch.zeros((M, buf.L), dtype=torch.float32, device=dev)
    rewards[:, :K] = -torch.arange(1, K + 1, device=dev, dtype=torch.float32)
    ops.replay_add(buf, states, policy, rewards, lengths, select=select, status=buf.status)
    return states, policy, rewards
