"""Host restatement of the replay buffers and the mixed dataset (not a test module): the ring of PlayedGamesDataset
(datasets.py:161-230) with the argmax tokens it trains on, act_step's best-game rule (training.py:468-483) and the
routing of TensorGameDataset.__getitem__ (datasets.py:286-303), in numpy.  Synthetic items come from
demo_items_ref.ref_items.  tests/test_replay_cpu.py checks it against tests/golden/replay_cases.npz (recorded from the
reference itself); tests/test_gpu_replay.py checks the device against it."""
import numpy as np

from demo_items_ref import ref_items

SYNTH, PLAYED, BEST, BAD = 0, 1, 2, 3


def argmax_tokens(policy):
    """torch's argmax over the last axis: the first maximal index, the first NaN when there is one."""
    p = np.asarray(policy, np.float32)
    nan = np.isnan(p)
    first_nan = np.argmax(nan, axis=-1)
    filled = np.where(nan, -np.inf, p)
    first_max = np.argmax(filled, axis=-1)
    return np.where(nan.any(-1), first_nan, first_max).astype(np.int8)


class Ring:
    """PlayedGamesDataset with capacity C, slots of L moves: slot -> (frames (n,T,S,S,S) int8, tokens (n,3S) int8,
    rewards (n,) f32); games enter at the pointer, which wraps."""

    def __init__(self, C, L):
        self.C, self.L, self.slots, self.pointer, self.added = C, L, {}, 0, 0

    def add_game(self, states, policy, rewards, length):
        n = int(length)
        self.slots[self.pointer] = (np.asarray(states[:n], np.int8), argmax_tokens(policy[:n]),
                                    np.asarray(rewards[:n], np.float32))
        self.pointer = (self.pointer + 1) % self.C
        self.added += 1

    def add(self, states, policy, rewards, lengths, select=False):
        """One tg_replay_add call: returns the status bit (a game with length 0 or > L is skipped)."""
        ok = [1 <= int(n) <= self.L for n in lengths]
        if select:
            b = best_pick(rewards, lengths, self.L)
            if b >= 0:
                self.add_game(states[b], policy[b], rewards[b], lengths[b])
        else:
            for b, good in enumerate(ok):
                if good:
                    self.add_game(states[b], policy[b], rewards[b], lengths[b])
        return 0 if all(ok) else 1

    def __len__(self):
        return sum(len(v[2]) for v in self.slots.values())

    def getitem(self, i):
        """(frames (T,S,S,S) int8, scalar = move index, tokens (3S,), reward), slots walked in slot order."""
        for s in range(self.C):
            if s not in self.slots:
                continue
            n = len(self.slots[s][2])
            if i < n:
                f, t, r = self.slots[s]
                return f[i], np.float32(i), t[i], r[i]
            i -= n
        raise IndexError(i)


def best_pick(rewards, lengths, L):
    """act_step's loop: the first game whose final reward is > every earlier one and > -1e6; -1 for none.  Games of
    length 0 or > L take no part."""
    best, pick = np.float32(-1e6), -1
    for b, n in enumerate(lengths):
        n = int(n)
        if not 1 <= n <= L:
            continue
        r = np.float32(rewards[b][n - 1])
        if r > best:
            best, pick = r, b
    return pick


def route(is_synth, index_synth, index_played, index_best, fract_best):
    """(kind, src) of every dataset index: __getitem__'s routing.  A position outside its index list is BAD."""
    is_synth = np.asarray(is_synth, bool)
    kind = np.full(len(is_synth), BAD, np.int64)
    src = np.full(len(is_synth), -1, np.int64)
    n_synth = 0
    for x, s in enumerate(is_synth):
        if s:
            if n_synth < len(index_synth):
                kind[x], src[x] = SYNTH, index_synth[n_synth]
            n_synth += 1
            continue
        r = x - n_synth
        lb = len(index_best) if (fract_best > 0 and index_best is not None) else 0
        if r < lb:
            kind[x], src[x] = BEST, index_best[r]
        elif index_played is not None and r - lb < len(index_played):
            kind[x], src[x] = PLAYED, index_played[r - lb]
    return kind, src


def mixed_items(kind, src, tokens, targets, played, best, T, shift=1):
    """(frames int8 (N,T,S,S,S), scalars f32 (N,1), actions int8 (N,3S), rewards f32 (N,1), status) of rows (kind, src):
    synthetic rows from ref_items, played / best rows from the rings, bad rows all zero with status 1."""
    tokens = np.asarray(tokens)
    S = tokens.shape[2] // 3
    N = len(kind)
    frames = np.zeros((N, T, S, S, S), np.int8)
    scalars = np.zeros((N, 1), np.float32)
    actions = np.zeros((N, 3 * S), np.int8)
    rewards = np.zeros((N, 1), np.float32)
    status = 0
    for n, (k, s) in enumerate(zip(kind, src)):
        ring = {PLAYED: played, BEST: best}.get(int(k))
        if int(k) == SYNTH:
            f, sc, a, rw, _, st = ref_items(tokens, targets, [s], T, shift)
            frames[n], scalars[n], actions[n], rewards[n] = f[0], sc[0], a[0], rw[0]
            status |= int(st[0])
        elif ring is not None and 0 <= s < len(ring):
            frames[n], scalars[n, 0], actions[n], rewards[n, 0] = ring.getitem(int(s))
        else:
            status |= 1
    return frames, scalars, actions, rewards, status
