"""Host restatement of tg_replay_pack / tg_replay_add_packed (include/tensor_game_replay_io.h) and of the buffer file
of mat_mul_amd.replay_io (not a test module), in numpy on the ``replay_ref.Ring`` (slot -> (frames, tokens, rewards)).
tests/test_replay_io_cpu.py checks it against tests/golden/replay_cases.npz; tests/test_gpu_replay_io.py checks the
device against it."""
import struct

import numpy as np

from replay_ref import Ring, argmax_tokens

BAD_LENGTH, TRUNCATED = 1, 2


def age_slots(ring):
    """The slots that hold a game, oldest first: age position j is slot (pointer + j) mod C."""
    return [s for s in ((ring.pointer + j) % ring.C for j in range(ring.C)) if s in ring.slots]


def pack(ring, T, S, max_moves=None):
    """tg_replay_pack: dict(lengths int32 (G,), move_offset int64 (G+1,), counts int64 (2,), written = the rows that
    are written (whole games inside max_moves), rewards / tokens / frames of those rows, status)."""
    slots = age_slots(ring)
    lengths = np.array([len(ring.slots[s][2]) for s in slots], np.int32)
    off = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
    G, M = len(slots), int(off[-1])
    cap = M if max_moves is None else int(max_moves)
    whole = [r for r in range(G) if off[r + 1] <= cap]
    written = int(off[len(whole)])
    assert whole == list(range(len(whole)))  # rows rise with the rank: the games that fit are a prefix
    cat = lambda k, shape, dt: (np.concatenate([ring.slots[slots[r]][k] for r in whole]).astype(dt) if whole
                                else np.zeros(shape, dt))
    return dict(lengths=lengths, move_offset=off, counts=np.array([G, M], np.int64), written=written,
                frames=cat(0, (0, T, S, S, S), np.int8), tokens=cat(1, (0, 3 * S), np.int8),
                rewards=cat(2, (0,), np.float32), status=TRUNCATED if M > cap else 0)


def add_packed(ring, frames, tokens, rewards, lengths, M=None, first_slot=-1, games_added=-1):
    """tg_replay_add_packed on the Ring; returns the status bits.  No games: a no-op, whatever the other arguments."""
    if len(lengths) == 0:
        return 0
    M = len(rewards) if M is None else int(M)
    status, start, stored = 0, 0, []
    for n in (int(x) for x in lengths):
        if not 1 <= n <= ring.L:
            status |= BAD_LENGTH
        elif start + n > M:
            status |= TRUNCATED
        else:
            stored.append((start, n))
        start += max(n, 0)
    V = len(stored)
    nxt = ring.pointer if first_slot < 0 else int(first_slot)
    for r, (lo, n) in enumerate(stored):
        if r >= V - min(V, ring.C):  # more than C in one call: only the last C are written
            ring.slots[(nxt + r) % ring.C] = (np.asarray(frames[lo:lo + n], np.int8),
                                              np.asarray(tokens[lo:lo + n], np.int8),
                                              np.asarray(rewards[lo:lo + n], np.float32))
    ring.pointer = (nxt + V) % ring.C
    ring.added = int(games_added) if games_added >= 0 else ring.added + V
    return status


def buffer_words(ring):
    """(length int32 (C,), offset int64 (C+1,), ring int64 (2,)) of the device buffer that holds ``ring``."""
    length = np.array([len(ring.slots[s][2]) if s in ring.slots else 0 for s in range(ring.C)], np.int32)
    return length, np.concatenate([[0], np.cumsum(length, dtype=np.int64)]).astype(np.int64), \
        np.array([ring.pointer, ring.added], np.int64)


def rings_equal(a, b):
    return (a.C, a.L, a.pointer, a.added, sorted(a.slots)) == (b.C, b.L, b.pointer, b.added, sorted(b.slots)) and all(
        np.array_equal(x, y, equal_nan=True) for s in a.slots for x, y in zip(a.slots[s], b.slots[s]))


def copy_ring(ring):
    out = Ring(ring.C, ring.L)
    out.slots, out.pointer, out.added = dict(ring.slots), ring.pointer, ring.added
    return out


def file_bytes(C, L, T, S, ring, lengths, rewards, tokens, frames):
    """The buffer file: ``TGREPLY1``, fifteen little-endian int64 (C, L, T, S, G, M, ring[0], ring[1], seven zeros),
    then lengths int32, rewards float32, tokens int8, frames int8."""
    lengths = np.asarray(lengths, "<i4")
    head = struct.pack("<8s15q", b"TGREPLY1", C, L, T, S, len(lengths), int(lengths.sum()), ring[0], ring[1],
                       0, 0, 0, 0, 0, 0, 0)
    return head + lengths.tobytes() + np.asarray(rewards, "<f4").tobytes() + np.asarray(tokens, np.int8).tobytes() + \
        np.asarray(frames, np.int8).tobytes()


def add_games(ring, states, policy, rewards, lengths):
    """``Ring.add(select=False)`` with the argmax taken once for the whole batch (the same slots, pointer and count;
    quick enough for the capacity bound); returns the status bit."""
    tok = argmax_tokens(policy)
    bad = 0
    for b, n in enumerate(int(x) for x in lengths):
        if not 1 <= n <= ring.L:
            bad = 1
            continue
        ring.slots[ring.pointer] = (np.asarray(states[b, :n], np.int8), tok[b, :n], np.asarray(rewards[b, :n], np.float32))
        ring.pointer = (ring.pointer + 1) % ring.C
        ring.added += 1
    return bad
