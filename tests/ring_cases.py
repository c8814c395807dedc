"""What the GPU tests of the three entries that store games in a replay ring share (tg_replay_add, tg_replay_add_packed,
tg_replay_add_lists; csrc/tg_ring.h is their one protocol; not a test module): the same games in the three input forms,
the cases at the edges of the plan's 1024-item chunk and of the rebuild's slots per thread with their restatement
(replay_ref, replay_io_ref, replay_lists_ref stay the oracles), a ring between guard bytes, and the comparison of a
device ring with a restated one."""
import functools

import numpy as np

import replay_io_ref as IO
import replay_lists_ref as LR
import replay_ref as RR

ENTRIES = ("add", "add_packed", "add_lists")
ARRAYS = ("frames", "tokens", "rewards", "length", "offset", "ring")
S, T, L, N_LOGITS, SHIFT = 2, 1, 2, 2, 1  # the smallest games: tokens 0 and 1 (factors -1 and 0), lists of 1 or 2 moves
EDGE_N = (1023, 1024, 1025, 2049)  # candidates: one short of a plan chunk, a whole one, one more, two chunks and one
EDGE_C = (1, 3, 1025, 2049)        # slots: one; fewer than anything; two per rebuild thread, ragged; three, ragged


def edge_starts(C):
    """The values of ring[0] a case starts from: the first slot and the last."""
    return sorted({0, C - 1})


# ---- the same games in three forms --------------------------------------------------------------------------------------
def solvable_lists(rng, M, S=S, T=T, K=L, n_tokens=N_LOGITS):
    """M valid move lists of 1 .. K moves (both ends occur), one start state each: frame 0 is the sum of the list's
    terms, the history frames are random.  (starts int8 (M,T,S,S,S), tokens int8 (M,K,3S), lengths int64 (M,))."""
    tokens = rng.integers(0, n_tokens, size=(M, K, 3 * S)).astype(np.int8)
    lengths = rng.integers(1, K + 1, size=M).astype(np.int64)
    lengths[0], lengths[-1] = K, 1
    starts = rng.integers(-3, 4, size=(M, T, S, S, S)).astype(np.int8)
    for m in range(M):
        starts[m, 0] = -LR.heads_of(np.zeros((S, S, S), np.int32), tokens[m], int(lengths[m]), SHIFT)[-1]
    return starts, tokens, lengths


def three_forms(starts, tokens, lengths, ring_L, n_logits=N_LOGITS):
    """Valid lists as what each entry takes: dict(add=(states, policy, rewards, lengths int64), add_packed=(frames,
    tokens, rewards, lengths int32), add_lists=(starts, tokens, lengths int64))."""
    games = []
    for m in range(len(lengths)):
        flags, heads = LR.list_flags(starts, tokens[m], int(lengths[m]), m, tokens.shape[1], ring_L, SHIFT)
        assert flags == 0
        games.append(LR.game_of(starts[m], heads, tokens[m], int(lengths[m])))
    rows = tuple(np.concatenate([g[k] for g in games]) for k in range(3))
    return dict(add=LR.padded_form(starts, tokens, lengths, None, ring_L, SHIFT, n_logits),
                add_packed=rows + (lengths.astype(np.int32),), add_lists=(starts, tokens, lengths))


# ---- the edge cases -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(entry, N):
    """The arguments of ``entry`` for N candidates of which every seventh (3, 10, 17, ...) is invalid for that entry:
    a length of 0 or above L (and a negative one for add_packed), or, for add_lists, a list that does not reach zero.
    add's rewards are random, so that its best game is not simply the first shortest one."""
    rng = np.random.default_rng(N)
    starts, tokens, lengths = solvable_lists(rng, N)
    bad = np.arange(3, N, 7)
    if entry == "add_lists":
        lengths[bad[0::3]], lengths[bad[1::3]] = 0, L + 1
        starts[bad[2::3], 0, 0, 0, 0] += 1
        return starts, tokens, lengths
    form = three_forms(starts, tokens, lengths, L)[entry]
    if entry == "add":
        st, po, _, ln = form
        ln[bad[0::2]], ln[bad[1::2]] = 0, L + 1
        return st, po, -rng.integers(1, 9, size=(N, L)).astype(np.float32), ln
    ln = form[3].copy()
    ln[bad[0::3]], ln[bad[1::3]], ln[bad[2::3]] = 0, L + 1, -1
    M = int(np.maximum(ln, 0).sum())  # (the rows of a game do not depend on the games around it: fresh random rows)
    return (rng.integers(-3, 4, size=(M, T, S, S, S)).astype(np.int8),
            rng.integers(0, N_LOGITS, size=(M, 3 * S)).astype(np.int8), -rng.integers(1, 9, size=M).astype(np.float32), ln)


def restate(entry, args, C, first, select=False):
    """One call of ``entry`` on an empty ring of C slots whose pointer is ``first``: (the ring, the status bits, stored
    or None)."""
    ring = RR.Ring(C, L)
    ring.pointer = first
    if entry == "add":
        return ring, (ring.add(*args, select=True) if select else IO.add_games(ring, *args)), None
    if entry == "add_packed":
        return ring, IO.add_packed(ring, *args), None
    stored, status = LR.add_lists(ring, *args, shift=SHIFT, select=bool(select))
    return ring, status, stored


# ---- device rings -------------------------------------------------------------------------------------------------------
def guarded_buffer(C, L, T, S, device="cuda:0"):
    """A GameBuffer whose six arrays lie between guard bytes; frames, tokens and rewards are poisoned, so whatever a
    call leaves outside the stored moves is seen."""
    import torch

    from guarded_buffers import CANARY, guarded
    from mat_mul_amd import GameBuffer, _lib

    buf = GameBuffer(C, L, T, S, device)
    buf.guards = {}
    for name in ARRAYS:
        old = getattr(buf, name)
        raw, t = guarded(tuple(old.shape), old.dtype, device)
        if name in ("length", "offset", "ring"):
            t.zero_()
        buf.guards[name] = raw
        setattr(buf, name, t)
    buf.desc = _lib.ReplayBufferDesc(C, L, T, S, *(getattr(buf, n).data_ptr() for n in ARRAYS))
    poison = np.frombuffer(bytes([CANARY] * 4), np.float32)[0]
    buf.shadow = (np.full((C, L, T, S, S, S), CANARY, np.int8), np.full((C, L, 3 * S), CANARY, np.int8),
                  np.full((C, L), poison, np.float32))
    torch.cuda.synchronize()
    return buf


def assert_ring(buf, want, what=""):
    """Every valid byte of the device buffer equals the restatement's ring."""
    host = lambda t: t.cpu().numpy()
    length, offset, ring = host(buf.length), host(buf.offset), host(buf.ring)
    assert ring.tolist() == [want.pointer, want.added], what
    assert length.tolist() == [len(want.slots[s][2]) if s in want.slots else 0 for s in range(buf.C)], what
    assert offset.tolist() == [0] + np.cumsum(length).tolist(), what
    frames, tokens, rewards = host(buf.frames), host(buf.tokens), host(buf.rewards)
    for s, (f, t, r) in want.slots.items():
        n = len(r)
        assert np.array_equal(frames[s, :n], f) and np.array_equal(tokens[s, :n], t), (what, s)
        assert np.array_equal(rewards[s, :n].view(np.uint32), r.view(np.uint32)), (what, s)


def ring_of(buf):
    """The device buffer as a replay_ref.Ring (its stored moves only)."""
    host = lambda t: t.cpu().numpy()
    ring = RR.Ring(buf.C, buf.L)
    ring.pointer, ring.added = (int(x) for x in host(buf.ring))
    frames, tokens, rewards = host(buf.frames), host(buf.tokens), host(buf.rewards)
    for s, n in enumerate(host(buf.length).tolist()):
        if n:
            ring.slots[s] = (frames[s, :n].copy(), tokens[s, :n].copy(), rewards[s, :n].copy())
    return ring


def check_edges(entry, N, C, device="cuda:0"):
    """``entry`` with the N candidates of ``edge_case`` into an empty ring of C slots, from each starting ring[0] and with
    each select rule it has: the device leaves length, offset, ring and every valid byte as the restatement does."""
    from mat_mul_amd import GameBuffer

    args = edge_case(entry, N)
    for first in edge_starts(C):
        for select in (False,) if entry == "add_packed" else (False, True):
            want, status, want_stored = restate(entry, args, C, first, select)
            assert want.added >= 1 and status, "the case stores a game and rejects one"
            buf = GameBuffer(C, L, T, S, device)
            buf.ring[0] = first
            stored = call_entry(entry, buf, args, select, buf.status)
            assert_ring(buf, want, (first, select))
            assert int(buf.status[0]) == status, (first, select)
            if want_stored is not None:
                assert stored.cpu().numpy().tolist() == want_stored.tolist(), (first, select)


def call_entry(entry, buf, args, select=False, status=None):
    """``entry`` on the device with host arrays as ``edge_case`` and ``three_forms`` give them; returns stored or None."""
    import torch

    from mat_mul_amd import ops

    d = [torch.from_numpy(np.ascontiguousarray(x)).to(buf.device) for x in args]
    if entry == "add":
        return ops.replay_add(buf, *d, select=bool(select), status=status)
    if entry == "add_packed":
        return ops.replay_add_packed(buf, *d, status=status)
    return ops.replay_add_lists(buf, *d, shift=SHIFT, select=bool(select), status=status)
