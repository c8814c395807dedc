"""numpy restatement of the solution search over a queue of start states (tg_rollout_advance_slots and tg_rollout_refill
of include/tensor_game_rollout_slots.h, ``solve_stream`` of mat_mul_amd/rollout.py), on top of tests/rollout_ref.py and
tests/rollout_masked_ref.py.  Shared by test_rollout_slots_cpu.py, test_gpu_rollout_slots.py and
test_gpu_rollout_sizes.py; the case tables of those tests are in rollout_slots_cases.py."""
import copy

import numpy as np

import rollout_masked_ref as M
import rollout_ref as R
from net_ref import philox_uniforms

ROW_FIELDS = ("frames", "scalars", "nnz", "overflow", "active", "actions", "rows", "uniforms")
SLOT_FIELDS = ("best_nnz", "hits", "solved_step", "solved_sample", "slot_state", "slot_step")
OUT_FIELDS = ("best_nnz", "hits", "solved_step", "solved_sample", "overflow", "tokens")


class Slots:
    """The slot-side buffers, as ``ops.rollout_slots`` allocates them (everything empty)."""

    def __init__(self, R_, n, S, T, dim_s, K):
        B = R_ * n
        self.n, self.S, self.T, self.K = n, S, T, K
        self.frames = np.zeros((B, T, S, S, S), np.int8)
        self.scalars = np.zeros((B, dim_s), np.float32)
        self.nnz = np.zeros(B, np.int32)
        self.overflow = np.zeros(B, np.uint8)
        self.active = np.zeros(B, np.uint8)
        self.actions = np.zeros((B, K, 3 * S), np.int8)
        self.rows = np.full(B, -1, np.int64)
        self.uniforms = np.zeros((B, 1, 3 * S), np.float32)
        self.best_nnz, self.hits, self.solved_step, self.solved_sample = R.fresh_records(R_, S)
        self.slot_state = np.full(R_, -1, np.int64)
        self.slot_step = np.zeros(R_, np.int32)
        self.head = np.zeros(1, np.int64)
        self.live = np.zeros(1, np.int32)

    @property
    def records(self):
        return (self.best_nnz, self.hits, self.solved_step, self.solved_sample)

    def copy(self):
        return copy.deepcopy(self)


class Out:
    """The dense per-state outputs of the refill; ``fill`` is what they hold before a state is flushed."""

    def __init__(self, N, S, K, fill=None):
        self.best_nnz = np.full(N, S ** 3 if fill is None else fill, np.int32)
        self.hits = np.full(N, 0 if fill is None else fill, np.int32)
        self.solved_step = np.full(N, -1 if fill is None else fill, np.int32)
        self.solved_sample = np.full(N, -1 if fill is None else fill, np.int32)
        self.overflow = np.full(N, 0 if fill is None else fill, np.uint8)
        self.tokens = np.full((N, K, 3 * S), 0 if fill is None else fill, np.int8)


def live_slots(sl):
    return (sl.slot_state >= 0) & (sl.solved_step < 0) & (sl.slot_step < sl.K)


def advance_slots(sl, tokens, shift=1):
    """tg_rollout_advance_slots, in place on ``sl``: the live slots are stepped one by one through the masked
    restatement with step = their own slot_step (a group's result depends on nothing outside the group)."""
    n = sl.n
    tokens = np.asarray(tokens, np.int8)
    for g in np.nonzero(live_slots(sl))[0]:
        r = slice(g * n, (g + 1) * n)
        rec = tuple(x[g:g + 1] for x in sl.records)
        fr, nnz, rec2, sc, ovf, act, active = M.advance_masked(sl.frames[r], tokens[r], n, int(sl.slot_step[g]), rec,
                                                               sl.nnz[r], sl.scalars[r], sl.overflow[r], sl.actions[r],
                                                               sl.active[r], shift)
        sl.frames[r], sl.nnz[r], sl.scalars[r], sl.overflow[r], sl.actions[r], sl.active[r] = fr, nnz, sc, ovf, act, active
        for x, y in zip(sl.records, rec2):
            x[g] = y[0]
        sl.slot_step[g] += 1


def refill(sl, out, q_states, q_scalars, seed=0, first_state=0, uniforms=True):
    """tg_rollout_refill, in place on ``sl`` and ``out`` (vectorised over the slots: R goes up to 65 536)."""
    n, S, K = sl.n, sl.S, sl.K
    N, R_ = len(q_states), len(sl.slot_state)
    if N == 0 or R_ == 0:
        return
    finished = (sl.slot_state >= 0) & ((sl.solved_step >= 0) | (sl.slot_step >= K))
    empty = sl.slot_state < 0
    # 1. flush the finished slots to their states
    gf = np.nonzero(finished)[0]
    q = sl.slot_state[gf]
    out.best_nnz[q], out.hits[q] = sl.best_nnz[gf], sl.hits[gf]
    out.solved_step[q], out.solved_sample[q] = sl.solved_step[gf], sl.solved_sample[gf]
    out.overflow[q] = sl.overflow.reshape(R_, n)[gf].any(axis=1).astype(np.uint8)
    won = sl.solved_step[gf] >= 0
    win_rows = gf * n + np.where(won, sl.solved_sample[gf], 0)
    keep = np.arange(K)[None, :] <= np.where(won, sl.solved_step[gf], -1)[:, None]
    out.tokens[q] = sl.actions[win_rows] * keep[:, :, None].astype(np.int8)
    # 2. the next states, in slot order
    want = np.nonzero(finished | empty)[0]
    head = int(sl.head[0])
    qs = head + np.arange(len(want), dtype=np.int64)
    take = qs < N
    gt, qt, gd = want[take], qs[take], want[~take]
    sl.head[0] = head + min(len(want), max(N - head, 0))
    # 3. fill the slots that take a state; the others go (or stay) empty
    sl.frames.reshape((R_, n) + sl.frames.shape[1:])[gt] = np.asarray(q_states)[qt][:, None]
    sl.scalars.reshape(R_, n, -1)[gt] = np.asarray(q_scalars, np.float32)[qt][:, None]
    sl.best_nnz[gt], sl.hits[gt], sl.solved_step[gt], sl.solved_sample[gt] = S ** 3, 0, -1, -1
    sl.slot_state[gt], sl.slot_step[gt] = qt, 0
    sl.nnz.reshape(R_, n)[gt] = 0
    sl.overflow.reshape(R_, n)[gt] = 0
    sl.rows.reshape(R_, n)[gt] = (first_state + qt)[:, None] * n + np.arange(n)[None, :]
    sl.slot_state[gd] = -1
    sl.rows.reshape(R_, n)[gd] = -1
    # 4. every state held now is unfinished
    holds = sl.slot_state >= 0
    sl.active[:] = np.repeat(holds, n).astype(np.uint8)
    sl.live[0] = int(holds.sum())
    # 5. the uniforms of the rows that will be evaluated: the header rule at (row key, call = the slot's own step)
    if uniforms:
        row_step = np.repeat(sl.slot_step, n)
        row_holds = np.repeat(holds, n)
        for call in np.unique(sl.slot_step[holds]):
            sel = row_holds & (row_step == call)
            u = philox_uniforms(seed, sl.rows[sel], int(call), 1, 3 * S)
            u32 = u.astype(np.float32)
            assert np.array_equal(u32.astype(np.float64), u)           # exactly representable
            sl.uniforms[sel] = u32


def bound(N, R_, K):
    return K * (N // R_ + 1)


def solve_stream(policy, states, scalars, n, K, R_, shift=1, first_state=0, seed=None):
    """The loop of ``rollout.solve_stream``: policy(frames, scalars, rows, steps) -> tokens int8 (B,3S) sees all rows
    (``steps`` int32 (B,): each row's own step; the rows of empty slots have row key -1).  With ``seed`` the uniforms
    are generated too and the policy is called as policy(frames, scalars, rows, steps, active, uniforms).  Returns a
    ``rollout_ref.Result`` with the fields of SolveResult."""
    states = np.asarray(states, np.int8)
    N, T, S = states.shape[:3]
    sl = Slots(R_, n, S, T, np.asarray(scalars).shape[1], K)
    out = Out(N, S, K)
    ticks = 0
    if N:
        refill(sl, out, states, scalars, seed or 0, first_state, seed is not None)
        while sl.live[0] != 0:
            assert ticks < bound(N, R_, K), (ticks, N, R_, K)
            steps = np.repeat(sl.slot_step, n).astype(np.int32)
            if seed is None:
                tokens = policy(sl.frames, sl.scalars, sl.rows, steps)
            else:
                tokens = policy(sl.frames, sl.scalars, sl.rows, steps, sl.active, sl.uniforms)
            advance_slots(sl, np.asarray(tokens, np.int8), shift)
            refill(sl, out, states, scalars, seed or 0, first_state, seed is not None)
            ticks += 1
    r = R.Result()
    r.best_nnz, r.hits, r.solved_step, r.solved_sample = out.best_nnz, out.hits, out.solved_step, out.solved_sample
    r.overflow, r.ticks, r.steps_run = out.overflow, ticks, (ticks,)
    r.groups = np.nonzero(out.solved_step >= 0)[0].astype(np.int64)
    r.tokens = out.tokens[r.groups]
    r.lengths = out.solved_step[r.groups].astype(np.int64) + 1
    return r


def solve_states(policy, states, scalars, n, K, shift=1):
    """``rollout.solve_states`` in one chunk: policy(frames, scalars, rows, step) with the host step."""
    m = M.rollout_masked(policy, states, scalars, n, K, shift)
    r = R.Result()
    r.best_nnz, r.hits, r.solved_step, r.solved_sample = m.best_nnz, m.hits, m.solved_step, m.solved_sample
    r.groups, r.tokens, r.lengths = R.solutions(m)
    r.overflow = m.overflow.reshape(-1, n).max(axis=1) if len(states) else m.overflow
    return r


RESULT_FIELDS = ("best_nnz", "hits", "solved_step", "solved_sample", "groups", "tokens", "lengths")


def check_equal(stream, chunked, get=np.asarray):
    for name in RESULT_FIELDS:
        assert np.array_equal(get(getattr(stream, name)), get(getattr(chunked, name))), name


def keyed_table_policy(table, n):
    """(stream policy, chunk policy) that both play table[row key, the row's step] (table int8 (rows, K, 3S)); a row
    key of -1 (an empty slot) plays table[-1], which cannot matter."""
    K = table.shape[1]

    def stream(frames, scalars, rows, steps):
        return table[rows, np.minimum(steps, K - 1)]

    def chunk(frames, scalars, rows, step):
        return table[rows, step]

    return stream, chunk


def scripted_table(scripts, S, n, slot, shift, K, seed=0, values=3):
    """int8 (G*n, K, 3S): ``rollout_ref.scripted_policy`` as a table indexed by (row, step)."""
    pol = R.scripted_policy(scripts, S, n, slot, shift, seed, values)
    return np.stack([pol(None, None, None, k) for k in range(K)], axis=1)
