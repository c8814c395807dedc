"""Case tables and input builders of the slot kernels' tests (tg_rollout_advance_slots, tg_rollout_refill), numpy only:
what test_gpu_rollout_slots.py and test_gpu_rollout_sizes.py put on the device, and what test_rollout_slots_cpu.py
checks of the same tables through the restatement (tests/rollout_slots_ref.py) alone, so that a case which no longer
reaches what it was written for shows up without a GPU."""
import numpy as np

import rollout_ref as R
import rollout_slots_ref as SR

EMPTY, SOLVED, EXHAUSTED, LIVE0, LIVE2, LIVE_LAST = range(6)
ADVANCE_K = 4                                             # max_actions of the advance cases
KIND_STEPS = [1, 2, ADVANCE_K, 0, 2, ADVANCE_K - 1]       # slot_step of the six kinds

# (S, T, n, R, misalign): many small groups per workgroup; the dword path with a 3-byte tail, misaligned frames; S = 9;
# one group per workgroup with 16-byte items; T = 8
ADVANCE_CASES = [(4, 2, 4, 37, 0), (3, 1, 1, 9, 1), (9, 3, 3, 7, 0), (16, 2, 64, 2, 0), (5, 8, 2, 6, 0)]

# (S, T, n, R, misalign), each the first case to reach: S = 25 (15 625-byte frames: dwords and a ONE-byte tail item, one
# group per workgroup); the same off its alignment with T = 1 (the head alone is loaded) and n = 1; S = 32 = TG_MAX_S
# (96-byte token rows, 2048 16-byte items per row); S % 4 == 0 with frames off their 16-byte alignment (dwords, NO tail
# item); 256 groups in workgroup 0 -- four passes of the 64-wide scan, s_act / s_step filled beyond 64 -- and a partial
# second workgroup of 44; the same on the dword path with two rows per group
SIZE_CASES = [(25, 3, 4, 7, 0), (25, 1, 1, 6, 3), (32, 2, 2, 6, 0), (16, 2, 8, 6, 1), (4, 1, 1, 300, 0),
              (2, 2, 2, 300, 0)]
WIDE_CASES = SIZE_CASES[-2:]                              # more than 64 groups per workgroup, more than one workgroup
PLANTED_CASE = (4, 1, 1, 256, 0)                          # one workgroup: 200 dead slots, then 56 live ones

# kRollItems, kRollMaxRows, kRollTokBytes of mat_mul_amd/csrc/tg_rollout.hip
ROLL_ITEMS, ROLL_MAX_ROWS, ROLL_TOK_BYTES = 1024, 1024, 6144


def groups_per_workgroup(S, n, R_, misalign):
    """The host rule of rollout_entry (tg_rollout.hip), restated: about ROLL_ITEMS items per workgroup, within the LDS
    tables for the rows and for their tokens, at least one group and no more than there are."""
    W = 16 if S % 4 == 0 and misalign % 16 == 0 else 4
    ipr = (S ** 3 + W - 1) // W
    gpw = ROLL_ITEMS // (n * ipr)
    gpw = min(gpw, ROLL_MAX_ROWS // n)
    gpw = min(gpw, ROLL_TOK_BYTES // (n * 3 * S))
    return max(1, min(gpw, R_))


def slot_words(sl, kinds, rng):
    """The slot words and records that make slot g of ``sl`` the kind kinds[g] (K = ADVANCE_K)."""
    R_ = len(kinds)
    sl.slot_state[:] = np.where(kinds == EMPTY, -1, rng.integers(0, 50, size=R_))
    sl.solved_step[:] = np.where(kinds == SOLVED, 1, -1)
    sl.solved_sample[:] = np.where(kinds == SOLVED, 0, -1)
    sl.hits[:] = kinds == SOLVED
    sl.slot_step[:] = np.choose(kinds, KIND_STEPS)


def advance_inputs(S, T, n, kinds, rng, dim_s=2):
    """(slots, tokens int8 (B,3S)) of one advance_slots launch at shift 1 in which slot g is of kind kinds[g]: arbitrary
    rows and records everywhere, a LIVE2 slot solved by this step through its sample g % n (the head is the tensor of
    the row's action), and the tokens of the rows that are not live poisoned with 127, which must not be read."""
    R_, K = len(kinds), ADVANCE_K
    B = R_ * n
    sl = SR.Slots(R_, n, S, T, dim_s, K)
    sl.frames[:] = rng.integers(-2, 3, size=sl.frames.shape)
    sl.scalars[:] = rng.integers(0, 5, size=sl.scalars.shape)
    sl.nnz[:] = rng.integers(1, 9, size=B)
    sl.active[:] = rng.integers(0, 2, size=B)
    sl.actions[:] = rng.integers(0, 3, size=sl.actions.shape)
    sl.rows[:] = np.arange(B) + 11
    sl.best_nnz[:] = rng.integers(1, S ** 3, size=R_)
    slot_words(sl, kinds, rng)
    tokens = rng.integers(0, 3, size=(B, 3 * S)).astype(np.int8)
    for g in np.nonzero(kinds == LIVE2)[0]:
        b = g * n + g % n
        tokens[b] = rng.choice([0, 2], size=3 * S)
        sl.frames[b, 0] = np.asarray(R.O.action_to_tensor(tokens[b][None], 1))[0]
    live = np.repeat(SR.live_slots(sl), n)
    assert np.array_equal(SR.live_slots(sl), kinds >= LIVE0)
    tokens[~live] = 127
    return sl, tokens


def advance_launches(S, T, n, R_, rng):
    """The launches of one advance case, as (rot, kinds, slots, tokens): slot g is of kind (g + rot) % 6, over as many
    launches as R needs to meet all six kinds."""
    for rot in range(0, 6, min(R_, 6)):
        kinds = (np.arange(R_) + rot) % 6
        yield (rot, kinds) + advance_inputs(S, T, n, kinds, rng)


def check_advance(kinds, n, before, sl):
    """What the restatement must have done to ``before`` for a case to mean anything."""
    R_ = len(kinds)
    gl = kinds >= LIVE0
    live = np.repeat(gl, n)
    assert np.array_equal(sl.slot_step[gl], before.slot_step[gl] + 1)
    assert np.array_equal(sl.slot_step[~gl], before.slot_step[~gl])
    assert (sl.solved_step[kinds == LIVE2] == 2).all() and (sl.solved_sample[kinds == LIVE2] ==
                                                             (np.arange(R_) % n)[kinds == LIVE2]).all()
    assert np.array_equal(sl.frames[~live], before.frames[~live])
    assert not live.any() or (sl.frames[live] != before.frames[live]).any()


def planted_kinds(R_=PLANTED_CASE[3], dead=200):
    """Slots 0 .. dead-1 empty, solved or exhausted in turn, the others live at their first, third and last step."""
    g = np.arange(R_)
    return np.where(g < dead, g % 3, LIVE0 + g % 3)


# ---- overflow in slot mode ----------------------------------------------------------------------------------------------
# (S, T, n, R): several groups per workgroup with 16-byte items; S = 25 (dwords, one group per workgroup)
OVERFLOW_CASES = [(4, 2, 4, 12), (25, 1, 2, 6)]
OVERFLOW_SHIFT = 2


def overflow_inputs(S, T, n, R_, rng, dim_s=1):
    """(slots, tokens, q_states, q_scalars) at max_actions = 1 and shift 2: slot g is empty, solved, exhausted or live
    as g % 4 says (a live slot is finished by its one step).  EVERY row, live or not, has a head with 127 at (0,0,0)
    and -128 at (0,0,1) and entries of [-2, 2] elsewhere; an even row plays u_0 = v_0 = 1 with w_0 = -1, w_1 = 1, which
    takes both planted entries out of int8 (127 + 1, -128 - 1), an odd row plays u_0 = 0, which leaves the whole slice
    i = 0 as it is; the other factors are random in [-2, 2], so no other entry can leave int8 (|2 + 8| < 128).  The
    slots hold the states 0 .. R-1 of a queue of 2R + 3 whose head stands at R: every slot takes a new state."""
    B, K, N = R_ * n, 1, 2 * R_ + 3
    kinds = np.arange(R_) % 4
    sl = SR.Slots(R_, n, S, T, dim_s, K)
    sl.frames[:] = rng.integers(-2, 3, size=sl.frames.shape)
    sl.frames[:, 0, 0, 0, 0], sl.frames[:, 0, 0, 0, 1] = 127, -128
    sl.scalars[:] = rng.integers(0, 5, size=sl.scalars.shape)
    sl.nnz[:] = rng.integers(1, 9, size=B)
    sl.active[:] = 1
    sl.rows[:] = np.arange(B) + 11
    sl.best_nnz[:] = rng.integers(1, S ** 3, size=R_)
    sl.slot_state[:] = np.where(kinds == EMPTY, -1, np.arange(R_))
    sl.solved_step[:] = np.where(kinds == SOLVED, 0, -1)
    sl.solved_sample[:] = np.where(kinds == SOLVED, 0, -1)
    sl.hits[:] = kinds == SOLVED
    sl.slot_step[:] = np.where((kinds == SOLVED) | (kinds == EXHAUSTED), 1, 0)
    sl.head[0] = R_
    assert np.array_equal(SR.live_slots(sl), kinds == LIVE0)
    factors = rng.integers(-2, 3, size=(B, 3, S))
    even = np.arange(B) % 2 == 0
    factors[even, 0, 0], factors[even, 1, 0], factors[even, 2, 0], factors[even, 2, 1] = 1, 1, -1, 1
    factors[~even, 0, 0] = 0
    tokens = (factors + OVERFLOW_SHIFT).reshape(B, 3 * S).astype(np.int8)
    q_states = rng.integers(-2, 3, size=(N, T, S, S, S)).astype(np.int8)
    q_scalars = rng.integers(0, 9, size=(N, dim_s)).astype(np.float32)
    return sl, tokens, q_states, q_scalars


def check_overflow_step(n, before, sl, tokens):
    """After the restatement's step of ``before``: the live rows hold what oracle.tensor_game.step_i8 gives them (wrapped
    as tg_step_i8 wraps) and its flags, at least one of them is flagged and one is not, and the other rows are as they
    were, unflagged."""
    live = np.repeat(SR.live_slots(before), n)
    assert not before.overflow.any()
    head, _, ovf = R.O.step_i8(before.frames[live, 0], tokens[live], OVERFLOW_SHIFT)
    assert np.array_equal(sl.frames[live, 0], head) and np.array_equal(sl.overflow[live], np.asarray(ovf, np.uint8))
    assert sl.overflow[live].any() and not sl.overflow[live].all()
    flagged = sl.frames[live][sl.overflow[live] == 1]
    assert (flagged[:, 0, 0, 0, 0] == -128).all() and (flagged[:, 0, 0, 0, 1] == 127).all()     # 127 + 1, -128 - 1
    assert np.array_equal(sl.frames[~live], before.frames[~live]) and not sl.overflow[~live].any()
    assert np.array_equal(sl.nnz[~live], before.nnz[~live])


def check_overflow_flush(n, stepped, sl, out):
    """After the restatement's refill of ``stepped``: out.overflow is the OR of the rows' flags per flushed state (set
    for some, clear for others), and no slot keeps a flag."""
    held = stepped.slot_state >= 0
    assert held.any() and (SR.live_slots(stepped) == 0).all()          # K = 1: every slot that holds a state is finished
    want = np.full(len(out.overflow), 77, np.uint8)
    want[stepped.slot_state[held]] = stepped.overflow.reshape(-1, n)[held].any(axis=1)
    assert np.array_equal(out.overflow, want)
    assert (want == 1).any() and (want == 0).any()
    assert not sl.overflow.any() and (sl.slot_state >= len(held)).all()


# ---- the refill ---------------------------------------------------------------------------------------------------------
# (S, T, n, R, N, K, first_state, misalign): 16-byte copies; R = 1 on the dword path (27-byte rows); 729*T-byte rows and
# n = 64; R crosses a scan thread's 64 slots and the queue runs dry inside a tick; R > N; R crosses wavefronts; the
# maximum R; misaligned frames at S = 4 (the dword path without a tail)
REFILL_CASES = [(4, 2, 4, 5, 40, 4, 7, 0), (3, 1, 1, 1, 6, 3, 0, 0), (9, 3, 64, 3, 7, 2, 3, 0),
                (3, 2, 4, 65, 100, 3, 1, 1), (4, 1, 2, 9, 4, 3, 5, 0), (2, 1, 1, 5000, 12000, 3, 2, 0),
                (1, 1, 1, 65536, 100000, 2, 0, 0), (4, 2, 2, 6, 20, 3, 0, 4)]

# the same fields, each the first case to reach: the 16-byte copy at a real row size (8 KiB rows, n * ipr = 4096 items
# for a block of 256); S = 16 with the queue AND the frames off their alignment (dwords, no tail); S = 32 with n = 64
# (131 072 items per slot); S = 25 with T = 1, 2, 3: 15 625 * T-byte rows, a tail of 1, 2 and 3 bytes behind the
# dwords, the last one misaligned too, and 75 uniforms per row (18 whole Philox quads and three words of the 19th);
# row keys (first_state + q) * n + s that cross 2^32 inside the run
KEY_CASE = (4, 1, 4, 6, 20, 3, 2 ** 30 - 3, 0)
REFILL_SIZE_CASES = [(16, 2, 8, 5, 12, 3, 1, 0), (16, 1, 2, 4, 9, 2, 0, 4), (32, 1, 64, 2, 5, 2, 0, 0),
                     (25, 1, 4, 3, 7, 2, 0, 0), (25, 2, 1, 3, 7, 2, 5, 0), (25, 3, 4, 3, 7, 2, 0, 1), KEY_CASE]
REFILL_SEED = 0x1234567887654321


def play(sl, rng):
    """What some steps of the search could leave behind: about half of the occupied slots solved, some exhausted, the
    others somewhere on their way, with arbitrary records, actions, counts and a few overflow flags."""
    R_, n, K, B = len(sl.slot_state), sl.n, sl.K, len(sl.nnz)
    held = sl.slot_state >= 0
    fate = rng.integers(0, 4, size=R_)           # 0, 1: solved; 2: exhausted; 3: on its way
    solved, done = held & (fate <= 1), held & (fate == 2)
    sl.slot_step[held] = rng.integers(1, K, size=int(held.sum())) if K > 1 else 1
    sl.slot_step[done] = K
    sl.solved_step[solved] = sl.slot_step[solved] - 1
    sl.slot_step[solved & (fate == 1)] = K       # solved by its last step
    sl.solved_step[solved & (fate == 1)] = K - 1
    sl.solved_sample[solved] = rng.integers(0, n, size=int(solved.sum()))
    sl.hits[solved] = 1
    sl.best_nnz[held] = np.where(solved, 0, rng.integers(1, sl.S ** 3 + 1, size=R_))[held]
    sl.actions[:] = rng.integers(1, 4, size=sl.actions.shape)
    sl.nnz[:] = rng.integers(0, 9, size=B)
    sl.overflow[:] = rng.integers(0, 8, size=B) == 0
    sl.frames[:] = rng.integers(-2, 3, size=sl.frames.shape)
    sl.scalars[:] += 1


class RefillRun:
    """The three ticks of one refill case through the restatement: ``ticks()`` yields (tick, the slots as the tick finds
    them) after ``slots`` and ``out`` have been brought to what the tick leaves, so a device run of the same tick can be
    compared with them; ``dry`` says whether the queue ran dry inside a tick that still had states to hand out."""

    def __init__(self, S, T, n, R_, N, K, first_state, misalign, dim_s=2):
        self.rng = np.random.default_rng(S + 10 * n + R_)
        self.n, self.N, self.K, self.first_state = n, N, K, first_state
        self.q_states = self.rng.integers(-2, 3, size=(N, T, S, S, S)).astype(np.int8)
        self.q_scalars = self.rng.integers(0, 9, size=(N, dim_s)).astype(np.float32)
        self.slots, self.out = SR.Slots(R_, n, S, T, dim_s, K), SR.Out(N, S, K, fill=77)
        self.slots.uniforms[:] = 2.0             # no draw is 2: the rows that get none keep it
        self.dry = False

    def ticks(self):
        sl = self.slots
        for tick in range(3):
            if tick:
                play(sl, self.rng)
            wanting = int(((sl.slot_state < 0) | (sl.solved_step >= 0) | (sl.slot_step >= self.K)).sum())
            self.dry |= 0 < self.N - int(sl.head[0]) < wanting
            before = sl.copy()
            SR.refill(sl, self.out, self.q_states, self.q_scalars, REFILL_SEED, self.first_state, True)
            self.check()
            yield tick, before

    def check(self):
        sl, n = self.slots, self.n
        holds = np.repeat(sl.slot_state >= 0, n)
        assert sl.live[0] == holds.sum() // n and np.array_equal(sl.active, holds)
        assert (sl.rows[holds] >= self.first_state * n).all() and (sl.rows[~holds] == -1).all()
        assert (sl.uniforms[holds] < 1).all()

    def check_end(self):
        assert 0 < self.slots.head[0] <= self.N
        assert (self.out.best_nnz != 77).any() and (self.out.tokens[self.out.solved_step == 77] == 77).all()


def check_key_crossing(sl, n, first_state):
    """The rows the first refill of KEY_CASE fills lie on both sides of 2^32, and their uniforms are the sampling rule at
    the key's LOW word (include/tensor_game_net.h), computed here without ``SR.refill``: returns them, float32
    (B,1,3S)."""
    from net_ref import philox_uniforms
    rows = sl.rows
    assert (rows >= 0).all() and rows.min() == first_state * n and rows.min() < 2 ** 32 <= rows.max()
    assert (rows < 2 ** 32).sum() >= n and (rows >= 2 ** 32).sum() >= n
    assert (sl.slot_step == 0).all()
    u = philox_uniforms(REFILL_SEED, rows, 0, 1, 3 * sl.S)
    low = philox_uniforms(REFILL_SEED, rows % 2 ** 32, 0, 1, 3 * sl.S)
    assert np.array_equal(u, low) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    return u.astype(np.float32)
