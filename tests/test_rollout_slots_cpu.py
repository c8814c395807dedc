"""CPU checks of the solution search over a queue of start states: the C ABI of include/tensor_game_rollout_slots.h
(declared, bound, exported; the host checks of both entries through ctypes, in their order), the property that makes
the feature checkable -- per start state the refilled search finds exactly what the chunked one finds, for every number
of slots -- between the numpy restatements (tests/rollout_slots_ref.py) on the recorded factorisations, what the case
tables of the GPU tests (tests/rollout_slots_cases.py) are there for, and the argument errors of solve_stream."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib

import rollout_ref as R
import rollout_slots_cases as CS
import rollout_slots_ref as SR
from rollout_ref import demo_cases, strassen_scripts

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "tensor_game_rollout_slots.h"
ENTRIES = ["tg_rollout_advance_slots", "tg_rollout_refill"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_slot_entries_are_declared_bound_and_exported():
    text = HEADER.read_text()
    syms = re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", text, flags=re.M)
    assert syms == ENTRIES == sorted(_lib.ROLLOUT_SLOTS_SIGNATURES)
    assert re.findall(r"^#define\s+(TG_\w+)\s+(\d+)", text, flags=re.M) == [("TG_ROLLOUT_MAX_SLOTS", "65536")]
    assert _lib.TG_ROLLOUT_MAX_SLOTS == 65536
    # the masked entry's arguments with (slot_state, slot_step) in place of the host step
    masked = _lib.ROLLOUT_MASKED_SIGNATURES["tg_rollout_advance_masked"]
    assert masked[16] is C.c_int                                   # step
    assert _lib.ROLLOUT_SLOTS_SIGNATURES["tg_rollout_advance_slots"] == masked[:11] + [C.c_void_p] * 2 + masked[11:16] + \
        masked[17:]
    assert len(_lib.ROLLOUT_SLOTS_SIGNATURES["tg_rollout_refill"]) == 35
    from mat_mul_amd import build
    assert HEADER in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        for name in ENTRIES:
            assert hasattr(C.CDLL(str(path)), name), (path, name)
    assert _lib.lib.tg_abi_version() == _lib.TG_ABI_VERSION == 4   # additive: the version stays


P = C.c_void_p(64)   # never dereferenced: every call that gets this far is refused before any launch
ODD = C.c_void_p(66)
MAX_R = 65536


def test_advance_slots_host_checks_in_order():
    lib = _lib.lib

    def adv(frames=P, tokens=P, scalars=P, nnz=P, overflow=P, best=P, hits=P, sstep=P, ssample=P, actions=P, active=P,
            slot_state=P, slot_step=P, B=8, n=4, S=4, T=2, dim_s=1, max_actions=4, shift=1):
        return lib.tg_rollout_advance_slots(frames, tokens, scalars, nnz, overflow, best, hits, sstep, ssample, actions,
                                            active, slot_state, slot_step, B, n, S, T, dim_s, max_actions, shift, None)

    for bad, word in ((dict(S=0), b"S=0"), (dict(S=33), b"S=33"), (dict(T=0), b"T=0"), (dict(T=9), b"TG_NET_MAX_T"),
                      (dict(n=0), b"n=0"), (dict(n=65), b"TG_NET_MAX_SAMPLES"), (dict(B=9), b"multiple of n"),
                      (dict(B=-4), b"B=-4"), (dict(dim_s=-1), b"dim_s"), (dict(dim_s=65), b"dim_s"),
                      (dict(max_actions=0), b"max_actions=0"), (dict(max_actions=0, actions=None), b"max_actions=0"),
                      (dict(B=(MAX_R + 1) * 4), b"TG_ROLLOUT_MAX_SLOTS"), (dict(B=MAX_R + 1, n=1), b"TG_ROLLOUT_MAX_SLOTS"),
                      (dict(frames=None), b"null frames"), (dict(tokens=None), b"null tokens"),
                      (dict(nnz=None), b"null nnz"), (dict(best=None), b"group record"),
                      (dict(hits=None), b"group record"), (dict(sstep=None), b"group record"),
                      (dict(ssample=None), b"group record"), (dict(slot_state=None), b"null slot_state"),
                      (dict(slot_step=None), b"slot_step"), (dict(nnz=ODD), b"aligned"), (dict(scalars=ODD), b"aligned"),
                      (dict(slot_state=C.c_void_p(68)), b"slot_state must be 8-byte"),
                      (dict(slot_step=ODD), b"slot_step 4-byte")):
        assert adv(**bad) == -1, bad
        msg = lib.tg_last_error()
        assert word in msg and msg.startswith(b"tg_rollout_advance_slots:"), (bad, msg)
    # sizes, then pointers, then alignment: with everything wrong the first check speaks, and each one that is put right
    # hands over to the next
    wrong = dict(S=0, T=0, n=0, B=-3, dim_s=-1, max_actions=0, frames=None, tokens=None, nnz=None, best=None,
                 slot_state=None, scalars=ODD, slot_step=ODD)
    for fix, word in ((dict(S=4), b"S=0"), (dict(T=2), b"T=0"), (dict(n=1), b"n=0"), (dict(B=MAX_R + 1), b"B=-3"),
                      (dict(dim_s=1), b"dim_s=-1"), (dict(max_actions=6), b"max_actions=0"),
                      (dict(B=8), b"TG_ROLLOUT_MAX_SLOTS"), (dict(frames=P), b"null frames"),
                      (dict(tokens=P), b"null tokens"), (dict(nnz=P), b"null nnz"), (dict(best=P), b"group record"),
                      (dict(slot_state=P), b"null slot_state"), (dict(scalars=P), b"must be 4-byte aligned"),
                      (dict(slot_step=P), b"slot_step 4-byte")):
        assert adv(**wrong) == -1
        assert word in lib.tg_last_error(), (fix, lib.tg_last_error())
        wrong.update(fix)
    assert adv(B=MAX_R, n=1, frames=None) == -1 and b"null frames" in lib.tg_last_error()   # the maximum passes the sizes
    # B = 0 returns 0 at once, with or without pointers; the sizes are still checked
    assert adv(B=0) == 0
    assert adv(B=0, frames=None, tokens=None, nnz=None, best=None, hits=None, sstep=None, ssample=None, active=None,
               slot_state=None, slot_step=None, actions=None) == 0
    assert adv(B=0, S=0) == -1 and adv(B=0, max_actions=0) == -1
    # NULL actions and NULL active are not among the refusals
    assert adv(actions=None, active=None, nnz=None) == -1 and b"null nnz" in lib.tg_last_error()


def test_refill_host_checks_in_order():
    lib = _lib.lib
    names = ("q_states", "q_scalars", "N", "head", "first_state", "seed", "n_uniforms", "frames", "scalars", "nnz",
             "overflow", "best", "hits", "sstep", "ssample", "actions", "active", "slot_state", "slot_step", "o_best",
             "o_hits", "o_sstep", "o_ssample", "o_overflow", "o_tokens", "rows", "uniforms", "live", "B", "n", "S", "T",
             "dim_s", "max_actions")
    sizes = dict(N=10, first_state=0, seed=1, n_uniforms=12, B=8, n=4, S=4, T=2, dim_s=1, max_actions=4)

    def refill(**kw):
        args = {k: sizes.get(k, P) for k in names}
        args.update(kw)
        return lib.tg_rollout_refill(*[args[k] for k in names], None)

    for bad, word in ((dict(S=0), b"S=0"), (dict(S=33), b"S=33"), (dict(T=0), b"T=0"), (dict(T=9), b"TG_NET_MAX_T"),
                      (dict(n=0), b"n=0"), (dict(n=65), b"TG_NET_MAX_SAMPLES"), (dict(B=9), b"multiple of n"),
                      (dict(B=-4), b"B=-4"), (dict(dim_s=-1), b"dim_s"), (dict(max_actions=0), b"max_actions=0"),
                      (dict(B=(MAX_R + 1) * 4), b"TG_ROLLOUT_MAX_SLOTS"), (dict(N=-1), b"N=-1"),
                      (dict(first_state=-2), b"first_state=-2"), (dict(n_uniforms=11), b"n_uniforms=11"),
                      (dict(q_states=None), b"null q_states"), (dict(q_scalars=None), b"null q_scalars"),
                      (dict(head=None), b"null head"), (dict(frames=None), b"null frames"), (dict(nnz=None), b"null nnz"),
                      (dict(overflow=None), b"null overflow"), (dict(best=None), b"group record"),
                      (dict(ssample=None), b"group record"), (dict(actions=None), b"null actions"),
                      (dict(slot_state=None), b"null slot_state"), (dict(slot_step=None), b"slot_step"),
                      (dict(o_best=None), b"null output"), (dict(o_overflow=None), b"null output"),
                      (dict(o_tokens=None), b"null output"), (dict(rows=None), b"null rows"),
                      (dict(live=None), b"null live"), (dict(nnz=ODD), b"4-byte aligned"),
                      (dict(q_scalars=ODD), b"4-byte aligned"), (dict(head=C.c_void_p(68)), b"8-byte"),
                      (dict(rows=C.c_void_p(68)), b"8-byte"), (dict(live=ODD), b"live 4-byte"),
                      (dict(o_hits=ODD), b"int32 outputs"), (dict(uniforms=ODD), b"uniforms must be 4-byte")):
        assert refill(**bad) == -1, bad
        msg = lib.tg_last_error()
        assert word in msg and msg.startswith(b"tg_rollout_refill:"), (bad, msg)
    wrong = dict(S=0, n=0, B=-3, max_actions=0, N=-5, first_state=-1, n_uniforms=3, q_states=None, head=None, frames=None,
                 rows=None, nnz=ODD, live=ODD)
    for fix, word in ((dict(S=4), b"S=0"), (dict(n=4), b"n=0"), (dict(B=8), b"B=-3"), (dict(max_actions=3), b"max_actions=0"),
                      (dict(N=7), b"N=-5"), (dict(first_state=3), b"first_state=-1"), (dict(n_uniforms=12), b"n_uniforms=3"),
                      (dict(q_states=P), b"null q_states"), (dict(head=P), b"null head"), (dict(frames=P), b"null frames"),
                      (dict(rows=P), b"null rows"), (dict(nnz=P), b"must be 4-byte aligned"),
                      (dict(live=P), b"live 4-byte")):
        assert refill(**wrong) == -1
        assert word in lib.tg_last_error(), (fix, lib.tg_last_error())
        wrong.update(fix)
    # B = 0 and N = 0 return 0 at once, with or without pointers; the sizes are still checked
    every = {k: None for k in names if k not in sizes}
    assert refill(B=0) == 0 and refill(N=0) == 0
    assert refill(B=0, **every) == 0 and refill(N=0, **every) == 0
    assert refill(B=0, S=0) == -1 and refill(N=0, max_actions=0) == -1
    # NULL uniforms (then n_uniforms is ignored), NULL active and NULL scalars with NULL q_scalars are accepted
    assert refill(uniforms=None, n_uniforms=0, active=None, scalars=None, q_scalars=None, live=None) == -1
    assert b"null live" in lib.tg_last_error()


# ---- the restatements against each other on recorded data -----------------------------------------------------------
def strassen_subset(golden, shift, n, slot):
    """Every third recorded Strassen state, every fifth of them with a script that never ends, as a (row, step) table."""
    states, scripts, lengths = strassen_scripts(golden, shift)
    states, scripts, lengths = states[::3], scripts[::3], lengths[::3]
    stuck = np.arange(len(scripts)) % 5 == 4
    scripts = [[R.null_action(4, shift)] if s else sc for s, sc in zip(stuck, scripts)]
    K = 9
    return states, SR.scripted_table(scripts, 4, n, slot, shift, K, seed=5), K, stuck, lengths


@pytest.mark.parametrize("shift,n,slot", [(1, 1, 0), (2, 1, 0), (1, 4, 2), (2, 4, 1)])
def test_property_on_the_strassen_states(golden, shift, n, slot):
    states, table, K, stuck, lengths = strassen_subset(golden, shift, n, slot)
    G = len(states)
    scal = np.arange(G, dtype=np.float32)[:, None]
    stream_pol, chunk_pol = SR.keyed_table_policy(table, n)
    want = SR.solve_states(chunk_pol, states, scal, n, K, shift)
    steps = want.solved_step
    assert len(set(steps[steps >= 0])) >= 2 and (steps < 0).any()       # what the subset is for
    if n == 1:
        assert np.array_equal(steps >= 0, ~stuck) and np.array_equal(steps[~stuck], lengths[~stuck] - 1)
    ticks = {}
    for R_ in (1, 5, G, G + 3):
        got = SR.solve_stream(stream_pol, states, scal, n, K, R_, shift)
        SR.check_equal(got, want)
        assert np.array_equal(got.overflow, want.overflow)
        assert got.ticks <= SR.bound(G, R_, K), (R_, got.ticks)
        ticks[R_] = got.ticks
    assert ticks[G] == ticks[G + 3] == K                                # an unsolved state takes every step
    assert ticks[1] == int(np.where(steps >= 0, steps + 1, K).sum())    # one slot: the states one after another
    for g, tok, L in zip(want.groups, want.tokens, want.lengths):
        assert not R.O.take_actions(list(tok[:L]), states[g, 0], shift).any()


def test_first_state_offsets_join_to_the_whole(golden):
    states, table, K, _, _ = strassen_subset(golden, 1, 4, 2)
    G, n, h = len(states), 4, len(states) // 2
    scal = np.zeros((G, 1), np.float32)
    stream_pol, _ = SR.keyed_table_policy(table, n)
    whole = SR.solve_stream(stream_pol, states, scal, n, K, 7)
    a = SR.solve_stream(stream_pol, states[:h], scal[:h], n, K, 7)
    b = SR.solve_stream(stream_pol, states[h:], scal[h:], n, K, 7, first_state=h)
    for name in ("best_nnz", "hits", "solved_step", "solved_sample", "overflow"):
        assert np.array_equal(np.concatenate([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    assert np.array_equal(np.concatenate([a.groups, b.groups + h]), whole.groups)
    assert np.array_equal(np.concatenate([a.tokens, b.tokens]), whole.tokens)


def test_property_on_the_recorded_demonstrations(golden):
    for name, target, script in demo_cases(golden):
        S, K, T, n = target.shape[-1], len(script) + 2, 2, 4
        states = np.zeros((3, T, S, S, S), np.int8)
        states[:, 0] = target[:, 0]
        states[1, 0, 0, 0, 0] += 1              # one entry off: the same script leaves this state unsolved
        table = SR.scripted_table([script] * 3, S, n, 2, 1, K, seed=3)
        stream_pol, chunk_pol = SR.keyed_table_policy(table, n)
        scal = np.arange(3, dtype=np.float32)[:, None]
        want = SR.solve_states(chunk_pol, states, scal, n, K, 1)
        assert want.solved_step[0] >= 0 and want.solved_step[1] < 0, name
        for R_ in (1, 2, 3, 5):
            got = SR.solve_stream(stream_pol, states, scal, n, K, R_, 1)
            SR.check_equal(got, want)
            assert got.ticks <= SR.bound(3, R_, K)


def test_restated_uniforms_follow_the_sampling_rule():
    from net_ref import philox_uniforms
    sl, out = SR.Slots(3, 2, 4, 1, 1, 5), SR.Out(2, 4, 5)
    SR.refill(sl, out, np.zeros((2, 1, 4, 4, 4), np.int8), np.zeros((2, 1), np.float32), seed=9, first_state=100)
    assert list(sl.rows) == [200, 201, 202, 203, -1, -1] and list(sl.active) == [1, 1, 1, 1, 0, 0]
    assert sl.live[0] == 2 and sl.head[0] == 2 and list(sl.slot_state) == [0, 1, -1]
    assert np.array_equal(sl.uniforms[:4], philox_uniforms(9, np.arange(200, 204), 0, 1, 12).astype(np.float32))
    assert not sl.uniforms[4:].any()


# ---- the case tables of the GPU tests, through the restatement alone (tests/rollout_slots_cases.py) -------------------
@pytest.mark.parametrize("S,T,n,R_,misalign", CS.ADVANCE_CASES + CS.SIZE_CASES)
def test_advance_cases_meet_all_six_kinds(S, T, n, R_, misalign):
    rng = np.random.default_rng(1000 * S + 10 * n + R_)
    seen = set()
    for rot, kinds, sl, tokens in CS.advance_launches(S, T, n, R_, rng):
        seen |= set(kinds.tolist())
        before = sl.copy()
        SR.advance_slots(sl, tokens, 1)
        CS.check_advance(kinds, n, before, sl)
        assert (tokens[np.repeat(kinds < CS.LIVE0, n)] == 127).all()
    assert seen == set(range(6))
    gpw = CS.groups_per_workgroup(S, n, R_, misalign)
    if (S, T, n, R_, misalign) in CS.WIDE_CASES:
        assert gpw > 64 and R_ > gpw and R_ % gpw           # several scan passes, a partial last workgroup
    else:
        assert gpw <= 64


def test_planted_case_has_its_live_slots_behind_200_dead_ones():
    S, T, n, R_, misalign = CS.PLANTED_CASE
    assert CS.groups_per_workgroup(S, n, R_, misalign) == R_ == 256       # one workgroup, four scan passes
    kinds = CS.planted_kinds()
    assert (kinds[:200] < CS.LIVE0).all() and (kinds[200:] >= CS.LIVE0).all() and set(kinds.tolist()) == set(range(6))
    sl, tokens = CS.advance_inputs(S, T, n, kinds, np.random.default_rng(256))
    before = sl.copy()
    SR.advance_slots(sl, tokens, 1)
    CS.check_advance(kinds, n, before, sl)
    for name in SR.ROW_FIELDS + SR.SLOT_FIELDS:
        assert np.array_equal(getattr(sl, name)[:200], getattr(before, name)[:200]), name


@pytest.mark.parametrize("S,T,n,R_", CS.OVERFLOW_CASES)
def test_overflow_cases_flag_some_live_rows_and_not_others(S, T, n, R_):
    sl, tokens, q_states, q_scalars = CS.overflow_inputs(S, T, n, R_, np.random.default_rng(S + R_))
    before = sl.copy()
    SR.advance_slots(sl, tokens, CS.OVERFLOW_SHIFT)
    CS.check_overflow_step(n, before, sl, tokens)
    stepped, out = sl.copy(), SR.Out(len(q_states), S, 1, fill=77)
    SR.refill(sl, out, q_states, q_scalars, 5, 0, True)
    CS.check_overflow_flush(n, stepped, sl, out)


# the new cases whose queue runs dry inside a tick that still has states to hand out: on the 16-byte path at S = 16 and
# S = 32, on the dword path without a tail, and on the dword path with a tail at S = 25
DRY_CASES = {(16, 2, 8, 5, 12, 3, 1, 0), (16, 1, 2, 4, 9, 2, 0, 4), (32, 1, 64, 2, 5, 2, 0, 0), (25, 1, 4, 3, 7, 2, 0, 0)}
assert DRY_CASES <= set(CS.REFILL_SIZE_CASES)


@pytest.mark.parametrize("case", [c for c in CS.REFILL_CASES + CS.REFILL_SIZE_CASES if c[3] <= 100])
def test_refill_cases_run_dry_and_cross_the_key_word(case):
    S, T, n, R_, N, K, first_state, misalign = case
    run = CS.RefillRun(*case)
    for tick, before in run.ticks():
        if case == CS.KEY_CASE and tick == 0:                # the row keys cross 2^32 inside the first tick
            want = CS.check_key_crossing(run.slots, n, first_state)
            assert np.array_equal(run.slots.uniforms, want)
    run.check_end()
    if case in DRY_CASES or (R_, N) == (65, 100):
        assert run.dry


def test_refill_size_cases_have_every_tail():
    tails = sorted(T * S ** 3 % 4 for S, T, *_ in CS.REFILL_SIZE_CASES if S == 25)
    assert tails == [1, 2, 3]                               # bytes behind the last whole dword of a row
    assert any(S % 4 == 0 and mis % 16 for S, *_, mis in CS.REFILL_SIZE_CASES)
    assert any(S % 4 == 0 and mis % 16 for S, *_, mis in CS.SIZE_CASES)


# ---- Python argument errors (no device) -------------------------------------------------------------------------------
def test_solve_stream_argument_errors():
    import torch
    import mat_mul_amd
    from mat_mul_amd import TensorGameError, rollout
    assert mat_mul_amd.solve_stream is rollout.solve_stream and "solve_stream" in mat_mul_amd.__all__
    states, scal = torch.zeros((2, 1, 4, 4, 4), dtype=torch.int8), torch.zeros((2, 1))
    policy = lambda *a, **k: None  # noqa: E731
    with pytest.raises(TensorGameError, match="no CPU path"):          # the device check comes first
        rollout.solve_stream(policy, states, scal, 4, 3, slots=0, check_every=-1)
    with pytest.raises(TensorGameError, match="slots=0 < 1"):
        rollout.solve_stream(policy, _Cuda(states), _Cuda(scal), 4, 3, slots=0)
    with pytest.raises(TensorGameError, match="check_every=-1"):
        rollout.solve_stream(policy, _Cuda(states), _Cuda(scal), 4, 3, slots=2, check_every=-1)
    with pytest.raises(TensorGameError, match="first_state=-8"):
        rollout.solve_stream(policy, _Cuda(states), _Cuda(scal), 4, 3, slots=2, first_state=-8)
    with pytest.raises(TensorGameError, match="max_actions=0"):
        rollout.solve_stream(policy, _Cuda(states), _Cuda(scal), 4, 0, slots=2)
    with pytest.raises(TensorGameError, match="int8"):
        rollout.solve_stream(policy, _Cuda(states.float()), _Cuda(scal), 4, 3, slots=2)
    with pytest.raises(TensorGameError, match="scalars must be float32"):
        rollout.solve_stream(policy, _Cuda(states), _Cuda(scal[:1]), 4, 3, slots=2)
    res = rollout.SolveResult(*([None] * 8))
    assert res.overflow is None and res.ticks == 0                     # the new fields come last, with defaults


class _Cuda:
    """A tensor that says it lives on a ROCm device, for the checks that solve_stream makes before it touches one."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    @property
    def device(self):
        import torch
        return torch.device("cuda:0")

    def __getattr__(self, name):
        return getattr(self._t, name)
