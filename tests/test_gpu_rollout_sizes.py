"""GPU checks of the solution search at the sizes its first tests left out (tg_rollout_advance_slots, tg_rollout_refill,
``sample_rollouts(stop_solved=True)``, ``solve_states``, ``solve_stream``): the slot step at S = 25 and S = 32, on the
dword path without a tail, and with more than 64 groups per workgroup in more than one workgroup; overflow produced by
the slot step itself and flushed by the refill; the refill at S = 16, 25 and 32 and with row keys beyond 2^32; and the
fused networks of the 4x4 and the 5x5 tensor (their sliced torsos and decoders, row-masked by the search's ``active``
bytes and sampled from the refill's uniforms) inside the search.  Everything is bit for bit against the restatements of
tests/rollout_slots_ref.py and tests/rollout_masked_ref.py; the case tables are tests/rollout_slots_cases.py's, which
test_rollout_slots_cpu.py checks without a GPU."""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedAlphaTensor25, ops, rollout

import rollout_masked_ref as M
import rollout_slots_cases as C
import rollout_slots_ref as SR
from net_s16_ref import CONFIGS as CONFIGS_S16
from net_s25_ref import CONFIGS as CONFIGS_S25
from test_gpu_rollout_masked import same
from test_gpu_rollout_slots import (DEV, SLOT_BUFFERS, check_guards, dev, fused_setup, guarded_from, host, run_advance,
                                    run_refill, same_result, same_slots, slot_field)

pytestmark = pytest.mark.gpu


# ---- the step against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,n,R_,misalign", C.SIZE_CASES)
def test_advance_slots_at_more_sizes(S, T, n, R_, misalign):
    """rollout_slots_cases.SIZE_CASES (the table names the path each case is the first to reach), as
    test_advance_slots_equals_the_restatement runs its cases: every buffer guarded, the tokens of the rows that are not
    live poisoned, all six kinds of slot met."""
    if (S, T, n, R_, misalign) in C.WIDE_CASES:          # a change of the constants must not turn them into small cases
        gpw = C.groups_per_workgroup(S, n, R_, misalign)
        assert gpw > 64 and R_ > gpw and R_ % gpw
    rng = np.random.default_rng(1000 * S + 10 * n + R_)
    seen = set()
    for rot, kinds, sl, tokens in C.advance_launches(S, T, n, R_, rng):
        seen |= set(kinds.tolist())
        before = sl.copy()
        run_advance(sl, tokens, misalign, 1, rot)
        C.check_advance(kinds, n, before, sl)
    assert seen == set(range(6))


def test_advance_slots_goes_on_past_dead_slots():
    """One workgroup of 256 one-row groups whose slots 0 .. 199 are empty, solved or exhausted: the first three passes
    of the 64-wide scan find nothing to do and the workgroup must still go on for the live slots 200 .. 255, whose
    activity and step index sit in s_act / s_step beyond 64.  The live ones are stepped, the others byte-identical."""
    S, T, n, R_, misalign = C.PLANTED_CASE
    assert C.groups_per_workgroup(S, n, R_, misalign) == R_ == 256
    kinds = C.planted_kinds()
    assert (kinds[:200] < C.LIVE0).all() and (kinds[200:] >= C.LIVE0).all() and set(kinds.tolist()) == set(range(6))
    sl, tokens = C.advance_inputs(S, T, n, kinds, np.random.default_rng(256))
    before = sl.copy()
    bufs, ds = run_advance(sl, tokens, misalign, 1, "planted")
    C.check_advance(kinds, n, before, sl)
    live = np.repeat(kinds >= C.LIVE0, n)
    assert (host(ds.frames)[live] != before.frames[live]).any(axis=(1, 2, 3, 4)).sum() > live.sum() // 2
    assert np.array_equal(host(ds.slot_step)[200:], before.slot_step[200:] + 1)
    for name in SLOT_BUFFERS:
        if name in ("head", "live"):
            continue
        got, was = host(slot_field(ds, name)), getattr(before, name)
        dead = ~live if len(was) == R_ * n else kinds < C.LIVE0
        assert np.array_equal(got[dead], was[dead]), name


# ---- overflow in slot mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,n,R_", C.OVERFLOW_CASES)
def test_overflow_of_the_slot_step_reaches_the_outputs(S, T, n, R_):
    """rollout_slots_cases.overflow_inputs at shift 2: the slot step itself takes head entries of 127 and -128 out of
    int8 on the even rows of the live slots (wrapped as tg_step_i8 wraps, ``overflow`` set) and on no other row, the
    same values on the slots that are not live stay as they are, unflagged; then one refill (max_actions = 1: every
    stepped slot is finished) writes the OR of a slot's flags to its state's out_overflow and clears the slot's."""
    sl, tokens, q_states, q_scalars = C.overflow_inputs(S, T, n, R_, np.random.default_rng(S + R_))
    before = sl.copy()
    bufs, ds = run_advance(sl, tokens, 0, C.OVERFLOW_SHIFT, "overflow")
    C.check_overflow_step(n, before, sl, tokens)
    stepped, out = sl.copy(), SR.Out(len(q_states), S, 1, fill=77)
    out_bufs, d_out = zip(*[guarded_from(getattr(out, name)) for name in SR.OUT_FIELDS])
    SR.refill(sl, out, q_states, q_scalars, 5, 0, True)
    ops.rollout_refill(ds, dev(q_states), dev(q_scalars), d_out, seed=5, first_state=0)
    same_slots(ds, sl, "flush")
    for name, t, buf in zip(SR.OUT_FIELDS, d_out, out_bufs):
        assert np.array_equal(host(t), getattr(out, name)), name
        check_guards(buf, 0, name)
    for name, buf in bufs.items():
        check_guards(buf, 0, name)
    C.check_overflow_flush(n, stepped, sl, out)


# ---- the refill against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,n,R_,N,K,first_state,misalign", C.REFILL_SIZE_CASES)
def test_refill_at_more_sizes(S, T, n, R_, N, K, first_state, misalign):
    """rollout_slots_cases.REFILL_SIZE_CASES (the table names the path each case is the first to reach), through the
    three ticks of test_refill_equals_the_restatement.  KEY_CASE: the row keys cross 2^32 inside the first tick, and the
    uniforms on both sides of the crossing are the sampling rule at the key's low word, computed without SR.refill."""
    case = (S, T, n, R_, N, K, first_state, misalign)
    crossed = []

    def after_tick(tick, ds, run):
        if case == C.KEY_CASE and tick == 0:
            want = C.check_key_crossing(run.slots, n, first_state)
            assert np.array_equal(host(ds.rows), run.slots.rows) and np.array_equal(host(ds.uniforms), want)
            crossed.append(tick)

    run_refill(*case, after_tick=after_tick)
    assert crossed == ([0] if case == C.KEY_CASE else [])


# ---- the fused networks of the 4x4 and the 5x5 tensor in the search -------------------------------------------------
NETS = {"b16": (CONFIGS_S16, FusedAlphaTensor), "c25": (CONFIGS_S25, FusedAlphaTensor25),
        "a16": (CONFIGS_S16, FusedAlphaTensor), "a25": (CONFIGS_S25, FusedAlphaTensor25)}
SMALL = ("b16", "c25")          # n_steps = 3 * dim_3d, n_logits = 3, a few layers
SEED, G, N_SAMPLES, K = 11, 9, 4, 3


@functools.lru_cache(maxsize=None)
def search_case(name):
    """(network, states, scalars, what solve_states finds in one chunk with the masked policy), computed once.  At b16
    and c25 the start states must exercise both halves of every property below: some solved, some not -- decided here,
    by the solve_states run, not by the code under test."""
    configs, cls = NETS[name]
    small = name in SMALL
    g, k = (G, K) if small else (3, 2)
    net, states, scalars = fused_setup(name, g, configs, cls)
    want = rollout.solve_states(net.rollout_policy(SEED, masked=True), states, scalars, N_SAMPLES, k, chunk_groups=g)
    steps = host(want.solved_step)
    print(name, "seed", SEED, "solved_step", steps.tolist())
    if small:
        assert (steps >= 0).any() and (steps < 0).any()
    return net, states, scalars, k, want


@pytest.mark.parametrize("name", SMALL)
def test_fused_masked_policy_at_s16_and_s25(name):
    """``rollout_policy(masked=True)`` under ``sample_rollouts(stop_solved=True)`` at S = 16 (FusedAlphaTensor: S torso
    workgroups per game) and S = 25 (FusedAlphaTensor25: one per game and slice, the shared-normalisation decoder), both
    row-masked by ``active`` into a persistent ee buffer: test_fused_masked_policy's checks at G = 9, n = 4, K = 3.
    Bias 3.0 on the zero factor's token (fused_setup's) and seed 11 give, on an MI355X, solved_step
    [0, -1, -1, 0, -1, -1, -1, -1, -1] at b16 (the zero state 6 comes within two entries, best_nnz 2, and stays unsolved)
    and [0, -1, -1, 0, -1, -1, 0, -1, -1] at c25; a16 and a25 (G = 3, K = 2) give [0, -1, -1]."""
    net, states, scalars, k, want = search_case(name)
    n = N_SAMPLES
    plain = rollout.sample_rollouts(net.rollout_policy(seed=SEED), states, scalars, n, k)
    pol = net.rollout_policy(seed=SEED, masked=True)
    assert pol.takes_active
    a = rollout.sample_rollouts(pol, states, scalars, n, k, stop_solved=True)
    n_solved, n_unsolved = M.check_property(a, plain, get=host)
    assert n_solved >= 1 and n_unsolved >= 1      # decided by the plain run: both halves of the property are exercised
    for x, y in zip(a.solutions(), plain.solutions()):
        assert torch.equal(x, y)
    # two runs are equal, and a fresh policy of the same seed plays the same games; another seed plays others
    same(rollout.sample_rollouts(pol, states, scalars, n, k, stop_solved=True), a)
    same(rollout.sample_rollouts(net.rollout_policy(seed=SEED, masked=True), states, scalars, n, k, stop_solved=True), a)
    c = rollout.sample_rollouts(net.rollout_policy(seed=SEED + 1, masked=True), states, scalars, n, k, stop_solved=True)
    assert not torch.equal(a.actions, c.actions)
    # graph=True equals eager bit for bit
    g = rollout.sample_rollouts(net.rollout_policy(seed=SEED, masked=True), states, scalars, n, k, stop_solved=True,
                                graph=True)
    torch.cuda.synchronize()
    same(g, a)
    assert g.graph is not None and a.graph is None
    # inactive rows of the token buffer keep what they held
    B = states.shape[0] * n
    frames = states.repeat_interleave(n, 0).contiguous()
    rows = torch.arange(B, device=DEV)
    active = (rows % 2).to(torch.uint8)
    out = torch.full((B, net.n_steps), 99, dtype=torch.int8, device=DEV)
    assert pol(frames, scalars.repeat_interleave(n, 0), rows, 0, active=active, out=out) is out
    assert bool((out[::2] == 99).all()) and torch.equal(out[1::2], a.actions[1::2, 0])
    # the dataset loop with the masked policy: the chunking does not show
    parts = rollout.solve_states(pol, states, scalars, n, k, chunk_groups=4)
    same(want, a, M.RECORDS)
    same(parts, a, M.RECORDS)
    for x, y, z in zip((parts.groups, parts.tokens, parts.lengths), (want.groups, want.tokens, want.lengths),
                       a.solutions()):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("name", SMALL)
def test_fused_slot_policy_at_s16_and_s25(name):
    """``slot_policy`` under ``solve_stream`` at S = 16 and S = 25: the masked torso and decoder of those sizes sampled
    from the uniforms tg_rollout_refill writes (48 per row: 12 Philox quads; 75 per row: 18 quads and three words of the
    19th), for 1, 4 and 10 slots (fewer than, and more than, the 9 states) and both ways of reading ``live``: every
    field equals what ``solve_states`` finds, in no more ticks than the bound.  The start states and their
    solved_step are test_fused_masked_policy_at_s16_and_s25's."""
    net, states, scalars, k, want = search_case(name)
    n, g = N_SAMPLES, states.shape[0]
    pol = net.slot_policy(SEED)
    assert pol.takes_slots and pol.seed == SEED
    for R_ in (1, 4, 10):
        for m in (1, 2):
            got = rollout.solve_stream(net.slot_policy(SEED), states, scalars, n, k, slots=R_, check_every=m)
            same_result(got, want)
            assert 0 < got.ticks <= SR.bound(g, R_, k) and not bool(got.overflow.any())
    same_result(rollout.solve_stream(pol, states, scalars, n, k, slots=4, check_every=2, graph=True), want)
    other = rollout.solve_stream(net.slot_policy(SEED + 1), states, scalars, n, k, slots=4)
    assert not all(torch.equal(getattr(other, f), getattr(want, f)) for f in ("best_nnz", "solved_step", "tokens"))


@pytest.mark.parametrize("name", SMALL)
def test_fused_slot_policy_halves_join_to_the_whole(name):
    """The two halves of the dataset, the second with ``first_state`` = its offset, concatenated equal the whole: the
    row keys of the refill, not the position in the run, decide what the networks of S = 16 and S = 25 draw."""
    net, states, scalars, k, want = search_case(name)
    n, h = N_SAMPLES, states.shape[0] // 2
    whole = rollout.solve_stream(net.slot_policy(SEED), states, scalars, n, k, slots=4)
    a = rollout.solve_stream(net.slot_policy(SEED), states[:h], scalars[:h], n, k, slots=4)
    b = rollout.solve_stream(net.slot_policy(SEED), states[h:], scalars[h:], n, k, slots=4, first_state=h)
    for name_ in ("best_nnz", "hits", "solved_step", "solved_sample", "overflow", "tokens", "lengths"):
        assert torch.equal(torch.cat([getattr(a, name_), getattr(b, name_)]), getattr(whole, name_)), name_
    assert torch.equal(torch.cat([a.groups, b.groups + h]), whole.groups)
    same_result(whole, want)


@pytest.mark.parametrize("name", ("a16", "a25"))
def test_training_app_networks_in_the_slot_search(name):
    """The training app's configuration at S = 16 and S = 25 (eight torso layers, T = 2, one decoder row per workgroup at
    S = 25) once through ``solve_stream`` with fewer slots than states: equal to ``solve_states``.  G = 3, n = 4, K = 2,
    the size of test_sampled_rollouts_with_the_fused_network_at_s25."""
    net, states, scalars, k, want = search_case(name)
    got = rollout.solve_stream(net.slot_policy(SEED), states, scalars, N_SAMPLES, k, slots=2, check_every=1)
    same_result(got, want)
    assert 0 < got.ticks <= SR.bound(states.shape[0], 2, k)
