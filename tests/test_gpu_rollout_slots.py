"""GPU checks of the solution search over a queue of start states (tg_rollout_advance_slots, tg_rollout_refill,
``solve_stream``, ``FusedAlphaTensor.slot_policy``): both entries bit for bit against the numpy restatement
(tests/rollout_slots_ref.py) with every buffer guarded, and the property that per start state the refilled search finds
exactly what ``solve_states`` finds, for every number of slots, with table policies and with the fused network."""
import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, ops, rollout

import rollout_ref as R
import rollout_slots_ref as SR
from guarded_buffers import CANARY, GUARD
from net_ref import CONFIGS as CONFIGS_S4, P, make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from rollout_ref import strassen_scripts
from rollout_slots_cases import ADVANCE_CASES, REFILL_CASES, REFILL_SEED, RefillRun, advance_launches, check_advance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NET_CONFIGS = {"a": CONFIGS_S4["a"], "a9": CONFIGS_S9["a9"]}
SLOT_BUFFERS = ("frames", "scalars", "nnz", "overflow", "active", "actions", "rows", "uniforms", "best_nnz", "hits",
                "solved_step", "solved_sample", "slot_state", "slot_step", "head", "live")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded_from(a, offset=0):
    """(buffer, device tensor equal to ``a``) with canary bytes around it; ``offset`` extra bytes in front misalign it."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    buf = torch.full((GUARD + offset + a.nbytes + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + a.nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return buf, view


def check_guards(buf, offset, what):
    assert bool((buf[:GUARD + offset] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all()), what


def device_slots(sl, misalign=0):
    """(guard buffers by name, ops.RolloutSlots) holding what the restatement's ``sl`` holds."""
    bufs, d = {}, {}
    for name in SLOT_BUFFERS:
        bufs[name], d[name] = guarded_from(getattr(sl, name), misalign if name == "frames" else 0)
    bufs["tokens"], d["tokens"] = guarded_from(np.zeros((len(sl.nnz), 3 * sl.S), np.int8))
    return bufs, ops.RolloutSlots(sl.n, sl.K, d["frames"], d["scalars"], d["nnz"], d["overflow"], d["active"],
                                  d["actions"], d["tokens"], d["rows"], d["uniforms"],
                                  (d["best_nnz"], d["hits"], d["solved_step"], d["solved_sample"]), d["slot_state"],
                                  d["slot_step"], d["head"], d["live"])


def slot_field(ds, name):
    return ds.records[SR.SLOT_FIELDS.index(name)] if name in SR.SLOT_FIELDS[:4] else getattr(ds, name)


def same_slots(ds, sl, what):
    for name in SLOT_BUFFERS:
        assert np.array_equal(host(slot_field(ds, name)), getattr(sl, name)), (name, what)


# ---- the step against the restatement -------------------------------------------------------------------------------
def run_advance(sl, tokens, misalign, shift, what):
    """One launch on guarded copies of ``sl`` and ``tokens`` beside the restatement (which steps ``sl`` in place): every
    slot buffer equal, the tokens as they were, no guard touched.  Returns the device slots and their guard buffers."""
    bufs, ds = device_slots(sl, misalign)
    buf_tok, d_tok = guarded_from(tokens)
    SR.advance_slots(sl, tokens, shift)
    ops.rollout_advance_slots(ds, d_tok, shift=shift)
    same_slots(ds, sl, what)
    assert np.array_equal(host(d_tok), tokens)
    for name, buf in (*bufs.items(), ("tokens in", buf_tok)):
        check_guards(buf, misalign if name == "frames" else 0, name)
    return bufs, ds


@pytest.mark.parametrize("S,T,n,R_,misalign", ADVANCE_CASES)
def test_advance_slots_equals_the_restatement(S, T, n, R_, misalign):
    rng = np.random.default_rng(1000 * S + 10 * n + R_)
    seen = set()
    for rot, kinds, sl, tokens in advance_launches(S, T, n, R_, rng):   # R < 6: as many launches as all six kinds take
        seen |= set(kinds.tolist())
        before = sl.copy()
        run_advance(sl, tokens, misalign, 1, rot)
        check_advance(kinds, n, before, sl)     # what the restatement must have done for the cases to mean anything
    assert seen == set(range(6))


# ---- the refill against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S,T,n,R_,N,K,first_state,misalign", REFILL_CASES)
def test_refill_equals_the_restatement(S, T, n, R_, N, K, first_state, misalign):
    run = run_refill(S, T, n, R_, N, K, first_state, misalign)
    if (R_, N) in ((65, 100), (9, 4)):
        assert run.dry or R_ > N                  # the queue ran dry inside a tick / could never fill the slots


def run_refill(S, T, n, R_, N, K, first_state, misalign, after_tick=None):
    """The three ticks of a refill case on the device beside the restatement's (rollout_slots_cases.RefillRun), every
    buffer guarded, then one refill without uniforms; ``after_tick(tick, device slots, run)`` sees every tick."""
    run = RefillRun(S, T, n, R_, N, K, first_state, misalign)
    sl, out, seed = run.slots, run.out, REFILL_SEED
    buf_qs, d_qs = guarded_from(run.q_states, misalign)
    buf_qc, d_qc = guarded_from(run.q_scalars)
    out_bufs, d_out = zip(*[guarded_from(getattr(out, name)) for name in SR.OUT_FIELDS])
    for tick, before in run.ticks():
        bufs, ds = device_slots(before, misalign)
        ops.rollout_refill(ds, d_qs, d_qc, d_out, seed=seed, first_state=first_state)
        same_slots(ds, sl, tick)
        for name, t in zip(SR.OUT_FIELDS, d_out):
            assert np.array_equal(host(t), getattr(out, name)), (name, tick)
        for name, buf in bufs.items():
            check_guards(buf, misalign if name == "frames" else 0, name)
        if after_tick:
            after_tick(tick, ds, run)
    for name, buf in (*zip(SR.OUT_FIELDS, out_bufs), ("q_states", buf_qs), ("q_scalars", buf_qc)):
        check_guards(buf, misalign if name == "q_states" else 0, name)
    assert np.array_equal(host(d_qs), run.q_states)
    run.check_end()
    # without uniforms: the same, and the uniforms stay as they are
    bufs, ds = device_slots(sl, misalign)
    ds.head.zero_()
    ds.slot_state.fill_(-1)
    sl.head[:], sl.slot_state[:] = 0, -1
    SR.refill(sl, out, run.q_states, run.q_scalars, seed, first_state, False)
    ops.rollout_refill(ds, d_qs, d_qc, d_out, seed=seed, first_state=first_state, uniforms=False)
    same_slots(ds, sl, "no uniforms")
    return run


# ---- table policies through solve_stream --------------------------------------------------------------------------------
def device_table_policies(table):
    """(stream policy, chunk policy) on the device that play table[row key, the row's own step]."""
    d_table = dev(table)
    K = table.shape[1]

    def stream(frames, scalars, rows, steps):
        return d_table[rows, steps.to(torch.int64).clamp(max=K - 1)]

    def chunk(frames, scalars, rows, step):
        return d_table[rows, step]

    return stream, chunk


_cache = {}


def strassen_case(golden, shift, n, slot):
    """The Strassen subset of test_rollout_slots_cpu.py, its table, and what solve_states finds (computed once)."""
    key = (shift, n, slot)
    if key not in _cache:
        states, scripts, lengths = strassen_scripts(golden, shift)
        states, scripts = states[::3], scripts[::3]
        stuck = np.arange(len(scripts)) % 5 == 4
        scripts = [[R.null_action(4, shift)] if s else sc for s, sc in zip(stuck, scripts)]
        K = 9
        table = SR.scripted_table(scripts, 4, n, slot, shift, K, seed=5)
        stream_pol, chunk_pol = device_table_policies(table)
        d_states = dev(states)
        scal = dev(np.arange(len(states), dtype=np.float32)[:, None])
        want = rollout.solve_states(chunk_pol, d_states, scal, n, K, chunk_groups=len(states), shift=shift)
        ref = SR.solve_states(SR.keyed_table_policy(table, n)[1], states, host(scal), n, K, shift)
        SR.check_equal(want, ref, get=lambda x: host(x) if torch.is_tensor(x) else x)
        steps = host(want.solved_step)
        assert len(set(steps[steps >= 0])) >= 2 and (steps < 0).any() and (steps >= 0).sum() >= 2
        _cache[key] = (d_states, scal, K, stream_pol, want, ref)
    return _cache[key]


def same_result(got, want):
    for name in SR.RESULT_FIELDS:
        assert torch.equal(getattr(got, name), getattr(want, name)), name


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("shift,n,slot", [(1, 1, 0), (2, 4, 1)])
def test_solve_stream_equals_solve_states(golden, shift, n, slot, graph):
    d_states, scal, K, pol, want, ref = strassen_case(golden, shift, n, slot)
    G = d_states.shape[0]
    for R_ in (1, 3, G, G + 5):
        for m in (1, 4):
            got = rollout.solve_stream(pol, d_states, scal, n, K, slots=R_, check_every=m, shift=shift, graph=graph)
            same_result(got, want)
            assert np.array_equal(host(got.overflow), ref.overflow)
            assert 0 < got.ticks <= SR.bound(G, R_, K) and got.steps_run == (got.ticks,)
    whole = rollout.solve_stream(pol, d_states, scal, n, K, slots=7, shift=shift, graph=graph)
    h = G // 2
    a = rollout.solve_stream(pol, d_states[:h], scal[:h], n, K, slots=7, shift=shift, graph=graph)
    b = rollout.solve_stream(pol, d_states[h:], scal[h:], n, K, slots=7, shift=shift, graph=graph, first_state=h)
    for name in ("best_nnz", "hits", "solved_step", "solved_sample", "overflow", "tokens", "lengths"):
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(whole, name)), name
    assert torch.equal(torch.cat([a.groups, b.groups + h]), whole.groups)
    same_result(whole, want)


def test_solve_stream_ticks_and_empty_dataset(golden):
    d_states, scal, K, pol, want, ref = strassen_case(golden, 1, 1, 0)
    G = d_states.shape[0]
    steps = host(want.solved_step)
    one = rollout.solve_stream(pol, d_states, scal, 1, K, slots=1, check_every=1)
    assert one.ticks == int(np.where(steps >= 0, steps + 1, K).sum())      # one slot: the states one after another
    assert rollout.solve_stream(pol, d_states, scal, 1, K, slots=G, check_every=1).ticks == K
    assert rollout.solve_stream(pol, d_states, scal, 1, K, slots=G, check_every=0).ticks == SR.bound(G, G, K)
    empty = rollout.solve_stream(pol, d_states[:0], scal[:0], 1, K, slots=4)
    assert empty.ticks == 0 and empty.groups.numel() == 0 and tuple(empty.tokens.shape) == (0, K, 12)


# ---- the fused network ------------------------------------------------------------------------------------------------
def fused_setup(name, G, configs=NET_CONFIGS, cls=FusedAlphaTensor):
    """The arrangement of test_gpu_rollout_masked.py: a network that depends on its input and likes the zero factor
    (the last layer of the policy head scaled down, its bias favouring the token of 0), so a row plays the null action
    often and a start state that is zero is solved by it at once; every third start state is zero, the others hold
    random entries."""
    cfg = configs[name]
    sd = make_weights(cfg, 77)
    sd[P + "li1.weight"] = sd[P + "li1.weight"] * 0.25
    assert cfg["n_logits"] == 3                                  # tokens 0, 1, 2 are the factors -1, 0, 1
    sd[P + "li1.bias"] = np.array([0.0, 3.0, 0.0], np.float32)
    net = cls.from_state_dict(sd, cfg["n_samples"], device=DEV)
    S, T = cfg["dim_3d"], cfg["dim_t"]
    rng = np.random.default_rng(S)
    states = np.zeros((G, T, S, S, S), np.int8)
    states[:, 0] = rng.integers(-1, 2, size=(G, S, S, S))
    states[::3] = 0
    return net, dev(states), torch.zeros((G, cfg["dim_s"]), device=DEV)


@pytest.mark.parametrize("name", sorted(NET_CONFIGS))
def test_fused_slot_policy(name):
    G, n, K = 12, 4, 3
    net, states, scalars = fused_setup(name, G)
    want = rollout.solve_states(net.rollout_policy(11, masked=True), states, scalars, n, K, chunk_groups=G)
    steps = host(want.solved_step)
    print(name, "solved_step", steps.tolist())
    assert (steps >= 0).any() and (steps < 0).any()      # decided by the solve_states run
    pol = net.slot_policy(11)
    assert pol.takes_slots and pol.seed == 11
    got = rollout.solve_stream(pol, states, scalars, n, K, slots=5, check_every=2)
    same_result(got, want)
    assert got.ticks <= SR.bound(G, 5, K)
    same_result(rollout.solve_stream(net.slot_policy(11), states, scalars, n, K, slots=G + 1, graph=True), want)
    other = rollout.solve_stream(net.slot_policy(12), states, scalars, n, K, slots=5)
    assert not all(torch.equal(getattr(other, f), getattr(want, f)) for f in ("best_nnz", "solved_step", "tokens"))
