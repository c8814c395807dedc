"""GPU checks of the solution search that stops solved groups (tg_rollout_advance_masked,
``sample_rollouts(stop_solved=True)``, ``FusedAlphaTensor.rollout_policy(masked=True)``, ``solve_states``): the step bit
for bit against the numpy restatement (tests/rollout_masked_ref.py) with planted solves, poisoned tokens and guarded
buffers, and the relation to the plain run (``rollout_masked_ref.check_property``) through every layer above it."""
import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, ops, rollout
from mat_mul_amd._lib import TensorGameError

import rollout_masked_ref as M
import rollout_ref as R
from guarded_buffers import CANARY, GUARD
from net_ref import CONFIGS as CONFIGS_S4, P, make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from rollout_ref import demo_cases, strassen_scripts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NET_CONFIGS = {"a": CONFIGS_S4["a"], "a9": CONFIGS_S9["a9"]}
FIELDS = M.RECORDS + M.ROWS + ("active",)


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


# ---- the step against the restatement -------------------------------------------------------------------------------
def planted(S, T, n, G, steps, rng):
    """(frames (B,T,S,S,S), tokens (steps,B,3S)), shift 1, in which group g is solved at step 0 when g % 3 == 0 and at
    step 1 when g % 3 == 1, by its sample g % n alone, and never when g % 3 == 2.  Every row but the winning ones has a
    head with four entries of 2 and plays tokens whose tensor has ONE entry of +-1: three steps change three entries by
    one, so such a row cannot reach zero.  A winning row plays rank-1 tensors with no zero factor and starts at their
    sum over the steps up to its solving step."""
    B = G * n
    frames = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    frames[:, 0, 0, 0, :4] = 2
    factors = np.zeros((steps, B, 3, S), np.int8)
    hot = rng.integers(0, S, size=(steps, B, 3))
    np.put_along_axis(factors, hot[..., None], rng.choice([-1, 1], size=(steps, B, 3, 1)).astype(np.int8), axis=3)
    for g in range(G):
        if g % 3 == 2:
            continue
        b, last = g * n + g % n, g % 3
        f = rng.integers(-1, 2, size=(last + 1, 3, S)).astype(np.int8)
        f[:, :, 0] = np.where(f.any(axis=2), f[:, :, 0], 1)  # no zero factor: every term is a non-zero tensor
        factors[:last + 1, b] = f
        terms = np.asarray(R.O.action_to_tensor((f + 1).reshape(last + 1, 3 * S), 1))
        frames[b, 0] = terms.sum(axis=0).astype(np.int8)
    return frames, (factors + 1).reshape(steps, B, 3 * S).astype(np.int8)


# (S, T, n, G, misalign): many small groups per workgroup with some of them solved; the dword path with a tail item,
# off its alignment; one group per workgroup with 16-byte items; about 32 one-row groups per workgroup; S = 25
MASKED_CASES = [(4, 2, 8, 37, 0), (9, 2, 3, 20, 1), (16, 2, 8, 8, 0), (5, 1, 1, 30, 3), (25, 3, 4, 3, 0)]


@pytest.mark.parametrize("S,T,n,G,misalign", MASKED_CASES)
def test_masked_advance_equals_the_restatement(S, T, n, G, misalign):
    rng = np.random.default_rng(100 * S + n + G)
    B, K, dim_s, steps = G * n, 4, 2, 3
    frames, tok_all = planted(S, T, n, G, steps, rng)
    scalars = rng.integers(0, 5, size=(B, dim_s)).astype(np.float32)
    rec = R.fresh_records(G, S)
    nnz, ovf, act, active = np.zeros(B, np.int32), np.zeros(B, np.uint8), np.zeros((B, K, 3 * S), np.int8), np.ones(B, np.uint8)

    bufs, d = {}, {}
    for name, a in (("frames", frames), ("scalars", scalars), ("nnz", nnz), ("overflow", ovf), ("actions", act),
                    ("active", active), *zip(M.RECORDS, rec)):
        bufs[name], d[name] = guarded_from(a, misalign if name == "frames" else 0)
    d_rec = [d[name] for name in M.RECORDS]
    # the same steps without `active`
    e_frames, e_rec = dev(frames), [dev(r) for r in rec]
    e_nnz = torch.zeros(B, dtype=torch.int32, device=DEV)

    for step in range(steps):
        solved_rows = np.repeat(rec[2] >= 0, n)
        want_tok = tok_all[step]
        poisoned = want_tok.copy()
        poisoned[solved_rows] = 127   # what an inactive row offers must not be read
        buf_tok, d_tok = guarded_from(poisoned)
        frames, nnz, rec, scalars, ovf, act, active = M.advance_masked(frames, want_tok, n, step, rec, nnz, scalars, ovf,
                                                                       act, active, 1)
        got = ops.rollout_advance(d["frames"], d_tok, n, step, d_rec, scalars=d["scalars"], nnz=d["nnz"],
                                  overflow=d["overflow"], actions=d["actions"], shift=1, active=d["active"],
                                  stop_solved=True)
        assert got.data_ptr() == d["nnz"].data_ptr()
        ops.rollout_advance(e_frames, d_tok, n, step, e_rec, nnz=e_nnz, shift=1, stop_solved=True)
        for name, want in (("frames", frames), ("scalars", scalars), ("nnz", nnz), ("overflow", ovf), ("actions", act),
                           ("active", active), *zip(M.RECORDS, rec)):
            assert np.array_equal(host(d[name]), want), (name, step)
        assert np.array_equal(host(d_tok), poisoned)
        check_guards(buf_tok, 0, "tokens")
        # the planted cases, exactly
        want_step = np.where(np.arange(G) % 3 <= min(step, 1), np.arange(G) % 3, -1)
        want_step[np.arange(G) % 3 == 2] = -1
        assert np.array_equal(rec[2], want_step), step
    for name, buf in bufs.items():
        check_guards(buf, misalign if name == "frames" else 0, name)
    thirds = [int((np.arange(G) % 3 == k).sum()) for k in range(3)]
    assert [int((rec[2] == 0).sum()), int((rec[2] == 1).sum()), int((rec[2] < 0).sum())] == thirds
    assert np.array_equal(rec[3][rec[2] >= 0], (np.arange(G) % n)[rec[2] >= 0])
    assert np.array_equal(rec[1], (rec[2] >= 0).astype(np.int32))          # hits: 0 or 1
    assert np.array_equal(active, np.repeat(rec[2] < 0, n).astype(np.uint8))
    assert not ovf.any()
    # NULL `active`: the same records, frames and counts
    assert np.array_equal(host(e_frames), frames) and np.array_equal(host(e_nnz), nnz)
    for name, a, b in zip(M.RECORDS, e_rec, rec):
        assert np.array_equal(host(a), b), name


def test_plain_entry_still_steps_solved_groups():
    """The same planted inputs through the plain entry: hits keeps counting and the rows keep moving."""
    S, T, n, G = 4, 2, 8, 37
    frames, tok_all = planted(S, T, n, G, 3, np.random.default_rng(5))
    tok_all[1:, np.repeat(np.arange(G) % 3 == 0, n)] = 1   # the null action from step 1 on keeps those groups at zero
    d_frames, rec = dev(frames), ops.rollout_records(G, S, DEV)
    want, want_rec = frames, R.fresh_records(G, S)
    for step in range(3):
        ops.rollout_advance(d_frames, dev(tok_all[step]), n, step, rec, shift=1)
        want, _, want_rec, _, _, _ = R.advance(want, tok_all[step], n, step, want_rec, None, None, None, 1)
    assert np.array_equal(host(d_frames), want)
    for a, b in zip(rec, want_rec):
        assert np.array_equal(host(a), b)
    assert (host(rec[1])[np.arange(G) % 3 == 0] == 3).all()


def test_ops_refuses_active_without_stop_solved():
    frames = torch.zeros((8, 2, 4, 4, 4), dtype=torch.int8, device=DEV)
    tok = torch.ones((8, 12), dtype=torch.int8, device=DEV)
    rec = ops.rollout_records(2, 4, DEV)
    with pytest.raises(TensorGameError, match="stop_solved=True"):
        ops.rollout_advance(frames, tok, 4, 0, rec, active=torch.ones(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(TensorGameError, match="active"):
        ops.rollout_advance(frames, tok, 4, 0, rec, active=torch.ones(7, dtype=torch.uint8, device=DEV), stop_solved=True)
    assert torch.equal(rec[1], torch.zeros_like(rec[1]))
    res = rollout.sample_rollouts(lambda *a: tok[:0], frames[:0], torch.zeros((0, 1), device=DEV), 4, 3, stop_solved=True)
    assert res.num_solved.item() == 0 and res.steps_run == 0 and res.active.numel() == 0


# ---- table policies through sample_rollouts ---------------------------------------------------------------------------
def table_policy(np_policy, K):
    """A device policy that plays the tokens a numpy policy (which ignores the state) produces, keyed by the row
    indices it is given, and the table itself."""
    table = np.stack([np_policy(None, None, None, k) for k in range(K)])
    d_table = dev(table)
    return (lambda frames, scalars, rows, step: d_table[step][rows]), table


def same(res, want, fields=FIELDS):
    for name in fields:
        a, b = getattr(res, name), getattr(want, name)
        assert np.array_equal(host(a) if torch.is_tensor(a) else a, host(b) if torch.is_tensor(b) else b), name


def run_both(table, pol, states, n, K, shift, **kw):
    """(plain run on the device, masked run on the device, plain numpy trace) of one table policy."""
    G = len(states)
    scal = np.arange(G, dtype=np.float32)[:, None]
    plain = rollout.sample_rollouts(pol, dev(states), dev(scal), n, K, shift=shift)
    masked = rollout.sample_rollouts(pol, dev(states), dev(scal), n, K, shift=shift, stop_solved=True, **kw)
    trace = M.plain_trace(lambda f, s, r, k: table[k], states, scal, n, K, shift)
    want = M.rollout_masked(lambda f, s, r, k: table[k], states, scal, n, K, shift)
    same(masked, want)
    assert masked.steps_run == K and masked.lowest_rank.item() == want.lowest_rank
    assert masked.num_hits.item() == want.num_hits == masked.num_solved.item() == plain.num_solved.item()
    return plain, masked, trace


@pytest.mark.parametrize("shift,n,slot", [(1, 1, 0), (2, 1, 0), (1, 4, 2)])
def test_property_on_the_strassen_states(golden, shift, n, slot):
    states, scripts, lengths = strassen_scripts(golden, shift)
    K = 9                                                        # two steps past the latest solve (step 6)
    stuck = np.arange(len(scripts)) % 5 == 4                     # these play the null action for ever
    scripts = [[R.null_action(4, shift)] if s else sc for s, sc in zip(stuck, scripts)]
    pol, table = table_policy(R.scripted_policy(scripts, 4, n, slot, shift, seed=5), K)
    plain, masked, trace = run_both(table, pol, states, n, K, shift)
    n_solved, n_unsolved = M.check_property(masked, plain, trace.after, get=host)
    steps = host(plain.solved_step)
    assert len(set(steps[steps >= 0])) >= 2 and n_unsolved >= 1 and n_solved >= 2
    if n == 1:
        assert np.array_equal(steps >= 0, ~stuck) and np.array_equal(steps[~stuck], lengths[~stuck] - 1)
    for a, b in zip(masked.solutions(), plain.solutions()):
        assert torch.equal(a, b)
    groups, tokens, lens = (host(x) for x in masked.solutions())
    for g, tok, L in zip(groups, tokens, lens):
        assert not R.O.take_actions(list(tok[:L]), states[g, 0], shift).any()
    # graph=True: the same launches, the mask read when they run
    scal = dev(np.arange(len(states), dtype=np.float32)[:, None])
    g = rollout.sample_rollouts(pol, dev(states), scal, n, K, shift=shift, stop_solved=True, graph=True)
    torch.cuda.synchronize()
    same(g, masked)
    assert g.graph is not None and g.steps_run == K


def test_property_on_the_recorded_demonstrations(golden):
    for name, target, script in demo_cases(golden):
        S, K, T, n = target.shape[-1], len(script) + 2, 2, 4
        states = np.zeros((2, T, S, S, S), np.int8)
        states[:, 0] = target[:, 0]
        states[1, 0, 0, 0, 0] += 1                              # one entry off: the script leaves this group unsolved
        pol, table = table_policy(R.scripted_policy([script, script], S, n, 2, 1, seed=3), K)
        plain, masked, trace = run_both(table, pol, states, n, K, 1)
        n_solved, n_unsolved = M.check_property(masked, plain, trace.after, get=host)
        assert n_solved >= 1 and host(plain.solved_step)[0] >= 0, name
        for a, b in zip(masked.solutions(), plain.solutions()):
            assert torch.equal(a, b)


def test_check_every_leaves_the_loop_at_the_first_multiple(golden):
    states, scripts, lengths = strassen_scripts(golden, 1)
    states, scripts, lengths = states[::9], scripts[::9], lengths[::9]
    G, K, k = len(scripts), 12, int(lengths.max()) - 1          # every group is solved by step k
    pol, table = table_policy(R.scripted_policy(scripts, 4, 1, 0, 1), K)
    d_states, scal = dev(states), torch.zeros((G, 1), device=DEV)
    full = rollout.sample_rollouts(pol, d_states, scal, 1, K, stop_solved=True)
    assert full.steps_run == K and full.num_solved.item() == G and int(host(full.solved_step).max()) == k
    for m in (1, 2, 3, 4, 5, K):
        got = rollout.sample_rollouts(pol, d_states, scal, 1, K, stop_solved=True, check_every=m)
        assert got.steps_run == -(-(k + 1) // m) * m
        same(got, full)
    with pytest.raises(TensorGameError, match="graph=True"):
        rollout.sample_rollouts(pol, d_states, scal, 1, K, stop_solved=True, check_every=2, graph=True)
    # a group that is never solved keeps the loop going to the end
    scripts[0] = [R.null_action(4, 1)]
    pol2, _ = table_policy(R.scripted_policy(scripts, 4, 1, 0, 1), K)
    assert rollout.sample_rollouts(pol2, d_states, scal, 1, K, stop_solved=True, check_every=1).steps_run == K


def test_solve_states_does_not_depend_on_the_chunks(golden):
    states, scripts, lengths = strassen_scripts(golden, 1)
    states, scripts = states[::20], scripts[::20]
    G, n, K = len(scripts), 2, 9
    assert G % 5 and G > 10
    scripts[3] = [R.null_action(4, 1)]                           # one group stays unsolved (its other sample is random)
    pol, table = table_policy(R.scripted_policy(scripts, 4, n, 1, 1, seed=2), K)
    d_states, scal = dev(states), torch.zeros((G, 1), device=DEV)
    one = rollout.sample_rollouts(pol, d_states, scal, n, K, stop_solved=True)
    sols = one.solutions()
    assert 2 <= one.num_solved.item() < G
    for c in (1, 5, G):
        got = rollout.solve_states(pol, d_states, scal, n, K, chunk_groups=c, check_every=2)
        same(got, one, M.RECORDS)
        for a, b in zip((got.groups, got.tokens, got.lengths), sols):
            assert torch.equal(a, b), c
        assert len(got.steps_run) == -(-G // c) and max(got.steps_run) <= K
    empty = rollout.solve_states(pol, d_states[:0], scal[:0], n, K, chunk_groups=4)
    assert empty.groups.numel() == 0 and tuple(empty.tokens.shape) == (0, K, 12) and empty.steps_run == (0,)


# ---- the fused network ------------------------------------------------------------------------------------------------
def fused_setup(name):
    """A network that depends on its input and likes the zero factor: the last layer of the policy head is scaled down
    and its bias favours the token of 0, so a row plays the null action often, and a start state that is zero is
    solved by it at once.  Every third group starts at zero, the others at random entries."""
    cfg = NET_CONFIGS[name]
    sd = make_weights(cfg, 77)
    sd[P + "li1.weight"] = sd[P + "li1.weight"] * 0.25
    assert cfg["n_logits"] == 3                                  # tokens 0, 1, 2 are the factors -1, 0, 1
    sd[P + "li1.bias"] = np.array([0.0, 3.0, 0.0], np.float32)
    net = FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)
    S, T = cfg["dim_3d"], cfg["dim_t"]
    G, K = {"a": 24, "a9": 6}[name], {"a": 5, "a9": 3}[name]
    rng = np.random.default_rng(S)
    states = np.zeros((G, T, S, S, S), np.int8)
    states[:, 0] = rng.integers(-1, 2, size=(G, S, S, S))
    states[::3] = 0
    return net, dev(states), torch.zeros((G, cfg["dim_s"]), device=DEV), K


@pytest.mark.parametrize("name", sorted(NET_CONFIGS))
def test_fused_masked_policy(name):
    net, states, scalars, K = fused_setup(name)
    n, G = 8, states.shape[0]
    plain = rollout.sample_rollouts(net.rollout_policy(seed=11), states, scalars, n, K)
    pol = net.rollout_policy(seed=11, masked=True)
    assert pol.takes_active
    a = rollout.sample_rollouts(pol, states, scalars, n, K, stop_solved=True)
    n_solved, n_unsolved = M.check_property(a, plain, get=host)
    print(name, "solved", n_solved, "unsolved", n_unsolved, "solved_step", host(plain.solved_step).tolist())
    assert n_solved >= 1 and n_unsolved >= 1      # decided by the plain run: both halves of the property are exercised
    for x, y in zip(a.solutions(), plain.solutions()):
        assert torch.equal(x, y)
    # the plain policy under stop_solved is asked for all rows and ends at the same results
    same(rollout.sample_rollouts(net.rollout_policy(seed=11), states, scalars, n, K, stop_solved=True), a)
    # two runs are equal, and a fresh policy of the same seed plays the same games
    same(rollout.sample_rollouts(pol, states, scalars, n, K, stop_solved=True), a)
    same(rollout.sample_rollouts(net.rollout_policy(seed=11, masked=True), states, scalars, n, K, stop_solved=True), a)
    c = rollout.sample_rollouts(net.rollout_policy(seed=12, masked=True), states, scalars, n, K, stop_solved=True)
    assert not torch.equal(a.actions, c.actions)
    # graph=True equals eager bit for bit
    g = rollout.sample_rollouts(net.rollout_policy(seed=11, masked=True), states, scalars, n, K, stop_solved=True,
                                graph=True)
    torch.cuda.synchronize()
    same(g, a)
    assert g.graph is not None and a.graph is None
    # inactive rows of the token buffer keep what they held
    frames = states.repeat_interleave(n, 0).contiguous()
    rows = torch.arange(G * n, device=DEV)
    active = (rows % 2).to(torch.uint8)
    out = torch.full((G * n, net.n_steps), 99, dtype=torch.int8, device=DEV)
    assert pol(frames, scalars.repeat_interleave(n, 0), rows, 0, active=active, out=out) is out
    assert bool((out[::2] == 99).all()) and torch.equal(out[1::2], a.actions[1::2, 0])
    # the dataset loop with the masked policy: the chunking does not show
    whole = rollout.solve_states(pol, states, scalars, n, K, chunk_groups=G)
    parts = rollout.solve_states(pol, states, scalars, n, K, chunk_groups=5, check_every=2)
    same(whole, a, M.RECORDS)
    same(parts, a, M.RECORDS)
    for x, y, z in zip((parts.groups, parts.tokens, parts.lengths), (whole.groups, whole.tokens, whole.lengths),
                       a.solutions()):
        assert torch.equal(x, y) and torch.equal(x, z)
