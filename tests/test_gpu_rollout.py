"""GPU checks of the sampled policy rollout (include/tensor_game_rollout.h, mat_mul_amd/rollout.py): bit for bit against
the numpy restatement (tests/rollout_ref.py), against the existing composition (functional.take_action), through
sample_rollouts with scripted policies on reference-recorded factorisations, with the fused network, and with a torch
stand-in model."""
import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, functional, ops, rollout
from mat_mul_amd._lib import TensorGameError

import rollout_ref as R
from guarded_buffers import CANARY, GUARD, check_flat, guarded
from net_ref import CONFIGS as CONFIGS_S4, make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from net_s16_ref import CONFIGS as CONFIGS_S16
from rollout_ref import demo_cases, strassen_scripts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NET_CONFIGS = {"a": CONFIGS_S4["a"], "a9": CONFIGS_S9["a9"], "a16": CONFIGS_S16["a16"]}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded_from(a, offset=0):
    """(buffer, device tensor equal to ``a``) with canary bytes around it; ``offset`` extra bytes in front misalign it."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    nbytes = a.nbytes
    buf = torch.full((GUARD + offset + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return buf, view


def check_guards(buf, offset, what):
    assert bool((buf[:GUARD + offset] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all()), what


# (S, T, n, G, misalign): every supported network size and two more, T = 1, 2, 4, n = 1, 3, 8, 64, from one group to a
# few thousand rows; misalign = 4 takes S = 4 / 16 off the 16-byte path
ADVANCE_CASES = [
    (3, 1, 1, 1, 0), (3, 2, 3, 50, 0), (3, 4, 64, 3, 0), (4, 1, 1, 4096, 0), (4, 2, 8, 300, 0), (4, 4, 64, 33, 0),
    (4, 2, 3, 41, 4), (5, 2, 3, 111, 0), (5, 4, 8, 17, 0), (5, 1, 64, 2, 0), (9, 1, 64, 5, 0), (9, 2, 8, 64, 0),
    (9, 4, 3, 7, 0), (9, 2, 1, 1, 0), (16, 2, 8, 40, 0), (16, 1, 1, 3, 0), (16, 4, 64, 2, 0), (16, 2, 3, 5, 4),
    (25, 2, 3, 5, 0), (25, 1, 8, 2, 0), (25, 4, 1, 3, 0), (25, 2, 64, 1, 0), (1, 1, 1, 7, 0), (2, 3, 8, 9, 0),
    (32, 2, 3, 1, 0),
]


@pytest.mark.parametrize("S,T,n,G,misalign", ADVANCE_CASES)
def test_advance_equals_the_restatement(S, T, n, G, misalign):
    rng = np.random.default_rng(1000 * S + 100 * T + n + G)
    B, K, dim_s, steps = G * n, 4, 2, 3
    frames = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    # some rows at zero from the start or after one step, so that hits / solved_* are exercised
    tok_all = rng.integers(0, 3, size=(steps, B, 3 * S)).astype(np.int8)
    zero_rows = rng.random(B) < 0.2
    frames[zero_rows, 0] = 0
    first = np.asarray(R.O.action_to_tensor(tok_all[0], 1))
    after_one = (rng.random(B) < 0.2) & ~zero_rows
    frames[after_one, 0] = first[after_one].astype(np.int8)
    tok_all[1, zero_rows | after_one] = 1  # the null action keeps them there for one more step
    scalars = rng.integers(0, 5, size=(B, dim_s)).astype(np.float32)
    rec = R.fresh_records(G, S)

    bufs = {}
    bufs["frames"], d_frames = guarded_from(frames, misalign)
    bufs["scalars"], d_scal = guarded_from(scalars)
    bufs["nnz"], d_nnz = guarded((B,), torch.int32)
    bufs["overflow"], d_ovf = guarded_from(np.zeros(B, np.uint8))
    bufs["actions"], d_act = guarded_from(np.zeros((B, K, 3 * S), np.int8))
    d_rec = []
    for name, r in zip(("best_nnz", "hits", "solved_step", "solved_sample"), rec):
        bufs[name], t = guarded_from(r)
        d_rec.append(t)

    ovf = np.zeros(B, np.uint8)
    act = np.zeros((B, K, 3 * S), np.int8)
    for step in range(steps):
        frames, nnz, rec, scalars, ovf, act = R.advance(frames, tok_all[step], n, step, rec, scalars, ovf, act, 1)
        got = ops.rollout_advance(d_frames, dev(tok_all[step]), n, step, d_rec, scalars=d_scal, nnz=d_nnz,
                                  overflow=d_ovf, actions=d_act, shift=1)
        assert got.data_ptr() == d_nnz.data_ptr()
        assert np.array_equal(host(d_frames), frames), step
        assert np.array_equal(host(d_nnz), nnz), step
        assert np.array_equal(host(d_scal), scalars), step
        assert np.array_equal(host(d_act), act), step
        assert np.array_equal(host(d_ovf), ovf), step
        for name, a, b in zip(("best_nnz", "hits", "solved_step", "solved_sample"), d_rec, rec):
            assert np.array_equal(host(a), b), (name, step)
    for name, buf in bufs.items():
        if name == "nnz":
            check_flat(buf, name)
        else:
            check_guards(buf, misalign if name == "frames" else 0, name)
    if G >= 5:
        assert rec[1].any() and (rec[2] >= 0).any()  # the planted zero rows were seen


@pytest.mark.parametrize("S,T,n", [(4, 2, 8), (9, 2, 3), (5, 1, 1), (16, 2, 8)])
def test_advance_overflow_wraps_and_is_flagged(S, T, n):
    rng = np.random.default_rng(S)
    G = 6
    B = G * n
    frames = rng.integers(-128, 128, size=(B, T, S, S, S)).astype(np.int8)
    frames[::2, 0] = np.clip(frames[::2, 0], -100, 100)   # these rows stay inside int8
    tokens = rng.integers(0, 3, size=(B, 3 * S)).astype(np.int8)
    want = R.advance(frames, tokens, n, 0, R.fresh_records(G, S), None, np.zeros(B, np.uint8), None, 1)
    assert want[4].any() and not want[4].all()
    d_frames, d_ovf, d_rec = dev(frames), torch.zeros(B, dtype=torch.uint8, device=DEV), ops.rollout_records(G, S, DEV)
    nnz = ops.rollout_advance(d_frames, dev(tokens), n, 0, d_rec, overflow=d_ovf, shift=1)
    assert np.array_equal(host(d_frames), want[0]) and np.array_equal(host(nnz), want[1])
    assert np.array_equal(host(d_ovf), want[4])
    # sticky: a second step that overflows nowhere clears nothing
    ops.rollout_advance(d_frames, dev(np.ones((B, 3 * S), np.int8)), n, 1, d_rec, overflow=d_ovf, shift=1)
    assert np.array_equal(host(d_ovf), want[4])
    # a wide shift takes the same 32-bit arithmetic
    tok2 = rng.integers(-3, 4, size=(B, 3 * S)).astype(np.int8)
    f2 = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    want2 = R.advance(f2, tok2, n, 0, R.fresh_records(G, S), None, np.zeros(B, np.uint8), None, -2)
    d_f2, d_o2 = dev(f2), torch.zeros(B, dtype=torch.uint8, device=DEV)
    nnz2 = ops.rollout_advance(d_f2, dev(tok2), n, 0, ops.rollout_records(G, S, DEV), overflow=d_o2, shift=-2)
    assert np.array_equal(host(d_f2), want2[0]) and np.array_equal(host(nnz2), want2[1])
    assert np.array_equal(host(d_o2), want2[4])


@pytest.mark.parametrize("S,T,n,G", [(4, 2, 8, 64), (9, 2, 3, 20), (16, 2, 8, 8), (5, 1, 1, 30), (25, 3, 4, 3)])
def test_one_step_equals_take_action(S, T, n, G):
    rng = np.random.default_rng(7 * S + n)
    B = G * n
    frames = dev(rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8))
    frames[::5, 0] = 0
    tokens = dev(rng.integers(1, 4, size=(B, 3 * S)).astype(np.int8))      # the reference's `- 2` vocabulary
    tokens[::5] = 2
    new_state, rank_ubs, best = functional.take_action(frames, tokens, n, shift=2)
    mine, rec = frames.clone(), ops.rollout_records(G, S, DEV)
    nnz = ops.rollout_advance(mine, tokens, n, 0, rec, shift=2)
    assert torch.equal(mine, new_state)
    assert torch.equal(nnz.view(-1, n), rank_ubs)
    assert torch.equal(rec[0], best.values)
    zero = best.values == 0
    assert bool(zero.any()) and torch.equal(rec[1], zero.to(torch.int32))
    assert torch.equal(rec[2], torch.where(zero, 0, -1).to(torch.int32))
    lowest = (rank_ubs == 0).to(torch.int32).argmax(dim=1).to(torch.int32)
    assert torch.equal(rec[3], torch.where(zero, lowest, torch.full_like(lowest, -1)))


def test_ops_validation_on_the_device():
    frames = torch.zeros((8, 2, 4, 4, 4), dtype=torch.int8, device=DEV)
    tok = torch.ones((8, 12), dtype=torch.int8, device=DEV)
    rec = ops.rollout_records(2, 4, DEV)
    with pytest.raises(TensorGameError, match="multiple of n"):
        ops.rollout_advance(frames, tok, 3, 0, ops.rollout_records(2, 4, DEV))
    with pytest.raises(TensorGameError, match="contiguous"):
        ops.rollout_advance(frames[:, :1], tok, 4, 0, rec)
    with pytest.raises(TensorGameError, match="best_nnz"):
        ops.rollout_advance(frames, tok, 4, 0, ops.rollout_records(3, 4, DEV))
    with pytest.raises(TensorGameError, match="max_actions"):
        ops.rollout_advance(frames, tok, 4, 2, rec, actions=torch.zeros((8, 2, 12), dtype=torch.int8, device=DEV))
    with pytest.raises(TensorGameError, match="tokens"):
        ops.rollout_advance(frames, tok.to(torch.int64), 4, 0, rec)
    assert not frames.any() and torch.equal(rec[1], torch.zeros_like(rec[1]))  # nothing was launched
    res = rollout.sample_rollouts(lambda *a: tok[:0], frames[:0], torch.zeros((0, 1), device=DEV), 4, 3)
    assert res.num_solved.item() == 0 and res.lowest_rank.item() == 64


# ---- scripted policies through sample_rollouts ------------------------------------------------------------------------
def table_policy(np_policy, K):
    """A device policy that plays the tokens a numpy policy (which ignores the state) produces, and the table itself."""
    table = np.stack([np_policy(None, None, None, k) for k in range(K)])
    d_table = dev(table)
    return (lambda frames, scalars, rows, step: d_table[step]), table


def compare(res, want):
    for name in ("best_nnz", "hits", "solved_step", "solved_sample", "frames", "scalars", "nnz", "overflow", "actions"):
        assert np.array_equal(host(getattr(res, name)), getattr(want, name)), name
    assert res.lowest_rank.item() == want.lowest_rank and res.num_hits.item() == want.num_hits
    assert res.num_solved.item() == want.num_solved
    for a, b in zip(res.solutions(), R.solutions(want)):
        assert np.array_equal(host(a), b)


@pytest.mark.parametrize("shift,n,slot", [(1, 1, 0), (2, 1, 0), (1, 4, 2)])
def test_strassen_states_through_sample_rollouts(golden, shift, n, slot):
    states, scripts, lengths = strassen_scripts(golden, shift)
    K, G = 9, len(scripts)
    pol, table = table_policy(R.scripted_policy(scripts, 4, n, slot, shift, seed=5), K)
    want = R.rollout(lambda f, s, r, k: table[k], states, np.zeros((G, 1), np.float32), n, K, shift)
    res = rollout.sample_rollouts(pol, dev(states), torch.zeros((G, 1), device=DEV), n, K, shift=shift)
    compare(res, want)
    assert res.num_solved.item() == 448
    if n == 1:
        assert np.array_equal(host(res.solved_step), lengths - 1)
        assert np.array_equal(host(res.hits), K - (lengths - 1))
    groups, tokens, lens = (host(x) for x in res.solutions())
    for g, tok, L in zip(groups, tokens, lens):
        assert not R.O.take_actions(list(tok[:L]), states[g, 0], shift).any()
    # record_actions=False keeps the statistics and refuses solutions()
    res2 = rollout.sample_rollouts(pol, dev(states), torch.zeros((G, 1), device=DEV), n, K, shift=shift,
                                   record_actions=False)
    assert torch.equal(res2.solved_step, res.solved_step) and res2.actions is None
    with pytest.raises(TensorGameError, match="record"):
        res2.solutions()


def test_recorded_demonstrations_through_sample_rollouts(golden):
    for name, target, script in demo_cases(golden):
        S, K, T, n = target.shape[-1], len(script) + 1, 2, 4
        states = np.zeros((1, T, S, S, S), np.int8)
        states[:, 0] = target[:, 0]
        pol, table = table_policy(R.scripted_policy([script], S, n, 2, 1, seed=3), K)
        want = R.rollout(lambda f, s, r, k: table[k], states, np.zeros((1, 1), np.float32), n, K, 1)
        res = rollout.sample_rollouts(pol, dev(states), torch.zeros((1, 1), device=DEV), n, K)
        compare(res, want)
        groups, tokens, lens = (host(x) for x in res.solutions())
        assert list(groups) == [0], name
        assert not R.O.take_actions(list(tokens[0][:lens[0]]), target[0, 0], 1).any()


# ---- the fused network ------------------------------------------------------------------------------------------------
def fused_setup(name):
    cfg = NET_CONFIGS[name]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 77), cfg["n_samples"], device=DEV)
    S, T = cfg["dim_3d"], cfg["dim_t"]
    G = {"a": 24, "a9": 6, "a16": 3}[name]
    K = {"a": 5, "a9": 3, "a16": 2}[name]
    rng = np.random.default_rng(S)
    states = np.zeros((G, T, S, S, S), np.int8)
    states[:, 0] = rng.integers(-1, 2, size=(G, S, S, S))
    return net, dev(states), torch.zeros((G, cfg["dim_s"]), device=DEV), K


def unfused(net, states, scalars, n, K, seed):
    """The same loop from the pieces that existed before: net.torso, net.sample(k=1, rows, call=step) and
    functional.take_action, the statistics in torch."""
    frames, scal = states.repeat_interleave(n, 0).contiguous(), scalars.repeat_interleave(n, 0).contiguous()
    B, G = frames.shape[0], states.shape[0]
    rows = torch.arange(B, device=DEV)
    best = torch.full((G,), states.shape[2] ** 3, dtype=torch.int32, device=DEV)
    hits = torch.zeros((G,), dtype=torch.int32, device=DEV)
    played = []
    for step in range(K):
        tok, _, _ = net.sample(net.torso(frames, scal), rows, seed, call=step, k=1)
        tok = tok.view(B, -1)
        played.append(tok.clone())
        frames, rank_ubs, m = functional.take_action(frames, tok, n, shift=1)
        scal = scal + 1
        best = torch.minimum(best, m.values)
        hits += (m.values == 0).to(torch.int32)
    return frames, scal, best, hits, torch.stack(played, 1)


@pytest.mark.parametrize("name", sorted(NET_CONFIGS))
def test_fused_policy_rollout(name):
    net, states, scalars, K = fused_setup(name)
    n = 8
    start = states.clone()
    a = rollout.sample_rollouts(net.rollout_policy(seed=11), states, scalars, n, K)
    b = rollout.sample_rollouts(net.rollout_policy(seed=11), states, scalars, n, K)
    assert torch.equal(states, start)
    for f in ("frames", "scalars", "actions", "best_nnz", "hits", "solved_step", "solved_sample", "nnz", "overflow"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    frames, scal, best, hits, played = unfused(net, states, scalars, n, K, 11)
    assert torch.equal(a.frames, frames) and torch.equal(a.scalars, scal) and torch.equal(a.actions, played)
    assert torch.equal(a.best_nnz, best) and torch.equal(a.hits, hits)
    assert a.lowest_rank.item() == best.min().item() and a.num_hits.item() == hits.sum().item()
    c = rollout.sample_rollouts(net.rollout_policy(seed=12), states, scalars, n, K)
    assert not torch.equal(a.actions, c.actions)
    g = rollout.sample_rollouts(net.rollout_policy(seed=11), states, scalars, n, K, graph=True)
    torch.cuda.synchronize()
    for f in ("frames", "scalars", "actions", "best_nnz", "hits", "solved_step", "solved_sample", "nnz", "overflow"):
        assert torch.equal(getattr(a, f), getattr(g, f)), f
    assert g.graph is not None and a.graph is None
    # the row keying: the n samples of a state do not all play the same first action (for this seed, every group)
    first = a.actions[:, 0].view(states.shape[0], n, -1)
    assert bool((first != first[:, :1]).flatten(1).any(1).all())
    # the restatement fed the same tokens agrees on every record
    table = host(a.actions).transpose(1, 0, 2)
    want = R.rollout(lambda f, s, r, k: table[k], host(states), host(scalars), n, K, 1)
    compare(a, want)


def test_rollout_policy_needs_one_action_per_sample():
    cfg = dict(NET_CONFIGS["a"], n_steps=8)
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 3), 8, device=DEV)
    with pytest.raises(TensorGameError, match="n_steps"):
        net.rollout_policy()


# ---- a torch model ------------------------------------------------------------------------------------------------------
class StandIn(torch.nn.Module):
    """Has AlphaTensor.fwd_infer's signature and return shapes (model.py:347-356); the tokens are a deterministic
    function of the float frames and the scalars."""

    def __init__(self, S, n_samples=2):
        super().__init__()
        self.S, self.n_samples = S, n_samples
        g = torch.Generator().manual_seed(S)
        self.proj = torch.nn.Parameter(torch.randint(0, 7, (S ** 3, n_samples * 3 * S), generator=g).float())

    def fwd_infer(self, xx, ss):
        assert xx.dtype == torch.float32 and xx.dim() == 5
        B = xx.shape[0]
        z = xx[:, 0].reshape(B, -1) @ self.proj + ss[:, :1] + torch.arange(B, device=xx.device)[:, None]
        aa = torch.remainder(z.round().to(torch.int64), 3).view(B, self.n_samples, 3 * self.S)
        return aa, torch.ones((B, self.n_samples), device=xx.device), torch.zeros((B,), device=xx.device)


@pytest.mark.parametrize("S,T,n,G", [(4, 2, 4, 32), (5, 1, 3, 10)])
def test_model_policy_with_a_stand_in_module(S, T, n, G):
    model = StandIn(S).to(DEV)
    rng = np.random.default_rng(S)
    states = np.zeros((G, T, S, S, S), np.int8)
    states[:, 0] = rng.integers(-1, 2, size=(G, S, S, S))
    states[::4, 0] = 0
    K = 4
    inner = rollout.model_policy(model)
    seen = []

    def logging(frames, scalars, rows, step):
        assert frames.dtype == torch.int8 and rows.dtype == torch.int64 and tuple(rows.shape) == (G * n,)
        tok = inner(frames, scalars, rows, step)
        assert tok.dtype == torch.int8 and tuple(tok.shape) == (G * n, 3 * S)
        seen.append(host(tok).copy())
        return tok

    res = rollout.sample_rollouts(logging, dev(states), torch.zeros((G, 1), device=DEV), n, K)
    assert len(seen) == K
    want = R.rollout(lambda f, s, r, k: seen[k], states, np.zeros((G, 1), np.float32), n, K, 1)
    compare(res, want)
