"""Paths of training at the 5x5 tensor (train_decode_s25_kernel / Game25 in mat_mul_amd/csrc/tg_train_sliced.hip,
include/tensor_game_train_s25.h) that tests/test_gpu_train_s25.py holds at one value, on the MI355X, each against
train_ref's float64 autograd under the suite's bound (train_ref.within: 1e-4 * max(1, max |ref|) per tensor, or twice
the eager float32 restatement's own error where that misses the bound too):

1. the torso backward's runs of (game, slice) units: B * 25 below 256, runs of one and two units, runs of two and three
   that straddle games, each batch under the default loss weights and under the row's scaled pair, where every torso.*
   tensor's bound is relative;
2. the decoder's runs of games around 256: a slab zeroed whole by launch 3 (B = 255), runs of two and three games, on
   odd25 and, at B = 513, on c25 (three games of 2 self-attention and 13 cross-attention chunks per workgroup);
3. each loss alone, with the exact zeros the header promises, on the rows with a partial last chunk in either block;
4. the quantile loss's four branches;
5. a workspace of exactly tg_net_train_s25_workspace_size bytes between guard bytes, full of 0xFF bytes (NaN) and of
   what a larger batch left behind (the part offsets, the accumulators' included, move with B), for the gradient call
   and the loss-only call, and through SlicedTrainer25;
6. every row with a token outside [0, n_logits): launch 2 adds no policy term to its slabs;
7. float32 frames with T > 1, bitwise equal to int8 frames.

Rewards are two-sided (train_ref.two_sided_rewards) throughout.  tests/test_train_s25_paths_cpu.py shows on the CPU that
these inputs reach the paths and tell wrong work-cutting from the right one.  Each check prints (run with -s) a
TRAIN-S25-PATHS-ERR line: the worst error of a tensor over that tensor's own max |ref| (no floor of 1), for the fused
kernels and for eager float32."""
import numpy as np
import pytest
import torch

from mat_mul_amd import SlicedTrainer25
from mat_mul_amd._lib import TG_TRAIN_STATUS_BAD_TOKEN
from mat_mul_amd.train import unpack_weights

import guarded_buffers as G
from net_ref import P, dims
from net_s25_train_family import ROWS, workspace_bytes
from train_ref import (GuardedCall, TrainRef, compare_grads, keep_mask, multipliers, two_sided_batch, value_branches)
from test_train_s25_paths_cpu import (B, B_TORSO, B_WORKSPACE, DECODER_CASES, ROWS_PATHS, ROWS_WORKSPACE, SEED_BATCH,
                                      SEED_BRANCH, WEIGHTS_DEFAULT, batch_seed, weights, weights_scaled)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_TRAIN = 1e-4
LI1 = (P + "li1.weight", P + "li1.bias")


def trainer(name, **kw):
    return SlicedTrainer25.from_state_dict(weights(name), **dict(dict(dropout_p=0.0, seed=7, device=DEV), **kw))


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def gradient(tr, name):
    """The trainer's gradient as a reference-format dict of numpy arrays."""
    got = unpack_weights(tr.params.grad, tr.config, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    return {k: v.numpy() for k, v in got.items() if k != P + "pos_enc_fix"}


def compare(name, what, got, batch, **kw):
    """got = (l_pol, l_val, {name: gradient}) of the fused kernels against TrainRef.loss_grad(*batch, **kw) in float64
    under the suite's bound."""
    ref = TrainRef(weights(name), ROWS[name], device=DEV).loss_grad(*batch, **kw)
    ref32 = TrainRef(weights(name), ROWS[name], device=DEV, dtype=torch.float32).loss_grad(*batch, **kw)
    compare_grads("TRAIN-S25-PATHS-ERR", f"{name} {what}", got, ref, ref32, TOL_TRAIN)


def fused(name, batch, **kw):
    """(l_pol, l_val, gradient dict, trainer) of one call on ``batch`` (numpy)."""
    tr = trainer(name, **{k: kw.pop(k) for k in ("weight_pol", "weight_val", "dropout_p") if k in kw})
    l_pol, l_val = tr.loss_and_grad(*dev_batch(batch), **kw)
    torch.cuda.synchronize()
    return float(l_pol), float(l_val), gradient(tr, name), tr


def check(name, b, seed, what, wpol, wval):
    """One call under the weights (wpol, wval) against float64; the losses compared are the unweighted ones."""
    batch = two_sided_batch(ROWS[name], b, seed)
    got = fused(name, batch, weight_pol=wpol, weight_val=wval)
    assert int(got[3].status[0]) == 0
    compare(name, f"B={b} {what} weights=({wpol:g}, {wval:g})", got[:3], batch, weight_pol=wpol, weight_val=wval)
    return got, batch


def bits(t):
    return t.view(torch.int32)


# ---- 1. the torso runs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [lambda name: WEIGHTS_DEFAULT, weights_scaled], ids=["default", "scaled"])
@pytest.mark.parametrize("b", B_TORSO)
def test_torso_runs_around_the_number_of_slabs(b, pair):
    check("odd25", b, SEED_BATCH, "torso runs", *pair("odd25"))


# ---- 2. the decoder runs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, b", DECODER_CASES)
def test_decoder_runs_around_the_number_of_slabs(name, b):
    (l_pol, l_val, _, tr), batch = check(name, b, batch_seed(name, b), "decoder runs", *weights_scaled(name))
    if b == 513:
        first = tr.params.grad.clone()
        tr.params.grad.zero_()
        again = tr.loss_and_grad(*dev_batch(batch))
        torch.cuda.synchronize()
        assert torch.equal(bits(first), bits(tr.params.grad))
        assert float(again[0]) == l_pol and float(again[1]) == l_val


# ---- 3. each loss alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wpol, wval", [(16.0, 0.0), (0.0, 8000.0), (0.25, 3.0)])
@pytest.mark.parametrize("name", ROWS_PATHS)
def test_each_loss_alone(name, wpol, wval):
    got, _ = check(name, B, SEED_BATCH, "alone", wpol, wval)
    if wval == 0.0:  # the loss gradient is multiplied by the weight before anything else
        zero = [k for k in got[2] if k.startswith("value_head.")]
        assert len(zero) == 8 and all(not got[2][k].any() for k in zero)
    if wpol == 0.0:
        assert all(not got[2][k].any() for k in LI1)


# ---- 4. the value branches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_PATHS)
def test_value_loss_branches(name):
    batch = two_sided_batch(ROWS[name], B, SEED_BRANCH)
    shares, margin = value_branches(TrainRef(weights(name), ROWS[name], device=DEV), *batch)
    assert min(shares.values()) >= 0.10, shares
    assert margin >= 1e-4, margin  # ten times the inference bound on q: float32 cannot change a branch
    check(name, B, SEED_BRANCH, "branches", *WEIGHTS_DEFAULT)


# ---- 5. the workspace and the output buffers -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_WORKSPACE)
def test_exact_workspace_between_guards_nans_and_what_a_larger_batch_left(name):
    """B = 300 on a workspace of NaNs, then B = 37 and B = 5 (Pt = 125, Pd = 5) in the same memory, the gradient call and
    the loss-only call in turn, then all of it again after a refill with NaNs: each result is that of the same call on
    a fresh zeroed workspace of exactly its own size."""
    tr = trainer(name)
    m = dims(ROWS[name])
    batches = {b: dev_batch(two_sided_batch(ROWS[name], b, SEED_BATCH)) for b in B_WORKSPACE}
    want = {}
    for b, batch in batches.items():
        fresh = GuardedCall(tr, batch, fill=0)
        assert fresh.ws.numel() == tr._workspace_size(tr.c, b) == workspace_bytes(m, b)
        want[b] = {grad: fresh.run(grad) for grad in (True, False)}
        assert torch.equal(bits(want[b][False][1]), bits(want[b][True][1]))  # the loss-only call's losses
    first = GuardedCall(tr, batches[300], fill=0xFF)  # every float of it a NaN
    calls = {300: first, B: GuardedCall(tr, batches[B], ws=first.ws), 5: GuardedCall(tr, batches[5], ws=first.ws)}
    assert tr._workspace_size(tr.c, 5) < tr._workspace_size(tr.c, B) < first.ws.numel()
    for refill in (False, True):
        if refill:
            first.ws.fill_(0xFF)
        for b in B_WORKSPACE:
            for grad in (True, False, True):
                g, l = calls[b].run(grad)
                assert torch.equal(bits(l), bits(want[b][grad][1])), (refill, b, grad)
                assert not grad or torch.equal(bits(g), bits(want[b][True][0])), (refill, b, grad)
                G.check_flat(first.bufs["workspace"], "workspace")  # the other buffers' guards: GuardedCall.run


def test_one_trainer_across_batch_sizes_equals_fresh_trainers():
    """SlicedTrainer25.workspace(B) reallocates when B changes: B = 300, 37, 300 on one trainer, dropout on."""
    name = "c25"
    batches = {b: dev_batch(two_sided_batch(ROWS[name], b, SEED_BATCH)) for b in (300, B)}

    def call(tr, b):
        tr.calls = 0  # the same call counter: the same internal keep rule
        tr.params.grad.fill_(float("nan"))
        l_pol, l_val = tr.loss_and_grad(*batches[b])
        torch.cuda.synchronize()
        assert int(tr.status[0]) == 0 and torch.isfinite(tr.params.grad).all()
        return tr.params.grad.clone(), l_pol.clone(), l_val.clone()

    one = trainer(name, dropout_p=0.5)
    for b in (300, B, 300):
        for got, want in zip(call(one, b), call(trainer(name, dropout_p=0.5), b)):
            assert torch.equal(bits(got), bits(want)), b


# ---- 6. every row bad ------------------------------------------------------------------------------------------------
def test_every_row_bad_adds_no_policy_term():
    name, b, p = "odd25", 300, 0.5
    m = dims(ROWS[name])
    xx, ss, aa, rr = two_sided_batch(ROWS[name], b, SEED_BATCH)
    keep = keep_mask(5, 0, b, m, p)
    masks = multipliers(keep, p)

    def run(actions):
        tr = trainer(name, dropout_p=p)
        tr.workspace(b).fill_(0xFF)  # every float of it a NaN
        l_pol, l_val = tr.loss_and_grad(*dev_batch((xx, ss, actions, rr)), keep_in=torch.from_numpy(keep).to(DEV))
        torch.cuda.synchronize()
        return float(l_pol), float(l_val), gradient(tr, name), int(tr.status[0])

    clean = run(aa)
    assert clean[3] == 0
    rows = np.arange(b)  # every row bad, at a position of its own
    bad = aa.copy()
    bad[rows, rows % m["n_steps"]] = np.where(rows % 2, m["n_logits"] + rows % 100, -1 - rows % 100).astype(np.int8)
    assert ((bad < 0) | (bad >= m["n_logits"])).any(1).all()
    got = run(bad)
    assert got[3] == TG_TRAIN_STATUS_BAD_TOKEN
    assert got[0] == 0.0 and got[1] == clean[1]  # l_val bit for bit: position 0 sees START alone
    assert all(not got[2][k].any() for k in LI1)
    compare(name, f"B={b} every row bad", got[:3], (xx, ss, bad, rr), masks=masks, skip_rows=np.ones(b, bool))


# ---- 7. float32 frames with T > 1 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, b", [("t2_25", 5), ("a25", 2)])
def test_float32_frames_equal_int8_frames_bit_for_bit(name, b):
    assert dims(ROWS[name])["T"] > 1
    xx, ss, aa, rr = dev_batch(two_sided_batch(ROWS[name], b, SEED_BATCH))
    tr = trainer(name, dropout_p=0.5)
    runs = []
    for frames in (xx, xx.float()):
        tr.calls = 0  # the same call counter: the same internal keep rule
        tr.params.grad.fill_(float("nan"))
        l_pol, l_val = tr.loss_and_grad(frames, ss, aa, rr)
        runs.append((tr.params.grad.clone(), l_pol.clone(), l_val.clone()))
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0]).all() and xx.dtype == torch.int8 and int(tr.status[0]) == 0
    for x, y in zip(*runs):
        assert torch.equal(bits(x), bits(y))
