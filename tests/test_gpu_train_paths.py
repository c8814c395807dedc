"""Paths of the training kernels (mat_mul_amd/csrc/tg_train.hip, include/tensor_game_train.h) that the other training
tests share one value of, on the MI355X, each against train_ref's float64 autograd under the suite's bound
(train_ref.within: 1e-4 * max(1, max |ref|) per tensor, or twice the eager float32 restatement's own error where that
misses the bound too):

1. each loss alone: weight_pol and weight_val away from (1, 1000), with the exact zeros the kernel promises;
2. the quantile loss's four branches (quadratic or linear, either sign of g_value - q), away from the kinks;
3. the S = 9 training torso with a partial last chunk and with nine chunks of one (net_family.CHUNKED);
4. the gradient when rows hold a token outside [0, n_logits);
5. float32 frames, bitwise equal to int8 frames;
6. a workspace of exactly tg_net_train_workspace_size bytes between guard bytes, and one full of 0xFF bytes (NaN);
7. the run partition B * p / P around TG_NET_TRAIN_PARTIALS = 256.

Rewards are two-sided (train_ref.two_sided_rewards) throughout.  tests/test_train_paths_cpu.py shows on the CPU that
these inputs reach the paths and tell wrong losses from the right one.  Each check prints (run with -s) a
TRAIN-PATHS-ERR line: the worst error of a tensor over that tensor's own max |ref| (no floor of 1), for the fused
kernels and for eager float32."""
import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedTrainer, ops
from mat_mul_amd.train import unpack_weights

import guarded_buffers as G
import net_family as F
from net_ref import P, Ref, dims
from train_ref import GuardedCall as Call
from train_ref import (TrainRef, bad_tokens, compare_grads, err, keep_mask, multipliers, two_sided_batch,
                       value_branches, within)
from test_train_paths_cpu import B, ROWS_BRANCH, ROWS_WEIGHTS, SEED_BATCH, SEED_BRANCH, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_INFER, TOL_TRAIN = 1e-5, 1e-4
LI1 = (P + "li1.weight", P + "li1.bias")


def trainer(name, **kw):
    return FusedTrainer.from_state_dict(weights(name), **dict(dict(dropout_p=0.0, seed=7, device=DEV), **kw))


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def gradient(tr, name):
    """The trainer's gradient as a reference-format dict of numpy arrays."""
    got = unpack_weights(tr.params.grad, tr.config, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    return {k: v.numpy() for k, v in got.items() if k != P + "pos_enc_fix"}


def compare(name, what, got, batch, **kw):
    """got = (l_pol, l_val, {name: gradient}) of the fused kernels against TrainRef.loss_grad(*batch, **kw) in float64
    under the suite's bound; returns the float64 reference."""
    cfg = F.train_config(name)
    ref = TrainRef(weights(name), cfg, device=DEV).loss_grad(*batch, **kw)
    ref32 = TrainRef(weights(name), cfg, device=DEV, dtype=torch.float32).loss_grad(*batch, **kw)
    compare_grads("TRAIN-PATHS-ERR", f"{name} {what}", got, ref, ref32, TOL_TRAIN)
    return ref


def fused(name, batch, grad=True, **kw):
    """(l_pol, l_val, gradient dict or None, trainer) of one call on ``batch`` (numpy)."""
    tr = trainer(name, **{k: kw.pop(k) for k in ("weight_pol", "weight_val", "dropout_p") if k in kw})
    l_pol, l_val = (tr.loss_and_grad if grad else tr.losses)(*dev_batch(batch), **kw)
    torch.cuda.synchronize()
    return float(l_pol), float(l_val), gradient(tr, name) if grad else None, tr


# ---- 1. each loss alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wpol, wval", [(16.0, 0.0), (0.0, 8000.0), (0.25, 3.0)])
@pytest.mark.parametrize("name", ROWS_WEIGHTS)
def test_each_loss_alone(name, wpol, wval):
    batch = two_sided_batch(F.train_config(name), B, SEED_BATCH)
    got = fused(name, batch, weight_pol=wpol, weight_val=wval)
    # the losses compared are the unweighted l_pol and l_val, whatever the weights
    compare(name, f"B={B} weights=({wpol:g}, {wval:g})", got[:3], batch, weight_pol=wpol, weight_val=wval)
    if wval == 0.0:  # the loss gradient is multiplied by the weight before anything else
        zero = [k for k in got[2] if k.startswith("value_head.")]
        assert len(zero) == 8 and all(not got[2][k].any() for k in zero)
    if wpol == 0.0:
        assert all(not got[2][k].any() for k in LI1)


# ---- 2. the value branches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_BRANCH)
def test_value_loss_branches(name):
    cfg = F.train_config(name)
    batch = two_sided_batch(cfg, B, SEED_BRANCH)
    shares, margin = value_branches(TrainRef(weights(name), cfg, device=DEV), *batch)
    assert min(shares.values()) >= 0.10, shares
    assert margin >= 1e-4, margin  # ten times the inference bound on q: float32 cannot change a branch
    compare(name, f"B={B} branches", fused(name, batch)[:3], batch)


# ---- 3. the S = 9 chunk tails ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, B])
@pytest.mark.parametrize("name", sorted(F.CHUNKED))
def test_chunked_torso_with_a_partial_last_chunk(name, b):
    batch = two_sided_batch(F.train_config(name), b, SEED_BATCH)
    l_pol, l_val, grad, tr = fused(name, batch)
    compare(name, f"B={b} chunk={F.CHUNKS[name]}", (l_pol, l_val, grad), batch)
    if b == B:  # the loss-only call: launches 1, 2 (stopping after the losses) and 4
        lp0, lv0 = tr.losses(*dev_batch(batch))
        assert float(lp0) == l_pol and float(lv0) == l_val


def test_chunked_row_inference_torso():
    name = "c5"
    cfg = F.train_config(name)
    xx, ss, _, _ = two_sided_batch(cfg, B, SEED_BATCH)
    net = FusedAlphaTensor.from_state_dict(weights(name), F.CHUNKED[name].k, device=DEV)
    ee = net.torso(torch.from_numpy(xx).to(DEV), torch.from_numpy(ss).to(DEV))
    want = Ref(weights(name), cfg, device=DEV).torso(xx, ss).cpu().numpy()
    f32 = lambda: err(Ref(weights(name), cfg, device=DEV, dtype=torch.float32).torso(xx, ss), want)  # noqa: E731
    assert within(err(ee, want), TOL_INFER, want, f32, f"{name} ee")


# ---- 4. bad tokens ---------------------------------------------------------------------------------------------------
def test_bad_token_rows_add_nothing_to_the_policy_gradient():
    name, b, p = "a", 300, 0.5
    cfg = F.train_config(name)
    m = dims(cfg)
    xx, ss, aa, rr = two_sided_batch(cfg, b, SEED_BATCH)
    keep = keep_mask(5, 0, b, m, p)
    kw = dict(dropout_p=p, keep_in=torch.from_numpy(keep).to(DEV))
    masks = multipliers(keep, p)
    clean = fused(name, (xx, ss, aa, rr), **kw)
    assert int(clean[3].status[0]) == 0
    bad, skip = bad_tokens(aa, m["n_logits"])
    got = fused(name, (xx, ss, bad, rr), **kw)
    assert int(got[3].status[0]) == 1
    assert got[1] == clean[1]  # l_val, bit for bit: position 0 sees START alone
    compare(name, f"B={b} bad tokens", got[:3], (xx, ss, bad, rr), masks=masks, skip_rows=skip)
    # every row bad, at a position of its own
    rows = np.arange(b)
    bad = aa.copy()
    bad[rows, rows % m["n_steps"]] = np.where(rows % 2, m["n_logits"] + rows % 100, -1 - rows % 100).astype(np.int8)
    got = fused(name, (xx, ss, bad, rr), **kw)
    assert int(got[3].status[0]) == 1
    assert got[0] == 0.0 and got[1] == clean[1]
    assert all(not got[2][k].any() for k in LI1)
    compare(name, f"B={b} every row bad", got[:3], (xx, ss, bad, rr), masks=masks, skip_rows=np.ones(b, bool))


# ---- 5. float32 frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "e", "a9", "c2"])
def test_float32_frames_equal_int8_frames_bit_for_bit(name):
    xx, ss, aa, rr = dev_batch(two_sided_batch(F.train_config(name), B, SEED_BATCH))
    tr = trainer(name, dropout_p=0.5)
    runs = []
    for frames in (xx, xx.float()):
        tr.calls = 0  # the same call counter: the same internal keep rule
        tr.params.grad.fill_(float("nan"))
        l_pol, l_val = tr.loss_and_grad(frames, ss, aa, rr)
        runs.append((tr.params.grad.clone(), l_pol.clone(), l_val.clone()))
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0]).all() and xx.dtype == torch.int8
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 6. the workspace and the output buffers -------------------------------------------------------------------------
# Call: ops.net_loss_grad on a trainer's weights with the workspace, grad, losses, status and keep_out each between guard
# bytes; the workspace defaults to exactly net_train_workspace_size bytes.
@pytest.mark.parametrize("name", ["odd", "c5"])
def test_exact_workspace_between_guards_and_a_workspace_of_nans(name):
    tr = trainer(name)
    cfg = F.train_config(name)
    big, small = (dev_batch(two_sided_batch(cfg, b, SEED_BATCH)) for b in (300, B))
    first = Call(tr, big, fill=0xFF)  # every float of it a NaN
    first.run()
    # B = 37 in the workspace B = 300 left behind, against a fresh zeroed one of exactly its size
    used, fresh = Call(tr, small, ws=first.ws), Call(tr, small, fill=0)
    assert fresh.ws.numel() == ops.net_train_workspace_size(tr.c, B) < first.ws.numel()
    want = {grad: fresh.run(grad) for grad in (True, False)}
    for refill in (False, True):  # what B = 300 left behind, then NaNs again
        if refill:
            first.ws.fill_(0xFF)
        for grad in (True, False):
            g, l = used.run(grad)
            assert torch.equal(l.view(torch.int32), want[grad][1].view(torch.int32))
            assert not grad or torch.equal(g.view(torch.int32), want[grad][0].view(torch.int32))
    G.check_flat(first.bufs["workspace"], "workspace")


# ---- 7. the run partition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [255, 256, 257, 513])
def test_run_partition_around_the_number_of_slabs(b):
    name = "b"
    batch = two_sided_batch(F.train_config(name), b, SEED_BATCH)
    l_pol, l_val, grad, tr = fused(name, batch)
    compare(name, f"B={b} partition", (l_pol, l_val, grad), batch)
    if b == 513:
        first = tr.params.grad.clone()
        tr.params.grad.zero_()
        again = tr.loss_and_grad(*dev_batch(batch))
        assert torch.equal(first.view(torch.int32), tr.params.grad.view(torch.int32))
        assert float(again[0]) == l_pol and float(again[1]) == l_val
