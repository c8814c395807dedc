"""The training loss and gradient at the 5x5 matmul tensor (S = 25, include/tensor_game_train_s25.h) on the MI355X:
losses and every gradient tensor against train_ref's float64 autograd across the slab and chunk shapes (one decoder
slab with 25 torso slabs, torso runs that straddle games, a decoder workgroup with two games, one chunk in both
attention blocks, a partial last chunk in either), with and without dropout and with the internal keep rule; bitwise
reproducibility and graph capture; the loss-only call; int8 against float32 frames; bad tokens; a stale workspace;
learning against eager float32; the train / act / replay loop at 5x5; save and resume.

The bound is the suite's (test_gpu_train_s9, test_gpu_train_s16): per tensor |got - ref| <= 1e-4 * max(1, max |ref|).
Where a tensor misses it, train_ref.compare_grads decides: it also admits an error no larger than twice eager float32's
own against float64 where that one misses the bound too, and prints both figures."""
import functools
import types

import numpy as np
import pytest
import torch

from mat_mul_amd import (FusedAlphaTensor25, SlicedTrainer25, SyntheticDemos, TensorGameData, load_run, ops, save_run,
                         search)
from mat_mul_amd._lib import TG_TRAIN_STATUS_BAD_TOKEN
from mat_mul_amd.train import unpack_weights

from net_ref import P, make_weights
from net_s25_train_family import ROWS
from train_ref import (GuardedCall, TrainRef, bad_tokens, compare_grads, keep_mask, make_batch, multipliers, rel_err)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4  # per tensor: |got - ref| <= TOL * max(1, max |ref|)
S = 25


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(ROWS[name], 250 + sorted(ROWS).index(name))


def trainer(name, dropout_p=0.0, seed=0):
    return SlicedTrainer25.from_state_dict(weights(name), dropout_p=dropout_p, seed=seed, device=DEV)


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def compare(tr, name, l_pol, l_val, batch, keep, p, skip_rows=None):
    masks = None if keep is None else multipliers(keep, p)
    ref = TrainRef(weights(name), ROWS[name], device=DEV)
    rp, rv, rg = ref.loss_grad(*batch, masks=masks, skip_rows=skip_rows)
    got = unpack_weights(tr.params.grad, tr.config, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    assert sorted(rg) == sorted(k for k in got if k != P + "pos_enc_fix")
    worst = {k: rel_err(got[k].numpy(), g) for k, g in rg.items()}
    what = f"{name} B={batch[0].shape[0]} p={p}"
    print(f"{what}: l_pol {rel_err(float(l_pol), rp):.3g} l_val {rel_err(float(l_val), rv):.3g} "
          f"worst tensor {max(worst, key=worst.get)} {max(worst.values()):.3g}")
    if max(rel_err(float(l_pol), rp), rel_err(float(l_val), rv), *worst.values()) < TOL:
        return
    ref32 = TrainRef(weights(name), ROWS[name], device=DEV, dtype=torch.float32)
    r32 = ref32.loss_grad(*batch, masks=masks, skip_rows=skip_rows)
    compare_grads("S25", what, (float(l_pol), float(l_val), {k: got[k].numpy() for k in rg}), (rp, rv, rg), r32, TOL)


def check_against_float64(name, B, p=0.0, seed=1, internal=False):
    tr = trainer(name, dropout_p=p, seed=7)
    batch = make_batch(ROWS[name], B, seed)
    m = tr.config
    if internal:  # the library's own keep rule, recorded through keep_out
        out = torch.empty((B, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV)
        l_pol, l_val = tr.loss_and_grad(*dev_batch(batch), keep_out=out)
        keep = out.cpu().numpy()
        assert np.array_equal(keep, keep_mask(7, 0, B, m, p))
    else:
        keep = keep_mask(5, 0, B, m, p) if p > 0 else None
        l_pol, l_val = tr.loss_and_grad(*dev_batch(batch),
                                        keep_in=None if keep is None else torch.from_numpy(keep).to(DEV))
    torch.cuda.synchronize()
    assert int(tr.status[0]) == 0
    compare(tr, name, l_pol, l_val, batch, keep, p)


# a25 at B = 1: one decoder slab, 25 torso slabs; a25 at B = 11: 275 units on 256 torso workgroups, runs of one and of
# two units; c25 at B = 15: 375 units, four runs straddle games; c25 at B = 257: one decoder workgroup takes two games;
# one25, odd25: one chunk in both blocks; xtail25: a partial last chunk in the cross-attention; stail25: a partial last
# chunk in the self-attention (test_train_s25_cpu asserts that the shapes reach these runs and chunks)
SHAPES = [("a25", 1), ("a25", 11), ("c25", 15), ("c25", 257), ("one25", 3), ("odd25", 3), ("xtail25", 3), ("stail25", 3)]


@pytest.mark.parametrize("name,B", SHAPES)
def test_loss_and_gradient_match_float64_autograd(name, B):
    check_against_float64(name, B)


@pytest.mark.parametrize("name,B", SHAPES)
def test_dropout_with_a_host_mask_matches_float64_autograd(name, B):
    check_against_float64(name, B, p=0.5, seed=2)


@pytest.mark.parametrize("name,B", SHAPES)
def test_internal_keep_rule_matches_the_header_and_float64_autograd(name, B):
    check_against_float64(name, B, p=0.5, seed=3, internal=True)


def raw_call(tr, batch, B, **kw):
    m = tr.config
    out = dict(grad=torch.empty_like(tr.params.detach()), losses=torch.empty(2, dtype=torch.float32, device=DEV),
               status=torch.empty(1, dtype=torch.int32, device=DEV),
               keep=torch.empty((B, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV))

    def run(grad=out["grad"]):
        ops.net_loss_grad_s25(tr.c, tr.params.detach(), tr.pos_fix, *batch, tr.workspace(B), grad=grad,
                              losses=out["losses"], status=out["status"], dropout_p=0.5, seed=3, call_idx=4,
                              keep_out=out["keep"], **kw)
    return out, run


def test_gradients_are_bitwise_reproducible_and_graph_capture_equals_eager():
    tr = trainer("c25", dropout_p=0.5)
    B = 263  # B * S = 6575 units, no multiple of the 256 torso workgroups; 7 decoder workgroups take two games
    batch = dev_batch(make_batch(ROWS["c25"], B, 3))
    o, run = raw_call(tr, batch, B)
    grad, losses, keep, status = o["grad"], o["losses"], o["keep"], o["status"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
        first = grad.clone()
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), grad.view(torch.int32))
    eager = (grad.clone(), losses.clone(), keep.clone())
    grad.zero_()
    losses.zero_()
    keep.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad.view(torch.int32), eager[0].view(torch.int32))
    assert torch.equal(losses, eager[1]) and torch.equal(keep, eager[2])
    assert int(status[0]) == 0


def test_the_loss_only_call_returns_the_same_losses_and_leaves_grad_alone():
    tr = trainer("c25", dropout_p=0.5)
    B = 21
    g = GuardedCall(tr, dev_batch(make_batch(ROWS["c25"], B, 4)))
    _, with_grad = g.run()
    poison = torch.full_like(g.grad, 12345.0)
    g.grad.copy_(poison)
    tr._loss_grad(tr.c, tr.params.detach(), tr.pos_fix, *g.batch, g.ws, grad=None, losses=g.losses, status=g.status,
                  dropout_p=0.5, seed=3, call_idx=4, keep_out=g.keep)
    torch.cuda.synchronize()
    assert torch.equal(g.losses.view(torch.int32), with_grad.view(torch.int32))
    assert torch.equal(g.grad, poison) and int(g.status[0]) == 0
    _, alone = g.run(grad=False)  # every buffer between guard bytes
    assert torch.equal(alone.view(torch.int32), with_grad.view(torch.int32))


def test_int8_and_float32_frames_give_identical_bits():
    tr = trainer("c25", dropout_p=0.5)
    B = 5
    xx, ss, aa, rr = dev_batch(make_batch(ROWS["c25"], B, 5))
    res = []
    for frames in (xx, xx.to(torch.float32)):
        o, run = raw_call(tr, (frames, ss, aa, rr), B)
        run()
        torch.cuda.synchronize()
        res.append((o["grad"].clone(), o["losses"].clone()))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))


def test_bad_tokens_skip_their_rows_and_set_the_status():
    name, B = "c25", 300
    tr = trainer(name)
    xx, ss, aa, rr = make_batch(ROWS[name], B, 6)
    bad, skip = bad_tokens(aa, tr.config["n_logits"])
    l_pol, l_val = tr.loss_and_grad(*dev_batch((xx, ss, bad, rr)))
    torch.cuda.synchronize()
    assert int(tr.status[0]) == TG_TRAIN_STATUS_BAD_TOKEN
    compare(tr, name, l_pol, l_val, (xx, ss, bad, rr), None, 0.0, skip_rows=skip)
    tr.loss_and_grad(*dev_batch((xx[:8], ss[:8], aa[:8], rr[:8])))
    assert int(tr.status[0]) == 0  # a clean batch afterwards


def test_a_stale_workspace_gives_the_same_bits():
    """The workspace full of NaN patterns (0xFF bytes) before the call against one full of zeros: two games per decoder
    workgroup, so the second game's dL/d ln2(ee) accumulator and saved block inputs start from the first game's."""
    tr = trainer("c25", dropout_p=0.5)
    batch = dev_batch(make_batch(ROWS["c25"], 260, 7))
    clean = GuardedCall(tr, batch, fill=0).run()
    stale = GuardedCall(tr, batch, fill=0xFF)
    assert torch.isnan(stale.ws.view(torch.float32)).all()
    for want, got in zip(clean, stale.run()):
        assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    for want, got in zip(clean, stale.run()):  # and once more on what the first call left
        assert torch.equal(want.view(torch.int32), got.view(torch.int32))


def test_learning_on_a_fixed_batch_tracks_eager_float32():
    """Five Adam steps: the combined loss of the fused step against eager float32 autograd under the suite's rtol 2e-3
    (test_gpu_train_s16)."""
    cfg = ROWS["c25"]
    tr = trainer("c25")
    xx, ss, aa, rr = make_batch(cfg, 8, 30)
    aa[:] = np.arange(75) % 3  # one token sequence for every game
    batch = (xx, ss, aa, rr)
    db = dev_batch(batch)
    opt = torch.optim.AdamW([tr.params], lr=1e-3, weight_decay=0.0)
    fused = []
    for _ in range(5):
        lp, lv = tr.train_step(db, opt)
        fused.append(lp + tr.weight_val * lv)
    fused = torch.stack(fused).cpu().numpy().astype(np.float64)
    assert np.isfinite(fused).all(), fused
    ref = TrainRef(weights("c25"), cfg, device=DEV, dtype=torch.float32)
    ropt = torch.optim.AdamW([v for v in ref.w.values() if v.requires_grad], lr=1e-3, weight_decay=0.0)
    eager = []
    for _ in range(5):
        ropt.zero_grad()
        lp, lv = ref.losses(*batch)
        loss = lp + 1000.0 * lv
        loss.backward()
        ropt.step()
        eager.append(loss.item())
    print("fused", fused, "eager", eager)
    assert fused[-1] < fused[0]
    np.testing.assert_allclose(fused, eager, rtol=2e-3)


def _model(name, n_samples, p):
    """What ``from_model`` reads of a reference ``AlphaTensor``: the state_dict, the device, n_samples and the
    PredictBlock dropout."""
    sd = {k: torch.from_numpy(v) for k, v in weights(name).items()}
    block = types.SimpleNamespace(dropout1=types.SimpleNamespace(p=p))
    head = types.SimpleNamespace(predict_action_logits=types.SimpleNamespace(blocks=[block]))
    return types.SimpleNamespace(state_dict=lambda: sd, device=torch.device("cpu"), n_samples=n_samples,
                                 policy_head=head)


def test_the_loop_at_5x5():
    """from_model, one train_step, net() acting with the new weights in the search, the replay data; afterwards the
    trainer's shared inference blob and a fresh FusedAlphaTensor25 from its state_dict sample the same tokens and agree
    on the values within 1e-6 (the two fold pos_enc + pos_enc_fix with different roundings, as at 4x4)."""
    name, B, T, k, L = "c25", 4, 1, 4, 3
    tr = SlicedTrainer25.from_model(_model(name, k, 0.5), seed=3)
    assert type(tr) is SlicedTrainer25 and tr.dropout_p == 0.5 and tr.n_samples == k and tr.config["S"] == S
    p0 = tr.params.detach().clone()
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    losses = tr.train_step(dev_batch(make_batch(ROWS[name], B, 9)), opt)
    assert torch.isfinite(torch.stack(list(losses))).all() and int(tr.status[0]) == 0
    assert not torch.equal(p0, tr.params.detach()) and torch.isfinite(tr.params).all()
    net = tr.net()
    assert type(net) is FusedAlphaTensor25
    demos = SyntheticDemos(L, B, T, S, device=DEV, seed=11)
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.to(torch.int8).reshape(B, S, S, S)
    forest = search.SearchForest(B, S, T, k=k, max_actions=L, n_sim=2, device=DEV)
    states, policy, rewards, lengths = search.actor_prediction(net.policy(seed=5), start, L, n_sim=2, n_bar=100,
                                                               n_logits=3, k=k, forest=forest)
    assert int(forest.status.abs().sum()) == 0 and int(lengths.sum()) > 0
    data = TensorGameData(demos.action_seq.to(torch.int8), demos.target_tensor.to(torch.int8), B * L, 0.5, dim_t=T,
                          max_actions=L, seed=0)
    data.add_act_step(states, policy, rewards, lengths)
    assert int(data.status[0]) == 0
    fresh = FusedAlphaTensor25.from_state_dict(tr.state_dict(), k, device=DEV)
    scal = torch.zeros((B, tr.config["dim_s"]), dtype=torch.float32, device=DEV)
    a = tr.net().fwd_infer(start, scal, seed=9)  # a network of its own call counter, as fresh is
    b = fresh.fwd_infer(start, scal, seed=9)
    for x, y in zip(a, b):
        if x.dtype.is_floating_point:
            assert float((x - y).abs().max()) <= 1e-6 * max(1.0, float(y.abs().max()))
        else:
            assert torch.equal(x, y)


def test_save_and_resume(tmp_path):
    name, B, T, L = "c25", 4, 1, 3
    tr = trainer(name, dropout_p=0.5, seed=3)
    demos = SyntheticDemos(L, B, T, S, device=DEV, seed=12)
    data = TensorGameData(demos.action_seq.to(torch.int8), demos.target_tensor.to(torch.int8), B * L, 0.5, dim_t=T,
                          max_actions=L, seed=0)
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    xx, ss, aa, rr = dev_batch(make_batch(ROWS[name], B, 8))
    tr.train_step((xx, ss, aa, rr), opt)
    save_run(tmp_path / "run", tr, opt, data)
    run = load_run(tmp_path / "run", DEV)
    assert type(run.trainer) is SlicedTrainer25
    opt2 = torch.optim.AdamW([run.trainer.params], lr=1e-4)
    opt2.load_state_dict(run.optimizer_state)
    want = tr.train_step((xx, ss, aa, rr), opt)
    got = run.trainer.train_step((xx, ss, aa, rr), opt2)
    torch.cuda.synchronize()
    assert torch.equal(tr.params.detach().view(torch.int32), run.trainer.params.detach().view(torch.int32))
    for w, g in zip(want, got):
        assert torch.equal(w.view(torch.int32), g.view(torch.int32))
