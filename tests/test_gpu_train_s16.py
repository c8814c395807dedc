"""The training loss and gradient at the 4x4 matmul tensor (S = 16, include/tensor_game_train_sliced.h) on the MI355X:
losses and every gradient tensor against train_ref's float64 autograd across the slab and chunk shapes (one decoder
slab with 16 torso slabs, torso runs that straddle games, a decoder workgroup with two games, one chunk, a partial last
chunk), with and without dropout and with the internal keep rule; bitwise reproducibility and graph capture; the
loss-only call; int8 against float32 frames; bad tokens; learning against eager float32; the train / act / replay loop
at 4x4; save and resume.

The bound is the suite's (test_gpu_train_s9): per tensor |got - ref| <= 1e-4 * max(1, max |ref|)."""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, SlicedTrainer, SyntheticDemos, TensorGameData, load_run, ops, save_run, search
from mat_mul_amd._lib import TG_TRAIN_STATUS_BAD_TOKEN
from mat_mul_amd.train import unpack_weights

from net_ref import P, make_weights
from net_s16_train_family import ROWS
from train_ref import TrainRef, bad_tokens, keep_mask, make_batch, multipliers, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4  # per tensor: |got - ref| <= TOL * max(1, max |ref|)


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(ROWS[name], 160 + sorted(ROWS).index(name))


def trainer(name, dropout_p=0.0, seed=0):
    return SlicedTrainer.from_state_dict(weights(name), dropout_p=dropout_p, seed=seed, device=DEV)


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def compare(tr, name, l_pol, l_val, batch, keep, p, skip_rows=None):
    ref = TrainRef(weights(name), ROWS[name], device=DEV)
    rp, rv, rg = ref.loss_grad(*batch, masks=None if keep is None else multipliers(keep, p), skip_rows=skip_rows)
    got = unpack_weights(tr.params.grad, tr.config, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    worst = {k: rel_err(got[k].numpy(), g) for k, g in rg.items()}
    print(f"{name} B={batch[0].shape[0]} p={p}: l_pol {rel_err(float(l_pol), rp):.3g} l_val {rel_err(float(l_val), rv):.3g} "
          f"worst tensor {max(worst, key=worst.get)} {max(worst.values()):.3g}")
    assert rel_err(float(l_pol), rp) < TOL, (float(l_pol), rp)
    assert rel_err(float(l_val), rv) < TOL, (float(l_val), rv)
    bad = {k: e for k, e in worst.items() if not e < TOL}
    assert not bad, bad
    assert sorted(rg) == sorted(k for k in got if k != P + "pos_enc_fix")


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


# a16 at B = 1: one decoder slab, 16 torso slabs; a16 at B = 19: 304 units on 256 torso workgroups, runs that straddle
# games; b16 at B = 257: one decoder workgroup takes two games; odd16, c13, ones16: one chunk; tail16: a partial last chunk
SHAPES = [("a16", 1), ("a16", 19), ("b16", 257), ("odd16", 5), ("c13", 5), ("ones16", 5), ("t8", 5), ("tail16", 5)]


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
        ops.net_loss_grad_sliced(tr.c, tr.params.detach(), tr.pos_fix, *batch, tr.workspace(B), grad=grad,
                                 losses=out["losses"], status=out["status"], dropout_p=0.5, seed=3, call_idx=4,
                                 keep_out=out["keep"], **kw)
    return out, run


def test_gradients_are_bitwise_reproducible_and_graph_capture_equals_eager():
    tr = trainer("b16", dropout_p=0.5)
    B = 273  # B * S = 4368 units, no multiple of the 256 torso workgroups; 17 decoder workgroups take two games
    batch = dev_batch(make_batch(ROWS["b16"], B, 3))
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
    tr = trainer("b16", dropout_p=0.5)
    B = 21
    batch = dev_batch(make_batch(ROWS["b16"], B, 4))
    o, run = raw_call(tr, batch, B)
    run()
    torch.cuda.synchronize()
    with_grad = o["losses"].clone()
    poison = torch.full_like(o["grad"], 12345.0)
    o["grad"].copy_(poison)
    o["losses"].zero_()
    run(grad=None)
    torch.cuda.synchronize()
    assert torch.equal(o["losses"].view(torch.int32), with_grad.view(torch.int32))
    assert torch.equal(o["grad"], poison) and int(o["status"][0]) == 0


def test_int8_and_float32_frames_give_identical_bits():
    tr = trainer("b16", dropout_p=0.5)
    B = 5
    xx, ss, aa, rr = dev_batch(make_batch(ROWS["b16"], B, 5))
    res = []
    for frames in (xx, xx.to(torch.float32)):
        o, run = raw_call(tr, (frames, ss, aa, rr), B)
        run()
        torch.cuda.synchronize()
        res.append((o["grad"].clone(), o["losses"].clone()))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))


def test_bad_tokens_skip_their_rows_and_set_the_status():
    name, B = "b16", 300
    tr = trainer(name)
    xx, ss, aa, rr = make_batch(ROWS[name], B, 6)
    bad, skip = bad_tokens(aa, tr.config["n_logits"])
    l_pol, l_val = tr.loss_and_grad(*dev_batch((xx, ss, bad, rr)))
    torch.cuda.synchronize()
    assert int(tr.status[0]) == TG_TRAIN_STATUS_BAD_TOKEN
    compare(tr, name, l_pol, l_val, (xx, ss, bad, rr), None, 0.0, skip_rows=skip)
    tr.loss_and_grad(*dev_batch((xx[:8], ss[:8], aa[:8], rr[:8])))
    assert int(tr.status[0]) == 0  # a clean batch afterwards


def test_learning_on_a_fixed_batch_tracks_eager_float32():
    cfg = ROWS["a16"]
    tr = trainer("a16")
    xx, ss, aa, rr = make_batch(cfg, 16, 30)
    aa[:] = np.arange(cfg["n_steps"]) % cfg["n_logits"]  # one token sequence for every game
    batch = (xx, ss, aa, rr)
    db = dev_batch(batch)
    opt = torch.optim.Adam([tr.params], lr=1e-3)
    fused = []
    for _ in range(20):
        lp, lv = tr.train_step(db, opt)
        fused.append(lp + tr.weight_val * lv)
    fused = torch.stack(fused).cpu().numpy().astype(np.float64)
    assert np.isfinite(fused).all(), fused
    ref = TrainRef(weights("a16"), cfg, device=DEV, dtype=torch.float32)
    ropt = torch.optim.Adam([v for v in ref.w.values() if v.requires_grad], lr=1e-3)
    eager = []
    for _ in range(5):
        ropt.zero_grad()
        lp, lv = ref.losses(*batch)
        loss = lp + 1000.0 * lv
        loss.backward()
        ropt.step()
        eager.append(loss.item())
    print("fused", fused[:5], "eager", eager)
    np.testing.assert_allclose(fused[:5], eager, rtol=2e-3)


def test_the_loop_at_4x4():
    """Demos, search with net().policy, the replay data, one epoch of train_step; afterwards the trainer's shared
    inference blob and a fresh FusedAlphaTensor from its state_dict sample the same tokens and agree on the values
    within 1e-6.  Bit equality is not claimed for the values: the fresh network folds pos_enc + pos_enc_fix in float64
    and rounds once (tensor_game_net.h), refresh() adds in float32, and the two roundings can differ in the last bit."""
    name, B, T, S, k, L = "b16", 16, ROWS["b16"]["dim_t"], 16, 4, 4
    tr = trainer(name, dropout_p=0.5)
    demos = SyntheticDemos(L, B, T, S, device=DEV, seed=11)
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.to(torch.int8)
    forest = search.SearchForest(B, S, T, k=k, max_actions=L, n_sim=4, device=DEV)
    states, policy, rewards, lengths = search.actor_prediction(tr.net(k).policy(seed=5), start, L, n_sim=4, n_bar=100,
                                                               n_logits=3, k=k, forest=forest)
    assert int(forest.status.abs().sum()) == 0 and int(lengths.sum()) > 0
    data = TensorGameData(demos.action_seq.to(torch.int8), demos.target_tensor.to(torch.int8), 64, 0.5, dim_t=T,
                          max_actions=L, seed=0)
    data.add_act_step(states, policy, rewards, lengths)
    p0 = tr.params.detach().clone()
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    losses = []
    for batch in data.batches(16, generator=gen):
        losses += list(tr.train_step(batch, opt))
    assert len(losses) > 0 and torch.isfinite(torch.stack(losses)).all()
    assert not torch.equal(p0, tr.params.detach()) and torch.isfinite(tr.params).all()
    assert int(data.status[0]) == 0
    fresh = FusedAlphaTensor.from_state_dict(tr.state_dict(), k, device=DEV)
    scal = torch.zeros((B, tr.config["dim_s"]), dtype=torch.float32, device=DEV)
    a = tr.net(k).fwd_infer(start, scal, seed=9)
    b = fresh.fwd_infer(start, scal, seed=9)
    for x, y in zip(a, b):
        if x.dtype.is_floating_point:
            assert float((x - y).abs().max()) <= 1e-6 * max(1.0, float(y.abs().max()))
        else:
            assert torch.equal(x, y)


def test_save_and_resume(tmp_path):
    name, B, T, S, L = "b16", 8, ROWS["b16"]["dim_t"], 16, 4
    tr = trainer(name, dropout_p=0.5, seed=3)
    demos = SyntheticDemos(L, B, T, S, device=DEV, seed=12)
    data = TensorGameData(demos.action_seq.to(torch.int8), demos.target_tensor.to(torch.int8), B * L, 0.5, dim_t=T,
                          max_actions=L, seed=0)
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    xx, ss, aa, rr = dev_batch(make_batch(ROWS[name], B, 8))
    tr.train_step((xx, ss, aa, rr), opt)
    save_run(tmp_path / "run", tr, opt, data)
    run = load_run(tmp_path / "run", DEV)
    assert type(run.trainer) is SlicedTrainer
    opt2 = torch.optim.AdamW([run.trainer.params], lr=1e-4)
    opt2.load_state_dict(run.optimizer_state)
    want = tr.train_step((xx, ss, aa, rr), opt)
    got = run.trainer.train_step((xx, ss, aa, rr), opt2)
    torch.cuda.synchronize()
    assert torch.equal(tr.params.detach().view(torch.int32), run.trainer.params.detach().view(torch.int32))
    for w, g in zip(want, got):
        assert torch.equal(w.view(torch.int32), g.view(torch.int32))
