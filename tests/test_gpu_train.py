"""The training loss and gradient on the MI355X (include/tensor_game_train.h, mat_mul_amd.train), for the three
configurations of net_ref: losses and every gradient tensor against train_ref's float64 autograd, with and without
dropout, bitwise determinism, the internal keep rule, loss-only calls, bad tokens, FusedTrainer with a torch optimizer,
learning, one self-play epoch on the device and graph capture."""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedTrainer, TensorGameData, ops, search
from mat_mul_amd.net import infer_config, pack_weights
from mat_mul_amd.train import unpack_weights

from net_ref import CONFIGS, P, Ref, make_weights
from train_ref import TrainRef, keep_mask, make_batch, multipliers, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(CONFIGS)
TOL = 1e-4  # per tensor: |got - ref| <= TOL * max(1, max |ref|)


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(CONFIGS[name], 40 + CASES.index(name))


def trainer(name, dropout_p=0.0, seed=0):
    return FusedTrainer.from_state_dict(weights(name), dropout_p=dropout_p, seed=seed, device=DEV)


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def check_against_float64(name, B, p=0.0, seed=1):
    cfg = CONFIGS[name]
    tr = trainer(name, dropout_p=p)
    batch = make_batch(cfg, B, seed)
    keep = keep_mask(5, 0, B, tr.config, p) if p > 0 else None
    l_pol, l_val = tr.loss_and_grad(*dev_batch(batch), keep_in=None if keep is None else torch.from_numpy(keep).to(DEV))
    torch.cuda.synchronize()
    ref = TrainRef(weights(name), cfg, device=DEV)
    rp, rv, rg = ref.loss_grad(*batch, masks=None if keep is None else multipliers(keep, p))
    assert rel_err(float(l_pol), rp) < TOL, (float(l_pol), rp)
    assert rel_err(float(l_val), rv) < TOL, (float(l_val), rv)
    got = unpack_weights(tr.params.grad, tr.config, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    worst = {k: rel_err(got[k].numpy(), g) for k, g in rg.items()}
    bad = {k: e for k, e in worst.items() if not e < TOL}
    assert not bad, bad
    assert sorted(rg) == sorted(k for k in got if k != P + "pos_enc_fix")
    return max(worst.values())


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("name", CASES)
def test_loss_and_gradient_match_float64_autograd(name, B):
    check_against_float64(name, B)


def test_loss_and_gradient_match_float64_autograd_large_batch():
    check_against_float64("a", 4096)


@pytest.mark.parametrize("B", [7, 300])
@pytest.mark.parametrize("name", CASES)
def test_dropout_with_a_host_mask_matches_float64_autograd(name, B):
    check_against_float64(name, B, p=0.5, seed=2)


def test_gradients_are_bitwise_reproducible():
    tr = trainer("a", dropout_p=0.5)
    batch = dev_batch(make_batch(CONFIGS["a"], 300, 3))
    keep = torch.empty((300, 2, 2, 12, 32), dtype=torch.uint8, device=DEV)
    tr.loss_and_grad(*batch, keep_out=keep)
    g1 = tr.params.grad.clone()
    tr.calls = 0
    tr.params.grad.zero_()
    tr.loss_and_grad(*batch)
    assert torch.equal(g1.view(torch.int32), tr.params.grad.view(torch.int32))
    tr.params.grad.zero_()
    tr.loss_and_grad(*batch, keep_in=keep)  # the recorded mask reproduces the internal stream's call
    assert torch.equal(g1.view(torch.int32), tr.params.grad.view(torch.int32))


@pytest.mark.parametrize("name", CASES)
def test_internal_keep_rule_matches_the_header(name):
    p, B, seed = 0.5, 64, 123
    tr = trainer(name, dropout_p=p, seed=seed)
    tr.calls = 9
    m = tr.config
    keep = torch.empty((B, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV)
    tr.loss_and_grad(*dev_batch(make_batch(CONFIGS[name], B, 4)), keep_out=keep)
    got = keep.cpu().numpy()
    assert np.array_equal(got, keep_mask(seed, 9, B, m, p))
    n = got.size
    assert abs(got.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)
    assert tr.calls == 10


def test_loss_only_call_and_bad_tokens():
    cfg = CONFIGS["a"]
    tr = trainer("a")
    batch = list(dev_batch(make_batch(cfg, 7, 5)))
    lp, lv = tr.loss_and_grad(*batch)
    lp0, lv0 = tr.losses(*batch)
    assert float(lp) == float(lp0) and float(lv) == float(lv0)
    assert int(tr.status[0]) == 0
    # per-row policy losses of the float64 restatement, to find what row 3 adds
    ref = TrainRef(weights("a"), cfg)
    xx, ss, aa, rr = (x.cpu().numpy() for x in batch)
    rows = [ref.losses(xx[i:i + 1], ss[i:i + 1], aa[i:i + 1], rr[i:i + 1])[0].item() for i in range(7)]
    bad = batch[2].clone()
    bad[3, 5] = 3  # == n_logits: outside [0, n_logits)
    lpb, lvb = tr.losses(batch[0], batch[1], bad, batch[3])
    assert int(tr.status[0]) == 1
    assert float(lvb) == float(lv0)
    assert rel_err(float(lpb), sum(rows) - rows[3]) < TOL
    g_before = tr.params.grad.clone()
    tr.loss_and_grad(batch[0], batch[1], bad, batch[3])
    assert int(tr.status[0]) == 1 and torch.isfinite(tr.params.grad).all()
    bad[3, 5] = -7
    tr.losses(batch[0], batch[1], bad, batch[3])
    assert int(tr.status[0]) == 1
    tr.losses(*batch)
    assert int(tr.status[0]) == 0
    assert not torch.equal(g_before, tr.params.grad)


def test_adamw_steps_keep_the_inference_blob_and_the_state_dict_in_step():
    cfg = CONFIGS["a"]
    tr = trainer("a", dropout_p=0.5)
    fix0 = tr.pos_fix.clone()
    opt = torch.optim.AdamW([tr.params], lr=1e-3)
    for k in range(4):
        tr.train_step(dev_batch(make_batch(cfg, 64, 10 + k)), opt)
    sd = tr.state_dict()
    assert torch.equal(tr.pos_fix, fix0)
    assert np.array_equal(sd[P + "pos_enc_fix"].numpy(), weights("a")[P + "pos_enc_fix"])
    net = tr.net()
    blob = pack_weights(sd, infer_config(sd))
    assert np.array_equal(net.w.cpu().numpy().view(np.int32), blob.view(np.int32))
    w0 = weights("a")
    assert sorted(sd) == sorted(w0) and all(tuple(sd[k].shape) == w0[k].shape for k in w0)
    assert not np.array_equal(sd[P + "pos_enc"].numpy(), w0[P + "pos_enc"])  # pos_enc trained
    # the trained weights drive the float64 restatement to the fused network's logits
    xx, ss, aa, _ = make_batch(cfg, 5, 20)
    oo, _ = net.logits(torch.from_numpy(xx).to(DEV), torch.from_numpy(ss).to(DEV), torch.from_numpy(aa).to(DEV))
    ref = Ref({k: v.numpy() for k, v in sd.items()}, cfg)
    roo, _, _ = ref.teacher(ref.torso(xx, ss), aa)
    assert rel_err(oo.cpu().numpy(), roo.numpy()) < 1e-5


def test_learning_on_a_fixed_batch_tracks_eager_float32():
    cfg = CONFIGS["a"]
    tr = trainer("a")
    batch = make_batch(cfg, 256, 30)
    db = dev_batch(batch)
    opt = torch.optim.Adam([tr.params], lr=1e-3)
    fused = []
    for _ in range(200):
        lp, lv = tr.train_step(db, opt)
        fused.append(lp + tr.weight_val * lv)
    fused = torch.stack(fused).cpu().numpy().astype(np.float64)
    assert np.isfinite(fused).all() and fused[-1] < 0.5 * fused[0], (fused[0], fused[-1])
    ref = TrainRef(weights("a"), cfg, device=DEV, dtype=torch.float32)
    ropt = torch.optim.Adam([v for v in ref.w.values() if v.requires_grad], lr=1e-3)
    eager = []
    for _ in range(10):
        ropt.zero_grad()
        lp, lv = ref.losses(*batch)
        loss = lp + 1000.0 * lv
        loss.backward()
        ropt.step()
        eager.append(loss.item())
    np.testing.assert_allclose(fused[:10], eager, rtol=2e-3)


def test_one_self_play_epoch_on_the_device(golden):
    g = golden("replay_cases")
    tr = trainer("a", dropout_p=0.5)
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    data = TensorGameData(torch.from_numpy(g["mix_tokens"]).to(DEV, torch.int8),
                          torch.from_numpy(g["mix_targets"]).to(DEV, torch.int8), 40, 0.9, dim_t=2, max_actions=4,
                          seed=0)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    losses = []
    for epoch in range(2):
        for batch in data.batches(16, generator=gen):
            losses += list(tr.train_step(batch, opt))
        B, S, T = 8, 4, 2
        start = torch.from_numpy(np.random.default_rng(epoch).integers(-1, 2, size=(B, T, S, S, S)).astype(
            np.int8)).to(DEV)
        states, policy, rewards, lengths = search.actor_prediction(tr.net().policy(seed=epoch), start, 4, n_sim=8,
                                                                   n_bar=100, n_logits=3, k=tr.n_samples)
        data.add_act_step(states, policy, rewards, lengths)
    assert torch.isfinite(torch.stack(losses)).all()
    assert torch.isfinite(tr.params).all() and torch.isfinite(tr.net().w).all()


def test_graph_capture_equals_the_eager_call():
    cfg = CONFIGS["a"]
    tr = trainer("a", dropout_p=0.5)
    m = tr.config
    batch = dev_batch(make_batch(cfg, 33, 40))
    keep = torch.empty((33, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV)
    ws = tr.workspace(33)
    grad = torch.empty_like(tr.params.detach())
    losses = torch.empty(2, dtype=torch.float32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)

    def run():
        ops.net_loss_grad(tr.c, tr.params.detach(), tr.pos_fix, *batch, ws, grad=grad, losses=losses, status=status,
                          dropout_p=0.5, seed=3, call_idx=4, keep_out=keep)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
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
