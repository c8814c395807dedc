"""The training loss and gradient at the 3x3 matmul tensor (S = TG_NET_WIDE_S = 9) on the MI355X, for the two S = 9
configurations of net_s9_ref: losses and every gradient tensor against train_ref's float64 autograd at B = 1, 37 and
256, with and without dropout, the internal keep rule, bitwise determinism, graph capture, learning against eager
float32, and the self-play loop at 3x3 (demos, search with net.policy, the replay data, a training epoch)."""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedTrainer, SyntheticDemos, TensorGameData, ops, search
from mat_mul_amd.train import unpack_weights

from net_ref import P, make_weights
from net_s9_ref import CONFIGS
from train_ref import TrainRef, keep_mask, make_batch, multipliers, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(CONFIGS)
TOL = 1e-4  # per tensor: |got - ref| <= TOL * max(1, max |ref|)


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(CONFIGS[name], 50 + CASES.index(name))


def trainer(name, dropout_p=0.0, seed=0):
    return FusedTrainer.from_state_dict(weights(name), dropout_p=dropout_p, seed=seed, device=DEV)


def dev_batch(batch):
    return tuple(torch.from_numpy(x).to(DEV) for x in batch)


def check_against_float64(name, B, p=0.0, seed=1, internal=False):
    cfg = CONFIGS[name]
    tr = trainer(name, dropout_p=p, seed=7)
    batch = make_batch(cfg, B, seed)
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


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("name", CASES)
def test_loss_and_gradient_match_float64_autograd(name, B):
    check_against_float64(name, B)


@pytest.mark.parametrize("B", [37, 256])
@pytest.mark.parametrize("name", CASES)
def test_dropout_with_a_host_mask_matches_float64_autograd(name, B):
    check_against_float64(name, B, p=0.5, seed=2)


@pytest.mark.parametrize("name", CASES)
def test_internal_keep_rule_matches_the_header_and_float64_autograd(name):
    check_against_float64(name, 37, p=0.5, seed=3, internal=True)


def test_gradients_are_bitwise_reproducible_and_graph_capture_equals_eager():
    tr = trainer("a9", dropout_p=0.5)
    m = tr.config
    B = 300  # two games for some of the 256 partial slabs
    batch = dev_batch(make_batch(CONFIGS["a9"], B, 3))
    ws = tr.workspace(B)
    grad = torch.empty_like(tr.params.detach())
    losses = torch.empty(2, dtype=torch.float32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    keep = torch.empty((B, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV)

    def run():
        ops.net_loss_grad(tr.c, tr.params.detach(), tr.pos_fix, *batch, ws, grad=grad, losses=losses, status=status,
                          dropout_p=0.5, seed=3, call_idx=4, keep_out=keep)

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


def test_learning_on_a_fixed_batch_tracks_eager_float32():
    cfg = CONFIGS["a9"]
    tr = trainer("a9")
    xx, ss, aa, rr = make_batch(cfg, 256, 30)
    # one token sequence for every game, which 100 steps can learn (random tokens keep a cross entropy near log 3 per
    # position, and the combined loss does not halve)
    aa[:] = np.arange(cfg["n_steps"]) % cfg["n_logits"]
    batch = (xx, ss, aa, rr)
    db = dev_batch(batch)
    opt = torch.optim.Adam([tr.params], lr=1e-3)
    fused = []
    for _ in range(100):
        lp, lv = tr.train_step(db, opt)
        fused.append(lp + tr.weight_val * lv)
    fused = torch.stack(fused).cpu().numpy().astype(np.float64)
    assert np.isfinite(fused).all() and fused[-1] < 0.5 * fused[0], (fused[0], fused[-1])
    ref = TrainRef(weights("a9"), cfg, device=DEV, dtype=torch.float32)
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


def _rank1_ternary(d):
    """Whether the int tensor d (S,S,S) is u (x) v (x) w with u, v, w in {-1, 0, 1}^S (zero included)."""
    if not d.any():
        return True
    if np.abs(d).max() > 1:
        return False
    i, j, k = np.argwhere(d)[0]
    u, v, w = d[:, j, k], d[i, :, k], d[i, j, :]
    return np.array_equal(np.einsum("a,b,c->abc", u, v, w), d)  # d[i,j,k]^2 = 1


@pytest.mark.parametrize("name", CASES)
def test_self_play_at_3x3(name):
    B, T, S, k, L = 64, CONFIGS[name]["dim_t"], 9, 8, 4
    tr = trainer(name, dropout_p=0.5)
    demos = SyntheticDemos(L, B, T, S, device=DEV, seed=11)
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.to(torch.int8)
    runs = []
    for _ in range(2):
        forest = search.SearchForest(B, S, T, k=k, max_actions=L, n_sim=4, device=DEV)
        out = search.actor_prediction(tr.net(k).policy(seed=5), start, L, n_sim=4, n_bar=100, n_logits=3, k=k,
                                      forest=forest)
        assert int(forest.status.abs().sum()) == 0
        runs.append([t.cpu() for t in out] + [forest.final_heads().cpu()])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    states, policy, rewards, lengths, final = runs[0]
    assert tuple(policy.shape) == (B, L, 3 * S, 3) and int(lengths.sum()) > 0
    heads = states[:, :, 0].numpy().astype(np.int64)
    for b in range(B):
        n = int(lengths[b])
        seq = [heads[b, m] for m in range(n)] + [final[b].numpy().astype(np.int64)]
        for m in range(n):
            assert _rank1_ternary(seq[m] - seq[m + 1]), (b, m)
    # the games go to the replay data, and one epoch of train_step on it learns
    data = TensorGameData(demos.action_seq.to(torch.int8), demos.target_tensor.to(torch.int8), 64, 0.5, dim_t=T,
                          max_actions=L, seed=0)
    data.add_act_step(*(t.to(DEV) for t in (states, policy, rewards, lengths)))
    p0 = tr.params.detach().clone()
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    losses = []
    for batch in data.batches(16, generator=gen):
        losses += list(tr.train_step(batch, opt))
    assert torch.isfinite(torch.stack(losses)).all() and len(losses) == 8
    assert not torch.equal(p0, tr.params.detach()) and torch.isfinite(tr.params).all()
    assert int(data.status[0]) == 0
