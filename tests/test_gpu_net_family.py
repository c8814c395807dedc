"""The fused network and its training on the MI355X across the supported family (tests/net_family.FAMILY): inference
against the reference's float64 outputs where they were recorded and the float64 restatement everywhere at B = 1, 16
and 37; the sampling rule at each row's samples per game (several workgroups per game, a partial last one); the
training loss and every gradient tensor against float64 autograd, with dropout (host masks and the internal keep rule
at W % 4 != 0); bitwise reproducible gradients; FusedTrainer's inference blob after an AdamW step.

Bounds are the suite's: 1e-5 * max(1, max |ref|) per inference tensor and 1e-4 per training tensor.  Where the eager
float32 restatement of the same inputs itself misses that bound against float64, the tensor's bound is twice that
eager float32 error, computed here (``train_ref.within``); the rows and tensors that used it are printed (run with -s), as are
the worst errors per row."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedTrainer, ops
from mat_mul_amd.net import pack_weights
from mat_mul_amd.train import unpack_weights

import net_family as F
from net_ref import P, Ref, dims, make_inputs, make_weights, philox_uniforms, pick
from train_ref import TrainRef, err, keep_mask, make_batch, multipliers, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = sorted(F.FAMILY)
TRAIN_ROWS = [n for n in ROWS if F.FAMILY[n].train]
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_family_cases.npz"
TOL_INFER, TOL_TRAIN = 1e-5, 1e-4


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name not in F.REFERENCE_ROWS:
        return None
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


def seed(name):
    f = fixture(name)
    return int(f["seed"].item()) if f is not None else 80 + ROWS.index(name)


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(F.FAMILY[name].cfg, seed(name))


@functools.lru_cache(maxsize=None)
def states(name, B):
    """The fixture's states at B = 16 where one was recorded; otherwise make_inputs'; with their g_action."""
    m = dims(F.FAMILY[name].cfg)
    f = fixture(name)
    if B == 16 and f is not None:
        return f["xx"], f["ss"], f["g_action"]
    xx, ss = make_inputs(m, B, 500 + B)
    ga = np.random.default_rng(600 + B).integers(0, m["n_logits"], size=(B, m["n_steps"])).astype(np.int8)
    return xx, ss, ga


@functools.lru_cache(maxsize=None)
def host(name, B, dtype=torch.float64):
    """The restatement's outputs (ee, oo, zz0, q, qq) for states(name, B), as float64 numpy."""
    ref = Ref(weights(name), F.FAMILY[name].cfg, device=DEV, dtype=dtype)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.detach().cpu().double().numpy()
            for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


def net(name, k=None):
    return FusedAlphaTensor.from_state_dict(weights(name), k or F.FAMILY[name].k, device=DEV)


# ---- inference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 37])
@pytest.mark.parametrize("name", ROWS)
def test_inference_against_float64(name, B):
    m = dims(F.FAMILY[name].cfg)
    fused = net(name)
    xx, ss, ga = (torch.from_numpy(a).to(DEV) for a in states(name, B))
    oo, zz0, q = fused.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = fused.fwd_infer(xx.float(), ss, seed=3)
    k = F.FAMILY[name].k
    assert tuple(aa.shape) == (B, k, m["n_steps"]) and tuple(pp.shape) == (B, k)
    assert int(aa.min()) >= 0 and int(aa.max()) < m["n_logits"]
    h, f = host(name, B), fixture(name)
    for got, key in ((fused.torso(xx, ss), "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        f32 = lambda: err(host(name, B, torch.float32)[key], h[key])  # noqa: E731
        e = err(got, h[key])
        print(f"FAMILY-ERR infer {name} B={B} {key} {e / max(1.0, float(np.abs(h[key]).max())):.3g}")
        assert within(e, TOL_INFER, h[key], f32, f"{name} B={B} {key}"), (key, e)
        if B == 16 and f is not None:  # the reference's own float64 outputs of the first states
            rec = f[f"{key}64"]
            assert within(err(got[:rec.shape[0]], rec), TOL_INFER, rec, f32, f"{name} recorded {key}"), key


# ---- sampling ---------------------------------------------------------------------------------------------------------
def host_check(name, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities."""
    m = dims(F.FAMILY[name].cfg)
    ref = Ref(weights(name), m, device=DEV)
    B, k, n = tokens.shape
    ee = torch.from_numpy(host(name, 16)["ee"]).to(DEV).repeat_interleave(k, 0)
    tok = tokens.to(torch.int64).reshape(B * k, n)
    start = torch.full((B * k, 1), m["n_logits"], dtype=torch.long, device=DEV)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).cpu().numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    np.testing.assert_allclose(pp.cpu().numpy(), p_chosen.prod(-1), rtol=1e-5, atol=0)
    assert (~keep).sum() < 0.01 * keep.size


@pytest.mark.parametrize("name", ROWS)
def test_sampling_follows_the_host_rule(name):
    m, k = dims(F.FAMILY[name].cfg), F.FAMILY[name].k
    fused = net(name)
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, 16))
    ee = fused.torso(xx, ss)
    u = np.random.default_rng(5).random((16, k, m["n_steps"])).astype(np.float32)
    tokens, pp, _ = fused.sample(ee, uniforms=torch.from_numpy(u).to(DEV))
    assert tuple(tokens.shape) == (16, k, m["n_steps"])
    host_check(name, tokens, pp, u.astype(np.float64))
    rows = torch.arange(16, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = fused.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, m["n_steps"])
    t2, p2, q2 = fused.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    host_check(name, t1, p1, u)


@pytest.mark.parametrize("name", ROWS)
def test_int8_frames_and_row_subsets(name):
    fused = net(name)
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, 16))
    ee8, eef = fused.torso(xx, ss), fused.torso(xx.float(), ss)
    assert torch.equal(ee8, eef)
    rows = torch.arange(16, device=DEV, dtype=torch.int64) + 1000
    full = fused.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([15, 5, 7, 0, 10], device=DEV)
    part = fused.sample(fused.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)


# ---- training ---------------------------------------------------------------------------------------------------------
def trainer(name, dropout_p=0.0, seed=0):
    return FusedTrainer.from_state_dict(weights(name), dropout_p=dropout_p, seed=seed, device=DEV)


def check_training(name, B, p=0.0, batch_seed=1, internal=False):
    cfg = F.FAMILY[name].cfg
    tr = trainer(name, dropout_p=p, seed=7)
    m = tr.config
    batch = make_batch(cfg, B, batch_seed)
    dev = tuple(torch.from_numpy(x).to(DEV) for x in batch)
    if internal:  # the library's own keep rule, recorded through keep_out
        out = torch.empty((B, m["blocks"], 2, m["n_steps"], m["W"]), dtype=torch.uint8, device=DEV)
        l_pol, l_val = tr.loss_and_grad(*dev, keep_out=out)
        keep = out.cpu().numpy()
        assert np.array_equal(keep, keep_mask(7, 0, B, m, p))
    else:
        keep = keep_mask(5, 0, B, m, p) if p > 0 else None
        l_pol, l_val = tr.loss_and_grad(*dev, keep_in=None if keep is None else torch.from_numpy(keep).to(DEV))
    torch.cuda.synchronize()
    masks = None if keep is None else multipliers(keep, p)
    ref = TrainRef(weights(name), cfg, device=DEV).loss_grad(*batch, masks=masks)

    @functools.lru_cache(maxsize=None)
    def eager32():
        return TrainRef(weights(name), cfg, device=DEV, dtype=torch.float32).loss_grad(*batch, masks=masks)

    got = unpack_weights(tr.params.grad, m, np.zeros_like(weights(name)[P + "pos_enc_fix"]))
    assert sorted(ref[2]) == sorted(k for k in got if k != P + "pos_enc_fix")
    pairs = [("l_pol", float(l_pol), ref[0], lambda: eager32()[0]), ("l_val", float(l_val), ref[1], lambda: eager32()[1])]
    pairs += [(k, got[k].numpy(), g, functools.partial(lambda k: eager32()[2][k], k)) for k, g in ref[2].items()]
    worst, bad = 0.0, {}
    for key, value, want, want32 in pairs:
        e = err(value, want)
        worst = max(worst, e / max(1.0, float(np.abs(want).max())))
        if not within(e, TOL_TRAIN, want, lambda: err(want32(), want), f"{name} B={B} p={p} {key}"):
            bad[key] = e
    print(f"FAMILY-ERR train {name} B={B} p={p} internal={internal} {worst:.3g}")
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("name", TRAIN_ROWS)
def test_loss_and_gradient_match_float64_autograd(name, B):
    check_training(name, B)


@pytest.mark.parametrize("name", [n for n in ("e", "g") if n in TRAIN_ROWS])
def test_loss_and_gradient_match_float64_autograd_over_the_partial_slabs(name):
    check_training(name, 300)  # 256 slabs, 44 of them with two games


@pytest.mark.parametrize("name", ["e", "odd"])
def test_dropout_at_an_uneven_width(name):
    assert dims(F.FAMILY[name].cfg)["W"] % 4
    check_training(name, 37, p=0.5, batch_seed=2)
    check_training(name, 37, p=0.5, batch_seed=3, internal=True)


def test_gradients_are_bitwise_reproducible_at_the_decoder_plan_limit():
    tr = trainer("g", dropout_p=0.5)
    B = 300
    batch = tuple(torch.from_numpy(x).to(DEV) for x in make_batch(F.FAMILY["g"].cfg, B, 3))
    ws = tr.workspace(B)
    losses = torch.empty(2, dtype=torch.float32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    grads = []
    for _ in range(2):
        grad = torch.full_like(tr.params.detach(), float("nan"))
        ops.net_loss_grad(tr.c, tr.params.detach(), tr.pos_fix, *batch, ws, grad=grad, losses=losses, status=status,
                          dropout_p=0.5, seed=3, call_idx=4)
        grads.append(grad)
    torch.cuda.synchronize()
    assert torch.isfinite(grads[0]).all() and int(status[0]) == 0
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))


def test_trainer_blob_after_an_adamw_step_equals_the_packed_state_dict():
    name = "odd"
    tr = trainer(name, dropout_p=0.5)
    batch = tuple(torch.from_numpy(x).to(DEV) for x in make_batch(F.FAMILY[name].cfg, 37, 4))
    p0 = tr.params.detach().clone()
    opt = torch.optim.AdamW([tr.params], lr=1e-3)
    l_pol, l_val = tr.train_step(batch, opt)
    assert torch.isfinite(l_pol) and torch.isfinite(l_val)
    assert not torch.equal(p0, tr.params.detach())
    want = torch.from_numpy(pack_weights(tr.state_dict(), tr.config))
    assert torch.equal(tr.net().w.cpu().view(torch.int32), want.view(torch.int32))
