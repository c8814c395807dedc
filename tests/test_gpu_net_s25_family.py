"""The fused network at the 5x5 matmul tensor (S = 25, FusedAlphaTensor25) on the MI355X across the rows of
tests/net_s25_family.FAMILY25: inference against the float64 restatement at B = 1 and 11 (275 torso workgroups) and, at
e25 and f25, against the reference's own recorded float64 outputs at the fixture's states; the sampling rule with given
uniforms into guarded outputs and with the internal stream; that a sample does not depend on the workgroup it is decoded
in (R rows of a game per workgroup, a partial last one; r8_25 at k = 8, 9, 16 and 20 too); input dtypes, row subsets
and empty batches; guard bytes around every output; the row mask where a game is 25 torso and up to 64 decoder
workgroups; and the refusals of the partners just outside the family and of the class of the other sizes.

The bound is the suite's: 1e-5 * max(1, max |ref|) per tensor, with ``train_ref.within``'s fallback (twice the eager
float32 restatement's error where that itself misses the bound; tests/test_net_s25_family_cpu.py shows that it has no
reason to trigger here).  The worst relative error per row is printed as FAMILY-ERR infer25 lines (run with -s).
Measured on the MI355X, the worst of the five tensors relative to max(1, max |ref|) at B = 1 / B = 11: c13_25 1.9e-7 /
2.7e-7, c20_25 5.8e-7 / 4.8e-7, e25 3.7e-7 / 4.5e-7, f25 4.5e-7 / 6.9e-7, lim25 2.3e-7 / 3.1e-7, odd25 3.1e-7 / 3.2e-7,
ones25 2.0e-7 / 2.5e-7, r8_25 3.0e-7 / 6.1e-7, t8_25 2.9e-7 / 4.7e-7; at the fixture's two states against the
restatement / the recorded reference: e25 4.7e-7 / 3.5e-7, f25 5.9e-7 / 2.6e-7.  No tensor took the float32 fallback.

With the team loops of softmax_rows_team and weighted_sum_team cut to their first 8 (row, head) rows, the sampling
tests of odd25, t8_25 and r8_25 fail (b. and c. below) and no other test of this file: the teacher-forced entries run
one row per workgroup, so R * heads > 8 is reached by sampling alone.  With wq = W in dec_plan, c13_25 and c20_25 fail
(a. to d., and the refused partner's byte count).
"""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedAlphaTensor25, ops
from mat_mul_amd._lib import TensorGameError

import net_s25_family as F
from guarded_buffers import GUARD, check_flat, guarded
from net_ref import Ref, dims, make_weights, philox_uniforms, pick
from net_s25_ref import EE_SLICES
from net_sampling import check_pp
from train_ref import err, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = sorted(F.FAMILY25)
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_s25_family_cases.npz"
TOL_INFER = 1e-5
KEYS = ("ee", "oo", "zz0", "q", "qq")
PATTERN = 0xA5
S, J = 25, 1875
SEED = 0x1234_5678_9ABC  # above 2^32: both seed words are in use
NEEDS = r"LDS plan needs {} \(torso\) / {} \(decoder\) bytes"


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(F.FAMILY25[name].cfg, F.seed(name))


@functools.lru_cache(maxsize=None)
def net(name):
    return FusedAlphaTensor25.from_state_dict(weights(name), F.FAMILY25[name].k, device=DEV)


@functools.lru_cache(maxsize=None)
def states(name, B):
    """B = "fixture": the recorded states of a reference row; otherwise net_s25_family.states.  Shared, never written."""
    if B == "fixture":
        f = fixture(name)
        return f["xx"], f["ss"], f["g_action"]
    return F.states(name, B)


@functools.lru_cache(maxsize=None)
def device_states(name, B):
    return tuple(torch.from_numpy(a).to(DEV) for a in states(name, B))


@functools.lru_cache(maxsize=None)
def host(name, B, dtype=torch.float64):
    """The restatement's outputs (ee, oo, zz0, q, qq) for states(name, B), as float64 numpy."""
    ref = Ref(weights(name), F.FAMILY25[name].cfg, device=DEV, dtype=dtype)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.detach().cpu().double().numpy()
            for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


# ---- a. inference ---------------------------------------------------------------------------------------------------
def run_inference(name, B):
    """The five tensors of the fused network for states(name, B), after the checks of shapes, dtypes and token range."""
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    fused = net(name)
    xx, ss, ga = device_states(name, B)
    n = xx.shape[0]
    ee = fused.torso(xx, ss)
    oo, zz0, q = fused.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = fused.fwd_infer(xx.float(), ss, seed=3, call=B if isinstance(B, int) else 0)
    for t, shape, dtype in ((ee, (n, J, m["c"]), torch.float32), (oo, (n, m["n_steps"], m["n_logits"]), torch.float32),
                            (zz0, (n, m["W"]), torch.float32), (q, (n, m["n_quantile"]), torch.float32),
                            (aa, (n, k, m["n_steps"]), torch.int64), (pp, (n, k), torch.float32),
                            (qq, (n,), torch.float32)):
        assert tuple(t.shape) == shape and t.dtype == dtype, (tuple(t.shape), t.dtype, shape, dtype)
    assert int(aa.min()) >= 0 and int(aa.max()) < m["n_logits"]
    assert bool(torch.isfinite(pp).all()) and float(pp.min()) >= 0.0 and float(pp.max()) <= 1.0
    return dict(ee=ee, oo=oo, zz0=zz0, q=q, qq=qq)


def kept_slices(ee):
    """Rows i*75 .. i*75 + 74 of the first state's torso output for i in EE_SLICES: what the fixture keeps of ee."""
    return ee[:1].reshape(1, S, 3 * S, -1)[:, list(EE_SLICES)]


def compare(name, B, got, want, what, view=lambda key, t: t):
    """Every tensor of ``got`` inside the suite's bound of ``want`` (float64 numpy); prints the relative errors.
    ``view`` takes the part of a full tensor that ``want`` holds (the recorded slices of ee)."""
    worst = 0.0
    for key in KEYS:
        ref = want[key]
        part = lambda t: view(key, t)[:ref.shape[0]]  # noqa: E731
        f32 = lambda: err(part(host(name, B, torch.float32)[key]), ref)  # noqa: E731
        e = err(part(got[key]), ref)
        rel = e / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, rel)
        print(f"FAMILY-ERR infer25 {name} B={B} {what} {key} {rel:.3g}")
        assert within(e, TOL_INFER, ref, f32, f"{name} B={B} {what} {key}"), (key, e)
    print(f"FAMILY-ERR infer25 {name} B={B} {what} worst {worst:.3g}")


@pytest.mark.parametrize("B", [1, 11])
@pytest.mark.parametrize("name", ROWS)
def test_inference_against_float64(name, B):
    compare(name, B, run_inference(name, B), host(name, B), "restatement")


@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_inference_against_the_recorded_reference(name):
    f = fixture(name)
    assert f["xx"].shape[0] >= 1 and int(f["seed"].item()) == F.seed(name) and tuple(f["ee_slices"]) == EE_SLICES
    got = run_inference(name, "fixture")
    compare(name, "fixture", got, host(name, "fixture"), "restatement")
    compare(name, "fixture", got, {key: f[f"{key}64"] for key in KEYS}, "recorded",
            view=lambda key, t: kept_slices(t) if key == "ee" else t)


# ---- b. the sampling rule -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampling_ee(name):
    """(the device's ee, the float64 restatement's ee) of the sampling tests' states."""
    xx, ss, _ = device_states(name, F.sample_states(name))
    return net(name).torso(xx, ss), torch.from_numpy(host(name, F.sample_states(name))["ee"]).to(DEV)


def host_check(name, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities of the device's own
    prefix, outside draws nearer than 1e-5 to a cumulative boundary (at most 1 % of all draws)."""
    m = dims(F.FAMILY25[name].cfg)
    ref = Ref(weights(name), m, device=DEV)
    B, k, n = tokens.shape
    ee = sampling_ee(name)[1].repeat_interleave(k, 0)
    tok = tokens.to(torch.int64).reshape(B * k, n)
    start = torch.full((B * k, 1), m["n_logits"], dtype=torch.long, device=DEV)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).cpu().numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    print(f"{name}: {(~keep).sum()} of {keep.size} draws within 1e-5 of a boundary")
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    check_pp(name, pp.cpu().numpy(), p_chosen.prod(-1), n)
    assert (~keep).sum() < 0.01 * keep.size


@pytest.mark.parametrize("name", ROWS)
def test_sampling_follows_the_host_rule(name):
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    fused, B, n = net(name), F.sample_states(name), m["n_steps"]
    ee = sampling_ee(name)[0]
    u = F.uniforms(name)
    bufs = [guarded((B, k, n), torch.int8), guarded((B, k), torch.float32), guarded((B,), torch.float32)]
    tokens, pp, q = ops.net_s25_sample(fused.c, fused.w, ee, torch.arange(B, device=DEV), k, 0, 0,
                                       uniforms=torch.from_numpy(u).to(DEV), tokens=bufs[0][1], probs=bufs[1][1],
                                       q=bufs[2][1])
    torch.cuda.synchronize()
    for (buf, _), what in zip(bufs, ("tokens", "probs", "q")):
        check_flat(buf, f"{name} {what}")
    assert tokens.data_ptr() == bufs[0][1].data_ptr() and tokens.dtype == torch.int8
    assert int(tokens.min()) >= 0 and int(tokens.max()) < m["n_logits"]
    host_check(name, tokens, pp, u.astype(np.float64))
    rows = torch.arange(B, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = fused.sample(ee, rows=rows, seed=SEED, call=41)
    u = philox_uniforms(SEED, rows.cpu().numpy(), 41, k, n)
    assert u.shape == (B, k, n)
    t2, p2, q2 = fused.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert torch.equal(q1.view(torch.int32), q2.view(torch.int32)) and torch.equal(q1, q)
    host_check(name, t1, p1, u)


# ---- c. a sample does not depend on how samples are grouped ---------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_a_sample_alone_equals_the_same_sample_among_k(name):
    """Samples s0 .. s0 + R - 1 of a game share a workgroup (R from tg_net_s25_sample's rule; the last workgroup holds
    fewer), and with k = 1 a sample is alone in its own.  mm_rb, layernorm, softmax_rows, softmax_rows_team and
    weighted_sum_team apply the same operations to a row in an order that involves neither R nor the row's place, so
    sample s of the full call and the same uniforms alone give the same tokens, probability and value bit for bit.  At
    r8_25 the first k of the 20 samples also come out the same at k = 8 (one full workgroup), 9 (8 + 1) and 16."""
    k = F.FAMILY25[name].k
    R, chunks, last, _ = F.geometry(name)
    fused = net(name)
    B = 3
    ee = sampling_ee(name)[0][:B].contiguous()
    u = torch.from_numpy(F.uniforms(name)[:B]).to(DEV)
    tokens, pp, q = fused.sample(ee, uniforms=u)
    picked = sorted({s for s in (0, R - 1, R, k - 1) if 0 <= s < k})
    assert picked[0] == 0 and picked[-1] == k - 1
    for s in picked:
        t1, p1, q1 = fused.sample(ee, uniforms=u[:, s:s + 1].contiguous(), k=1)
        assert tuple(t1.shape) == (B, 1, tokens.shape[2])
        assert torch.equal(t1[:, 0], tokens[:, s]), (name, s, "tokens")
        assert torch.equal(p1[:, 0].view(torch.int32), pp[:, s].view(torch.int32)), (name, s, "pp")
        assert torch.equal(q1.view(torch.int32), q.view(torch.int32)), (name, s, "q")
    if name == "r8_25":
        assert len({tuple(r.tolist()) for r in tokens[0]}) > 1  # the samples differ from each other
        for kk in (8, 9, 16, 20):
            assert F.geometry(name, kk)[0] == 8
            tk, pk, qk = fused.sample(ee, uniforms=u[:, :kk].contiguous(), k=kk)
            assert torch.equal(tk, tokens[:, :kk]), (name, kk, "tokens")
            assert torch.equal(pk.view(torch.int32), pp[:, :kk].view(torch.int32)), (name, kk, "pp")
            assert torch.equal(qk.view(torch.int32), q.view(torch.int32)), (name, kk, "q")


# ---- d. inputs and subsets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_int8_frames_row_subsets_and_empty_batches(name):
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    fused = net(name)
    xx, ss, _ = device_states(name, F.sample_states(name))
    xx, ss = xx[:6].contiguous(), ss[:6].contiguous()
    ee8, eef = fused.torso(xx, ss), fused.torso(xx.float(), ss)
    assert torch.equal(ee8.view(torch.int32), eef.view(torch.int32))
    rows = torch.arange(6, device=DEV, dtype=torch.int64) + 1000
    full = fused.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([5, 2, 0, 4], device=DEV)
    part = fused.sample(fused.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)
    one = fused.sample(fused.torso(xx[3:4], ss[3:4]), rows=rows[3:4], seed=4, call=2)  # B = 1
    for a, b in zip(full, one):
        assert torch.equal(a[3:4], b)
    ee0 = fused.torso(xx[:0], ss[:0])  # B = 0 is a no-op
    assert tuple(ee0.shape) == (0, J, m["c"])
    t0, p0, q0 = fused.sample(ee0, rows=rows[:0])
    assert tuple(t0.shape) == (0, k, m["n_steps"]) and tuple(p0.shape) == (0, k) and tuple(q0.shape) == (0,)
    ga0 = torch.zeros((0, m["n_steps"]), dtype=torch.int64, device=DEV)
    oo0, zz0, qq0 = ops.net_s25_logits(fused.c, fused.w, ee0, ga0)
    assert tuple(oo0.shape) == (0, m["n_steps"], m["n_logits"]) and zz0.numel() == 0 and qq0.numel() == 0


# ---- e. nothing outside the outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd25", "lim25", "c20_25"])
def test_nothing_is_written_outside_the_outputs(name):
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    fused, B = net(name), 5
    xx, ss, ga = (t[:B].contiguous() for t in device_states(name, 11))
    n, W = m["n_steps"], m["W"]
    bufs = {}

    def out(what, shape, dtype):
        bufs[what], t = guarded(shape, dtype)
        return t

    ee = ops.net_s25_torso(fused.c, fused.w, xx, ss, out=out("ee", (B, J, m["c"]), torch.float32))
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    tokens, probs, q = ops.net_s25_sample(fused.c, fused.w, ee, rows, k, 9, 1,
                                          tokens=out("tokens", (B, k, n), torch.int8),
                                          probs=out("probs", (B, k), torch.float32), q=out("q", (B,), torch.float32))
    # ops.net_s25_logits allocates its outputs: the same entry, by the same launch path, on guarded ones
    oo, zz0, qt = (out("oo", (B, n, m["n_logits"]), torch.float32), out("zz0", (B, W), torch.float32),
                   out("qt", (B, m["n_quantile"]), torch.float32))
    ga64 = ga.to(torch.int64).contiguous()
    ops._launch(torch.device(DEV), "tg_net_s25_logits", C.byref(fused.c), ops._ptr(fused.w), ops._ptr(ee),
                ops._ptr(ga64), B, ops._ptr(oo), ops._ptr(zz0), ops._ptr(qt))
    torch.cuda.synchronize()
    for what, buf in bufs.items():
        check_flat(buf, f"{name} {what}")
    want = (fused.torso(xx, ss),) + tuple(fused.sample(ee, rows=rows, seed=9, call=1)) + tuple(
        ops.net_s25_logits(fused.c, fused.w, ee, ga64))
    for got, ref, what in zip((ee, tokens, probs, q, oo, zz0, qt), want, ("ee", "tokens", "probs", "q", "oo", "zz0", "qt")):
        assert torch.equal(got, ref), (name, what)


# ---- f. the row mask ------------------------------------------------------------------------------------------------
def raw(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


@pytest.mark.parametrize("name", ["lim25", "odd25"])
def test_the_row_mask_over_many_workgroups_per_game(name):
    """A game is 25 slice workgroups in the torso and ceil(k / R) in the decoder (64 at lim25, 6 at odd25): all of them
    take the game's flags byte.  Active rows equal the plain call bit for bit; inactive rows keep the sentinel."""
    m, k = dims(F.FAMILY25[name].cfg), F.FAMILY25[name].k
    fused, B, need = net(name), 5, 129
    assert F.geometry(name)[1] == (64 if name == "lim25" else 6)
    xx, ss, _ = (t[:B].contiguous() for t in device_states(name, 11))
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    plain_ee = fused.torso(xx, ss)
    plain = (plain_ee,) + tuple(fused.sample(plain_ee, rows=rows, seed=5, call=7))
    shapes = (((B, J, m["c"]), torch.float32), ((B, k, m["n_steps"]), torch.int8), ((B, k), torch.float32),
              ((B,), torch.float32))
    for flags in ([129, 0, 1, 128, 0], [0, 128, 1, 0, 137], [129, 0, 255, 1, 129], [128, 129, 1, 137, 0]):
        active = [g for g, f in enumerate(flags) if (f & need) == need]
        fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
        bufs, outs = zip(*(guarded(s, d) for s, d in shapes))
        for b in bufs:
            b[GUARD:-GUARD].fill_(PATTERN)
        ee, tokens, probs, q = outs
        assert ops.net_s25_torso(fused.c, fused.w, xx, ss, out=ee, flags=fl, need=need).data_ptr() == ee.data_ptr()
        # ee holds the sentinel at inactive games: their decoder workgroups return before they read it
        ops.net_s25_sample(fused.c, fused.w, ee, rows, k, 5, 7, tokens=tokens, probs=probs, q=q, flags=fl, need=need)
        torch.cuda.synchronize()
        for b, got, want, what in zip(bufs, outs, plain, ("ee", "tokens", "probs", "q")):
            check_flat(b, what)
            got, want = raw(got), raw(want)
            for g in range(B):
                if g in active:
                    assert torch.equal(got[g], want[g]), (name, flags, what, g)
                else:
                    assert bool((got[g] == PATTERN).all()), (name, flags, what, g)


# ---- g. refusals on the device path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.OUTSIDE25))
def test_a_partner_outside_is_refused_on_the_device_path(name):
    m = F.outside(name)
    row = F.OUTSIDE25[name][0]
    torso, dec = F.inference_bytes(m)
    message = "n_steps=76 above TG_NET_WIDE3_MAX_STEPS=75" if name == "e25_n76" else NEEDS.format(torso, dec)
    assert name == "e25_n76" or torso <= F.LDS < dec
    with pytest.raises(TensorGameError, match=message) as e:
        FusedAlphaTensor25.from_state_dict(make_weights(m, 1), F.FAMILY25[row].k, device=DEV)
    assert e.value.code == -2  # TG_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ROWS)
def test_the_class_of_the_other_sizes_refuses_each_row_and_names_this_one(name):
    with pytest.raises(TensorGameError, match="TG_NET_MAX_S") as e:
        FusedAlphaTensor.from_state_dict(weights(name), F.FAMILY25[name].k, device=DEV)
    assert e.value.code == -2 and "FusedAlphaTensor25" in str(e.value) and "tensor_game_net_s25.h" in str(e.value)
    fused = net(name)
    xx, ss, _ = (t[:1] for t in device_states(name, 1))
    with pytest.raises(TensorGameError, match="FusedAlphaTensor25"):
        ops.net_torso(fused.c, fused.w, xx, ss)
