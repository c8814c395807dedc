"""The fused network at the 4x4 matmul tensor (S = 16) on the MI355X across the rows of tests/net_s16_family.FAMILY16:
inference against the float64 restatement at B = 1 and 37 and, at e16 and f16, against the reference's own recorded
float64 outputs at the fixture's states; the sampling rule with given uniforms and with the internal stream; that a
sample does not depend on the workgroup it is decoded in (R rows of a game per workgroup, a partial last one); input
dtypes, row subsets and empty batches; guard bytes around every output; the row mask where a game is 16 torso and up to
64 decoder workgroups; and the slice kernel against the per-game kernel over the small-S rows of net_family.FAMILY.

The bound is the suite's: 1e-5 * max(1, max |ref|) per tensor, with ``train_ref.within``'s fallback (twice the eager
float32 restatement's error where that itself misses the bound; tests/test_net_s16_family_cpu.py shows that it has no
reason to trigger here).  The worst relative error per row is printed as FAMILY-ERR lines (run with -s)."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, ops

import net_s16_family as F
from guarded_buffers import GUARD, check_flat, guarded
from net_ref import Ref, dims, make_weights, philox_uniforms, pick
from train_ref import err, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
ROWS = sorted(F.FAMILY16)
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_s16_family_cases.npz"
TOL_INFER = 1e-5
KEYS = ("ee", "oo", "zz0", "q", "qq")
PATTERN = 0xA5


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(F.FAMILY16[name].cfg, F.seed(name))


@functools.lru_cache(maxsize=None)
def net(name):
    return FusedAlphaTensor.from_state_dict(weights(name), F.FAMILY16[name].k, device=DEV)


@functools.lru_cache(maxsize=None)
def states(name, B):
    """B = "fixture": the recorded states of a reference row; otherwise net_s16_family.states.  Shared, never written."""
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
    ref = Ref(weights(name), F.FAMILY16[name].cfg, device=DEV, dtype=dtype)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.detach().cpu().double().numpy()
            for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


# ---- a. inference ---------------------------------------------------------------------------------------------------
def run_inference(name, B):
    """The five tensors of the fused network for states(name, B), after the checks of shapes, dtypes and token range."""
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
    fused = net(name)
    xx, ss, ga = device_states(name, B)
    n = xx.shape[0]
    ee = fused.torso(xx, ss)
    oo, zz0, q = fused.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = fused.fwd_infer(xx.float(), ss, seed=3, call=B if isinstance(B, int) else 0)
    for t, shape, dtype in ((ee, (n, 768, m["c"]), torch.float32), (oo, (n, m["n_steps"], m["n_logits"]), torch.float32),
                            (zz0, (n, m["W"]), torch.float32), (q, (n, m["n_quantile"]), torch.float32),
                            (aa, (n, k, m["n_steps"]), torch.int64), (pp, (n, k), torch.float32),
                            (qq, (n,), torch.float32)):
        assert tuple(t.shape) == shape and t.dtype == dtype, (tuple(t.shape), t.dtype, shape, dtype)
    assert int(aa.min()) >= 0 and int(aa.max()) < m["n_logits"]
    assert bool(torch.isfinite(pp).all()) and float(pp.min()) >= 0.0 and float(pp.max()) <= 1.0
    return dict(ee=ee, oo=oo, zz0=zz0, q=q, qq=qq)


def compare(name, B, got, want, what):
    """Every tensor of ``got`` inside the suite's bound of ``want`` (float64 numpy); prints the relative errors."""
    worst = 0.0
    for key in KEYS:
        ref = want[key]
        f32 = lambda: err(host(name, B, torch.float32)[key][:ref.shape[0]], ref)  # noqa: E731
        e = err(got[key][:ref.shape[0]], ref)
        rel = e / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, rel)
        print(f"FAMILY-ERR infer16 {name} B={B} {what} {key} {rel:.3g}")
        assert within(e, TOL_INFER, ref, f32, f"{name} B={B} {what} {key}"), (key, e)
    print(f"FAMILY-ERR infer16 {name} B={B} {what} worst {worst:.3g}")


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("name", ROWS)
def test_inference_against_float64(name, B):
    compare(name, B, run_inference(name, B), host(name, B), "restatement")


@pytest.mark.parametrize("name", F.REFERENCE_ROWS)
def test_inference_against_the_recorded_reference(name):
    f = fixture(name)
    assert f["xx"].shape[0] >= 1 and int(f["seed"].item()) == F.seed(name)
    got = run_inference(name, "fixture")
    compare(name, "fixture", got, host(name, "fixture"), "restatement")
    compare(name, "fixture", got, {key: f[f"{key}64"] for key in KEYS}, "recorded")


# ---- b. the sampling rule -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampling_ee(name):
    """(the device's ee, the float64 restatement's ee) of the sampling tests' states."""
    xx, ss, _ = device_states(name, F.sample_states(name))
    return net(name).torso(xx, ss), torch.from_numpy(host(name, F.sample_states(name))["ee"]).to(DEV)


def check_pp(name, pp, want, n_steps):
    """pp float32 against the float64 product ``want`` of a sample's n_steps probabilities: rtol = 1e-5 wherever float32
    holds the product as a normal number.  Below its smallest normal number (1.18e-38; at wide16 48 probabilities of 8
    logits come to about 1e-40) float32 is subnormal, with an absolute spacing of 2^-149 and no relative precision to
    speak of: each multiply of the running product then rounds by up to half a spacing, and the later factors, all
    below 1, only shrink the earlier roundings, so n_steps / 2 spacings bound their sum.  Only there is that added."""
    tiny = float(np.finfo(np.float32).tiny)
    sub = want < tiny
    print(f"{name}: {int(sub.sum())} of {sub.size} products are subnormal in float32")
    assert np.isfinite(pp).all() and (pp >= 0).all()
    bound = 1e-5 * np.abs(want) + np.where(sub, 0.5 * n_steps * 2.0 ** -149, 0.0)
    bad = np.abs(pp.astype(np.float64) - want) > bound
    assert not bad.any(), (name, pp[bad][:4], want[bad][:4])


def host_check(name, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities of the device's own
    prefix, outside draws nearer than 1e-5 to a cumulative boundary (at most 1 % of all draws)."""
    m = dims(F.FAMILY16[name].cfg)
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
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
    fused, B = net(name), F.sample_states(name)
    ee = sampling_ee(name)[0]
    u = F.uniforms(name)
    tokens, pp, _ = fused.sample(ee, uniforms=torch.from_numpy(u).to(DEV))
    assert tuple(tokens.shape) == (B, k, m["n_steps"]) and tokens.dtype == torch.int8
    assert int(tokens.min()) >= 0 and int(tokens.max()) < m["n_logits"]
    host_check(name, tokens, pp, u.astype(np.float64))
    rows = torch.arange(B, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = fused.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, m["n_steps"])
    t2, p2, q2 = fused.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    host_check(name, t1, p1, u)


# ---- c. a sample does not depend on how samples are grouped ---------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_a_sample_alone_equals_the_same_sample_among_k(name):
    """Samples s0 .. s0 + R - 1 of a game share a workgroup (R from launch_decode's rule; the last workgroup holds
    fewer), and with k = 1 a sample is alone in its own.  mm_rb, layernorm, softmax_rows and softmax_rows_team apply the
    same operations to a row in an order that involves neither R nor the row's place, so sample s of the full call and
    the same uniforms alone give the same tokens, probability and value bit for bit."""
    k = F.FAMILY16[name].k
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


# ---- d. inputs and subsets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_int8_frames_row_subsets_and_empty_batches(name):
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
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
    ee0 = fused.torso(xx[:0], ss[:0])  # B = 0 is a no-op
    assert tuple(ee0.shape) == (0, 768, m["c"])
    t0, p0, q0 = fused.sample(ee0, rows=rows[:0])
    assert tuple(t0.shape) == (0, k, m["n_steps"]) and tuple(p0.shape) == (0, k) and tuple(q0.shape) == (0,)
    ga0 = torch.zeros((0, m["n_steps"]), dtype=torch.int64, device=DEV)
    oo0, zz0, qq0 = ops.net_logits(fused.c, fused.w, ee0, ga0)
    assert tuple(oo0.shape) == (0, m["n_steps"], m["n_logits"]) and zz0.numel() == 0 and qq0.numel() == 0


# ---- e. nothing outside the outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd16", "wide16", "t8"])
def test_nothing_is_written_outside_the_outputs(name):
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
    fused, B = net(name), 5
    xx, ss, ga = (t[:B].contiguous() for t in device_states(name, 37))
    n, W = m["n_steps"], m["W"]
    bufs = {}

    def out(what, shape, dtype):
        bufs[what], t = guarded(shape, dtype)
        return t

    ee = ops.net_torso(fused.c, fused.w, xx, ss, out=out("ee", (B, 768, m["c"]), torch.float32))
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    tokens, probs, q = ops.net_sample(fused.c, fused.w, ee, rows, k, 9, 1, tokens=out("tokens", (B, k, n), torch.int8),
                                      probs=out("probs", (B, k), torch.float32), q=out("q", (B,), torch.float32))
    # ops.net_logits allocates its outputs: the same entry, by the same launch path, on guarded ones
    oo, zz0, qt = (out("oo", (B, n, m["n_logits"]), torch.float32), out("zz0", (B, W), torch.float32),
                   out("qt", (B, m["n_quantile"]), torch.float32))
    ga64 = ga.to(torch.int64).contiguous()
    ops._launch(torch.device(DEV), "tg_net_logits", C.byref(fused.c), ops._ptr(fused.w), ops._ptr(ee),
                ops._ptr(ga64), B, ops._ptr(oo), ops._ptr(zz0), ops._ptr(qt))
    torch.cuda.synchronize()
    for what, buf in bufs.items():
        check_flat(buf, f"{name} {what}")
    want = (fused.torso(xx, ss),) + tuple(fused.sample(ee, rows=rows, seed=9, call=1)) + tuple(
        ops.net_logits(fused.c, fused.w, ee, ga64))
    for got, ref, what in zip((ee, tokens, probs, q, oo, zz0, qt), want, ("ee", "tokens", "probs", "q", "oo", "zz0", "qt")):
        assert torch.equal(got, ref), (name, what)


# ---- f. the row mask ------------------------------------------------------------------------------------------------
def raw(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


@pytest.mark.parametrize("name", ["wide16", "odd16"])
def test_the_row_mask_over_many_workgroups_per_game(name):
    """A game is 16 slice workgroups in the torso and ceil(k / R) in the decoder (64 at wide16, 3 at odd16): all of them
    take the game's flags byte.  Active rows equal the plain call bit for bit; inactive rows keep the sentinel."""
    m, k = dims(F.FAMILY16[name].cfg), F.FAMILY16[name].k
    fused, B, need = net(name), 5, 129
    assert F.geometry(name)[1] == (64 if name == "wide16" else 3)
    xx, ss, _ = (t[:B].contiguous() for t in device_states(name, 37))
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    plain_ee = fused.torso(xx, ss)
    plain = (plain_ee,) + tuple(fused.sample(plain_ee, rows=rows, seed=5, call=7))
    shapes = (((B, 768, m["c"]), torch.float32), ((B, k, m["n_steps"]), torch.int8), ((B, k), torch.float32),
              ((B,), torch.float32))
    for flags in ([129, 0, 1, 128, 0], [0, 128, 1, 0, 137], [129, 0, 255, 1, 129], [128, 129, 1, 137, 0]):
        active = [g for g, f in enumerate(flags) if (f & need) == need]
        fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
        bufs, outs = zip(*(guarded(s, d) for s, d in shapes))
        for b in bufs:
            b[GUARD:-GUARD].fill_(PATTERN)
        ee, tokens, probs, q = outs
        assert ops.net_torso(fused.c, fused.w, xx, ss, out=ee, flags=fl, need=need).data_ptr() == ee.data_ptr()
        # ee holds the sentinel at inactive games: their decoder workgroups return before they read it
        ops.net_sample(fused.c, fused.w, ee, rows, k, 5, 7, tokens=tokens, probs=probs, q=q, flags=fl, need=need)
        torch.cuda.synchronize()
        for b, got, want, what in zip(bufs, outs, plain, ("ee", "tokens", "probs", "q")):
            check_flat(b, what)
            got, want = raw(got), raw(want)
            for g in range(B):
                if g in active:
                    assert torch.equal(got[g], want[g]), (name, flags, what, g)
                else:
                    assert bool((got[g] == PATTERN).all()), (name, flags, what, g)


# ---- g. the slice kernel against the per-game kernel at the sizes both run (the A/B library's switch) ---------------
SMALL_ROWS = ("e", "g", "odd", "ones", "f")  # net_family.FAMILY's rows at S <= 5: dim_s up to 4, T = 8, odd c
SLICE_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from mat_mul_amd import FusedAlphaTensor, _lib
from net_family import FAMILY
from net_ref import dims, make_inputs, make_weights
assert _lib.AB_VARIANT and "libtensorgame_ab.so" in open("/proc/self/maps").read()
out = {}
for name in sys.argv[3].split(","):
    m = dims(FAMILY[name].cfg)
    net = FusedAlphaTensor.from_state_dict(make_weights(m, 7), FAMILY[name].k, device="cuda:0")
    xx, ss = make_inputs(m, 7, 77)
    out[name] = net.torso(torch.from_numpy(xx).cuda(), torch.from_numpy(ss).cuda()).cpu().numpy()
np.savez(sys.argv[2], **out)
print("TORSO_OK")
'''


def test_slice_kernel_equals_the_per_game_kernel_over_the_small_rows_bit_for_bit(tmp_path):
    """TG_NET_TORSO_SLICES (A/B library only) forces net_torso_slice_kernel where the product runs net_torso_kernel.
    Both are one body over nseq sequences, nseq = 1 or S, and apply the same operations to each row in the same order,
    so ee agrees bit for bit: here with dim_s up to 4 in torso_inputs at nseq = 1, T = 8, odd c and S from 1 to 5."""
    import net_family
    ms = [dims(net_family.FAMILY[r].cfg) for r in SMALL_ROWS]
    assert all(m["S"] <= 5 for m in ms) and {3, 4} <= {m["dim_s"] for m in ms} and any(m["T"] == 8 for m in ms)
    assert any(m["c"] % 2 for m in ms)
    script = tmp_path / "slice_case.py"
    script.write_text(SLICE_SCRIPT)
    got = {}
    for tag, extra in (("game", {}), ("slices", {"TG_NET_TORSO_SLICES": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "TG_NET_TORSO_SLICES"}
        env.update(TG_LIB_VARIANT="ab", **extra)
        res = subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_path / f"{tag}.npz"), ",".join(SMALL_ROWS)],
                             env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "TORSO_OK" in res.stdout, (res.stdout[-1000:], res.stderr[-3000:])
        got[tag] = np.load(tmp_path / f"{tag}.npz")
    assert sorted(got["game"].files) == sorted(SMALL_ROWS)
    for name, m in zip(SMALL_ROWS, ms):
        a, b = got["game"][name], got["slices"][name]
        assert a.shape == b.shape == (7, 3 * m["S"] ** 2, m["c"]) and np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, np.abs(a - b).max())
