"""The fused network at the 4x4 matmul tensor (S = TG_NET_WIDE2_S = 16) on the MI355X, for the two S = 16 configurations
of net_s16_ref: the precision bound against the reference's float64 outputs and the float64 restatement at the fixture's
batch and at B = 1, 37 and 256, the sampling rule with given uniforms and with the internal stream, input dtypes and row
subsets, the independence of games and slices on the device (the torso runs one workgroup per (game, slice) here),
guarded outputs, graph capture, self-play through search.actor_prediction, and the slice kernel against the per-game
kernel at S = 9 in the A/B library."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedTrainer, SyntheticDemos, ops, search
from mat_mul_amd._lib import TensorGameError

from guarded_buffers import check_flat, guarded
from net_ref import Ref, make_inputs, make_weights, philox_uniforms, pick
from net_s16_ref import CONFIGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
CASES = sorted(CONFIGS)
GOLDEN = Path(__file__).resolve().parent / "golden" / "net_s16_cases.npz"
N = 6  # the fixture's input states (make_golden_net_s16.N: 16 would take the archive past the size of the others)


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(GOLDEN)
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def states(name, B):
    """B = N: the fixture's states; otherwise make_inputs'; with their g_action."""
    cfg = CONFIGS[name]
    f = fixture(name)
    if B == N:
        return f["xx"], f["ss"], f["g_action"]
    xx, ss = make_inputs(cfg, B, 500 + B)
    ga = np.random.default_rng(600 + B).integers(0, cfg["n_logits"], size=(B, cfg["n_steps"])).astype(np.int8)
    return xx, ss, ga


@functools.lru_cache(maxsize=None)
def host(name, B):
    """The float64 restatement's outputs (ee, oo, zz0, q, qq) for states(name, B)."""
    cfg = CONFIGS[name]
    ref = Ref(make_weights(cfg, int(fixture(name)["seed"].item())), cfg, device=DEV)
    xx, ss, ga = states(name, B)
    ee = ref.torso(xx, ss)
    oo, zz0, q = ref.teacher(ee, ga)
    return {k: v.cpu() for k, v in (("ee", ee), ("oo", oo), ("zz0", zz0), ("q", q), ("qq", Ref.risk(q)))}


def setup(name):
    cfg = CONFIGS[name]
    sd = make_weights(cfg, int(fixture(name)["seed"].item()))
    return cfg, sd, FusedAlphaTensor.from_state_dict(sd, cfg["n_samples"], device=DEV)


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max()
    print(f"{what}: err {err:.3e}, bound {1e-5 * max(1.0, np.abs(ref).max()):.3e}")
    assert err <= 1e-5 * max(1.0, np.abs(ref).max()), (what, err)


@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_the_float64_reference(name):
    cfg, sd, net = setup(name)
    f = fixture(name)
    assert f["xx"].shape[0] == N
    xx, ss, ga = (torch.from_numpy(a).to(DEV) for a in states(name, N))
    ee = net.torso(xx.float(), ss)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = net.fwd_infer(xx.float(), ss, seed=1)
    assert tuple(aa.shape) == (N, cfg["n_samples"], 48) and tuple(pp.shape) == (N, cfg["n_samples"])
    assert tuple(ee.shape) == (N, 768, cfg["dim_c"])
    for got, key in ((ee, "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        rec = f[f"{key}64"]
        close(got[:rec.shape[0]], rec, f"{name} {key} (recorded)")
        close(got, host(name, N)[key].numpy(), f"{name} {key} (restatement)")


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("name", CASES)
def test_precision_bound_against_the_restatement_by_batch(name, B):
    cfg, sd, net = setup(name)
    xx, ss, ga = (torch.from_numpy(a).to(DEV) for a in states(name, B))
    h = host(name, B)
    oo, zz0, q = net.logits(xx, ss, ga, with_q=True)
    aa, pp, qq = net.fwd_infer(xx, ss, seed=2)
    assert tuple(aa.shape) == (B, cfg["n_samples"], 48)
    for got, key in ((net.torso(xx, ss), "ee"), (oo, "oo"), (zz0, "zz0"), (q, "q"), (qq, "qq")):
        close(got, h[key].numpy(), f"{name} B={B} {key}")


def host_check(name, sd, tokens, pp, u):
    """tokens / pp of the device against the rule applied to the float64 restatement's probabilities."""
    cfg = CONFIGS[name]
    ref = Ref(sd, cfg, device=DEV)
    B, k, n = tokens.shape
    ee = host(name, N)["ee"].to(DEV).repeat_interleave(k, 0)
    tok = tokens.to(torch.int64).reshape(B * k, n)
    start = torch.full((B * k, 1), cfg["n_logits"], dtype=torch.long, device=DEV)
    oo, _ = ref.decode(ee, torch.cat([start, tok[:, :-1]], 1))
    p = torch.softmax(oo, -1).cpu().numpy().reshape(B, k, n, -1)
    want, dist = pick(u, p)
    keep = dist >= 1e-5
    got = tokens.cpu().numpy()
    print(f"{name}: {(~keep).sum()} of {keep.size} draws within 1e-5 of a boundary")
    assert np.array_equal(got[keep], want[keep])
    p_chosen = np.take_along_axis(p, got[..., None].astype(np.int64), -1)[..., 0]
    np.testing.assert_allclose(pp.cpu().numpy(), p_chosen.prod(-1), rtol=1e-5, atol=0)
    assert (~keep).sum() < 0.01 * keep.size


@pytest.mark.parametrize("name", CASES)
def test_sampling_follows_the_host_rule(name):
    cfg, sd, net = setup(name)
    k, n = cfg["n_samples"], cfg["n_steps"]
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, N))
    ee = net.torso(xx, ss)
    u = np.random.default_rng(5).random((N, k, n)).astype(np.float32)
    tbuf, tok = guarded((N, k, n), torch.int8)
    tokens, pp, _ = ops.net_sample(net.c, net.w, ee, torch.arange(N, device=DEV), k, 0, 0,
                                   uniforms=torch.from_numpy(u).to(DEV), tokens=tok)
    check_flat(tbuf, "tokens")
    host_check(name, sd, tokens, pp, u.astype(np.float64))
    rows = torch.arange(N, device=DEV, dtype=torch.int64) * 977 + 3
    t1, p1, q1 = net.sample(ee, rows=rows, seed=0x1234_5678_9ABC, call=41)  # steps 0 .. 47: Philox blocks 0 .. 11
    u = philox_uniforms(0x1234_5678_9ABC, rows.cpu().numpy(), 41, k, n)
    t2, p2, q2 = net.sample(ee, uniforms=torch.from_numpy(u.astype(np.float32)).to(DEV))
    assert torch.equal(t1, t2) and torch.equal(p1, p2) and torch.equal(q1, q2)
    host_check(name, sd, t1, p1, u)


@pytest.mark.parametrize("name", CASES)
def test_int8_frames_row_subsets_and_empty_batches(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, N))
    ee8, eef = net.torso(xx, ss), net.torso(xx.float(), ss)
    assert torch.equal(ee8, eef)
    rows = torch.arange(N, device=DEV, dtype=torch.int64) + 1000
    full = net.sample(ee8, rows=rows, seed=4, call=2)
    sel = torch.tensor([5, 2, 0, 4], device=DEV)
    part = net.sample(net.torso(xx[sel].float(), ss[sel]), rows=rows[sel], seed=4, call=2)
    for a, b in zip(full, part):
        assert torch.equal(a[sel], b)
    one = net.sample(net.torso(xx[3:4], ss[3:4]), rows=rows[3:4], seed=4, call=2)  # B = 1
    for a, b in zip(full, one):
        assert torch.equal(a[3:4], b)
    ee0 = net.torso(xx[:0], ss[:0])  # B = 0 is a no-op
    assert tuple(ee0.shape) == (0, 768, cfg["dim_c"])
    t0, p0, q0 = net.sample(ee0, rows=rows[:0])
    assert tuple(t0.shape) == (0, cfg["n_samples"], 48) and p0.numel() == 0 and q0.numel() == 0


@pytest.mark.parametrize("name", CASES)
def test_games_and_slices_are_independent_on_the_device(name):
    """One workgroup per (game, slice i) writes rows i*3S .. i*3S + 3S - 1 of its game: a batch equals its games run one
    by one, nothing is written outside ee, and another game's input changes no row of this one."""
    cfg, sd, net = setup(name)
    B = 5
    xx, ss, _ = (torch.from_numpy(a).to(DEV) for a in states(name, 37))
    xx, ss = xx[:B].contiguous(), ss[:B].contiguous()
    buf, out = guarded((B, 768, cfg["dim_c"]), torch.float32)
    ee = ops.net_torso(net.c, net.w, xx, ss, out=out)
    check_flat(buf, "ee")
    assert ee.data_ptr() == out.data_ptr() and bool(torch.isfinite(ee).all())
    for g in range(B):
        assert torch.equal(net.torso(xx[g:g + 1], ss[g:g + 1])[0], ee[g]), g
    x2, s2 = xx.clone(), ss.clone()
    x2[2] = torch.roll(x2[2], 1, dims=-1) + 1
    s2[2] += 1.0
    ee2 = net.torso(x2, s2)
    keep = [0, 1, 3, 4]
    assert torch.equal(ee2[keep], ee[keep])
    # every slice of the changed game moves (the scalar reaches every position)
    moved = (ee2[2] != ee[2]).reshape(16, 48 * cfg["dim_c"]).any(1)
    assert bool(moved.all())
    # one slice of one grid of the input: frames[t, i] reaches grid 0 slice i, and every slice of grids 1 and 2
    x3 = xx.clone()
    x3[1, :, 7] += 1
    d = (net.torso(x3, ss)[1] != ee[1]).reshape(16, 3, 16 * cfg["dim_c"]).any(2)
    assert bool(d[7].all()) and bool(d.any(1).all())


@pytest.mark.parametrize("name", CASES)
def test_graph_capture_equals_eager(name):
    cfg, sd, net = setup(name)
    xx, ss, _ = states(name, N)
    x, s = torch.from_numpy(xx).to(DEV).float(), torch.from_numpy(ss).to(DEV)
    rows = torch.arange(N, device=DEV, dtype=torch.int64)
    want = net.fwd_infer(x, s, seed=2, call=5, rows=rows)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        net.fwd_infer(x, s, seed=2, call=5, rows=rows)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = net.fwd_infer(x, s, seed=2, call=5, rows=rows)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def test_the_trainer_refuses_s16():
    cfg = CONFIGS["a16"]
    with pytest.raises(TensorGameError, match="training at dim_3d=16 .* is not built"):
        FusedTrainer.from_state_dict(make_weights(cfg, 1), n_samples=cfg["n_samples"], device=DEV)


def _rank_one_signed(d):
    """d (S,S,S) integer: a rank-1 tensor u x v x w with u, v, w in {-1, 0, 1} (zero included)."""
    d = d.astype(np.int64)
    if not d.any():
        return True
    if np.abs(d).max() > 1:
        return False
    i, j, k = np.argwhere(d)[0]
    return np.array_equal(d, np.einsum("i,j,k->ijk", d[:, j, k], d[i, :, k], d[i, j, :]))


def test_self_play_search_with_the_fused_network_at_s16():
    cfg, sd, net = setup("a16")
    B, S, T, k = 8, 16, cfg["dim_t"], cfg["n_samples"]
    assert T == 2
    demos = SyntheticDemos(2, B, 1, S, device=DEV, seed=3)  # rank <= 2 targets
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.reshape(B, S, S, S)
    runs = []
    for _ in range(2):
        forest = search.SearchForest(B, S, T, k=k, max_actions=3, n_sim=2, device=DEV)
        out = search.actor_prediction(net.policy(seed=0), start, max_actions=3, n_sim=2, n_bar=100, n_logits=3, k=k,
                                      forest=forest)
        assert int(forest.status.abs().sum()) == 0
        runs.append([t.cpu() for t in out] + [forest.final_heads().cpu()])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    st, pol, rewards, lengths, final = runs[0]
    assert tuple(st.shape) == (B, 3, T, S, S, S) and tuple(pol.shape) == (B, 3, 3 * S, 3)
    assert tuple(rewards.shape) == (B, 3) and tuple(lengths.shape) == (B,)
    assert bool((lengths >= 1).all()) and bool((lengths <= 3).all())
    st, final = st.numpy(), final.numpy()
    for b in range(B):
        n = int(lengths[b])
        assert np.array_equal(st[b, 0], start[b].cpu().numpy())
        assert not st[b, n:].any()
        for l in range(n):  # the move played at step l: head(l) - head(l + 1) is one signed rank-1 term
            nxt = st[b, l + 1, 0] if l + 1 < n else final[b]
            assert _rank_one_signed(st[b, l, 0].astype(np.int64) - nxt), (b, l)
        assert n == 3 or not final[b].any()  # a game shorter than max_actions ended at the zero tensor


# ---- the slice kernel against the per-game kernel at a size both run (the A/B library's switch) ------------------------
SLICE_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from mat_mul_amd import FusedAlphaTensor, _lib
from net_ref import make_inputs, make_weights
from net_s9_ref import CONFIGS
assert _lib.AB_VARIANT and "libtensorgame_ab.so" in open("/proc/self/maps").read()
out = {}
for name in sorted(CONFIGS):
    cfg = CONFIGS[name]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 7), cfg["n_samples"], device="cuda:0")
    xx, ss = make_inputs(cfg, 19, 77)
    out[name] = net.torso(torch.from_numpy(xx).cuda(), torch.from_numpy(ss).cuda()).cpu().numpy()
np.savez(sys.argv[2], **out)
print("TORSO_OK")
'''


def test_slice_kernel_equals_the_per_game_kernel_at_s9_bit_for_bit(tmp_path):
    """TG_NET_TORSO_SLICES (A/B library only) forces net_torso_slice_kernel where the product runs net_torso_kernel.
    Both apply the same operations to each row in the same order, so ee agrees bit for bit."""
    script = tmp_path / "slice_case.py"
    script.write_text(SLICE_SCRIPT)
    got = {}
    for tag, extra in (("game", {}), ("slices", {"TG_NET_TORSO_SLICES": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "TG_NET_TORSO_SLICES"}
        env.update(TG_LIB_VARIANT="ab", **extra)
        res = subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_path / f"{tag}.npz")], env=env,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "TORSO_OK" in res.stdout, (res.stdout[-1000:], res.stderr[-3000:])
        got[tag] = np.load(tmp_path / f"{tag}.npz")
    for name in got["game"].files:
        a, b = got["game"][name], got["slices"][name]
        assert a.shape == b.shape and np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, np.abs(a - b).max())
