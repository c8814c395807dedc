"""tg_demo_items / ops.demo_items / SyntheticDemos.items, __getitem__, batches on the MI355X: random-index items of a
demo set against the reference's recorded __getitem__, the oracle helper (demo_items_ref.py) and the grouped
batch(k) / step_many path."""
import numpy as np
import pytest
import torch

from demo_items_ref import ref_items
from guarded_buffers import CANARY, GUARD, check_flat, check_states, guarded, guarded_states
from mat_mul_amd import SyntheticDemos, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.int8, torch.float32, torch.float16, torch.bfloat16]


def i8(frames):
    """frames of any output dtype -> their int8 values (the float forms carry an int8 exactly)"""
    f = frames.detach()
    return (f if f.dtype == torch.int8 else f.float()).cpu().numpy().astype(np.int8)


def to_dev(tokens, targets, pad_to=16):
    tok = torch.from_numpy(np.ascontiguousarray(tokens)).to(DEV)
    tgt = ops.alloc_states(targets.shape[0], targets.shape[1], DEV, pad_to=pad_to)
    tgt.copy_(torch.from_numpy(np.ascontiguousarray(targets)))
    return tok, tgt


def check_against_ref(got, want, what):
    frames, sc, ac, rw = got
    assert np.array_equal(i8(frames), want[0]), what
    assert np.array_equal(sc.cpu().numpy(), want[1]), what
    assert np.array_equal(ac.cpu().numpy(), want[2]), what
    assert np.array_equal(rw.cpu().numpy(), want[3]), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_reference_items_in_one_call(golden, dtype):
    g = golden("reference_dataset_getitem")
    tok, tgt = to_dev(g["tokens"], g["target"])
    frames, sc, ac, rw = ops.demo_items(tok, tgt, torch.arange(21, device=DEV), 2, dtype=dtype)
    assert frames.dtype == dtype and frames.shape == (21, 2, 4, 4, 4)
    assert np.array_equal(i8(frames), g["frames"]) and np.array_equal(ac.cpu().numpy(), g["action"])
    assert np.array_equal(torch.cat([sc, rw], 1).cpu().numpy(), g["meta"].astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_dataset_items_in_one_call_per_shape(golden, dtype):
    g = golden("synthetic_demos")
    shapes = sorted({k.rsplit("_", 2)[0] for k in g.files if k.startswith("ds_") and k.endswith("_tokens")})
    for shape in shapes:  # ds_S{S}_R{R}_T{T}: the demos of one shape, every item of every demo in one call
        S, R, T = (int(p[1:]) for p in shape.split("_")[1:4])
        demos = sorted({int(k.split("_")[4]) for k in g.files if k.startswith(shape + "_") and k.endswith("_tokens")})
        tok, tgt = to_dev(np.stack([g[f"{shape}_{d}_tokens"] for d in demos]),
                          np.stack([g[f"{shape}_{d}_target"] for d in demos]))
        n = len(demos) * R
        frames, sc, ac, rw = ops.demo_items(tok, tgt, torch.arange(n, device=DEV), T, dtype=dtype)
        got = i8(frames)
        for x in range(n):
            d, k = divmod(x, R)
            pre = f"{shape}_{demos[d]}_item{k}"
            assert np.array_equal(got[x], g[pre + "_frames"]), pre
            assert [float(sc[x, 0]), float(rw[x, 0])] == g[pre + "_meta"].tolist(), pre
            assert np.array_equal(ac[x].cpu().numpy(), g[pre + "_action"]), pre


def grouped_items(demos, idx, T):
    """What a caller has without demo_items: group the batch by action index, batch(k) per group, pick the demos."""
    R = demos.max_actions
    S = demos.dim_3d
    N = idx.shape[0]
    frames = torch.zeros((N, T, S, S, S), dtype=torch.int8, device=DEV)
    sc = torch.zeros((N, 1), device=DEV)
    ac = torch.zeros((N, 3 * S), dtype=torch.int8, device=DEV)
    rw = torch.zeros((N, 1), device=DEV)
    d_all, k_all = idx // R, idx % R
    for k in torch.unique(k_all).tolist():
        sel = (k_all == k).nonzero().flatten()
        st, s, a, r = demos.batch(k)
        d = d_all[sel]
        frames[sel], sc[sel], ac[sel], rw[sel] = st[d], s[d], a[d], r[d]
    return frames, sc, ac, rw


def cfg5_indices(n_demos, R, N, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_demos * R, size=N)
    idx[: N // 8] = idx[N // 8: N // 4]  # repeats
    idx[-4:] = [0, R - 1, (n_demos - 1) * R, n_demos * R - 1]  # k = 0 and k = R - 1, first and last demo
    return torch.from_numpy(idx).to(DEV)


@pytest.mark.parametrize("random_basis", [False, True])
def test_cfg5_random_indices_against_grouped_path_and_oracle(random_basis):
    R, S, T, n_demos = 64, 25, 2, 4096
    demos = SyntheticDemos.generate(n_demos, S, R, DEV, dim_t=T, seed=17, random_basis=random_basis)
    if random_basis:  # the basis widens the factors past {-1, 0, 1} (items with |u| or |v| > 11 would take the exact
        # path; at this seed they stay within 7 -- test_overflow_flag_equals_oracle_and_is_sticky covers that path)
        fac = demos.action_seq[..., : 2 * S].to(torch.int32) - demos.shift
        assert int(fac.abs().amax()) > 1
    idx = cfg5_indices(n_demos, R, 4096, seed=5)
    for dtype in (torch.int8, torch.float32):
        got = demos.items(idx, dtype=dtype)
        want = grouped_items(demos, idx, T)
        assert torch.equal(torch.from_numpy(i8(got[0])), want[0].cpu())
        for a, b in zip(got[1:], want[1:]):
            assert torch.equal(a, b)
    sub = torch.cat([idx[-4:], idx[:252]])
    d = torch.unique(sub // R)
    remap = torch.zeros(n_demos, dtype=torch.int64, device=DEV)
    remap[d] = torch.arange(d.numel(), device=DEV)
    loc = remap[sub // R] * R + sub % R
    want = ref_items(demos.action_seq[d].cpu().numpy(), demos.target_tensor[d].cpu().numpy(), loc.cpu().numpy(), T)
    ovf = torch.zeros((256,), dtype=torch.uint8, device=DEV)
    got = ops.demo_items(demos.action_seq, demos.target_tensor, sub, T, dtype=torch.int8, overflow=ovf)
    check_against_ref(got, want, "cfg5")
    assert np.array_equal(ovf.cpu().numpy(), want[4])


def random_demos(n, R, S, rng, stride_pad):
    tok = rng.choice(np.array([0, 1, 2], np.int8), size=(n, R, 3 * S), p=[0.15, 0.7, 0.15])
    tgt = rng.integers(-128, 128, size=(n, S, S, S)).astype(np.int8)
    t = torch.from_numpy(tok).to(DEV)
    stride = S ** 3 + stride_pad
    buf = torch.zeros((n, stride), dtype=torch.int8, device=DEV)
    g = buf[:, : S ** 3].unflatten(1, (S, S, S))
    g.copy_(torch.from_numpy(tgt))
    return tok, tgt, t, g


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 8, 9, 16, 17, 25, 32])
def test_shape_sweep_against_oracle(S):
    rng = np.random.default_rng(S)
    for ci, R in enumerate([1, 7, 33, 64, 100]):
        n = 3
        pad = [0, 16 - (S ** 3) % 16 if S ** 3 % 16 else 0, 5][(ci + S) % 3]  # unpadded, 16-aligned, odd stride
        tok, tgt, t, g = random_demos(n, R, S, rng, pad)
        idx = np.array([0, R - 1, n * R - 1, int(rng.integers(0, n * R)), R * 1 + R // 2])
        for ti, T in enumerate([1, 2, 4, R + 2]):
            dtype = DTYPES[(ci + ti + S) % 4]
            ovf = torch.zeros((idx.size,), dtype=torch.uint8, device=DEV)
            got = ops.demo_items(t, g, torch.from_numpy(idx).to(DEV), T, dtype=dtype, overflow=ovf)
            want = ref_items(tok, tgt, idx, T)
            check_against_ref(got, want, (S, R, T, dtype))
            assert np.array_equal(ovf.cpu().numpy(), want[4]), (S, R, T)


@pytest.mark.parametrize("S, R", [(4, 7), (16, 20), (25, 40)])
def test_items_at_one_action_index_equal_batch(S, R):
    demos = SyntheticDemos(R, 48, 3, S, DEV, seed=9)
    for k in range(R):
        idx = torch.arange(48, device=DEV) * R + k
        st, sc, ac, rw = demos.items(idx)
        bst, bsc, bac, brw = demos.batch(k)
        assert torch.equal(st.to(torch.int8), bst) and torch.equal(sc, bsc) and torch.equal(ac, bac)
        assert torch.equal(rw, brw)
    f, s, a, r = demos[5 * R + 2]
    assert f.shape == (3, S, S, S) and s.shape == (1,) and a.shape == (3 * S,) and r.shape == (1,)
    assert float(s) == R - 2 and float(r) == -3


@pytest.mark.parametrize("S", [4, 9, 16, 25])
def test_overflow_flag_equals_oracle_and_is_sticky(S):
    rng = np.random.default_rng(100 + S)
    R, T, n = 9, 3, 4
    tok = rng.integers(-3, 6, size=(n, R, 3 * S)).astype(np.int8)  # |u|,|v| <= 4: the matrix-core path at 16 / 25
    tok[0, :, 2 * S:] = rng.integers(60, 120, size=(R, S))           # w wide: frame 0 leaves int8
    tok[1] = rng.integers(-128, 128, size=(R, 3 * S))                 # everything wide (the exact path)
    tgt = rng.integers(-128, 128, size=(n, S, S, S)).astype(np.int8)
    t, g = to_dev(tok, tgt)
    idx = np.array([0, 3, R - 1, R + 1, R + 4, 2 * R, 3 * R + 2, 3 * R + R - 1])
    want = ref_items(tok, tgt, idx, T)
    assert want[4].any() and not want[4].all()
    ovf = torch.zeros((idx.size,), dtype=torch.uint8, device=DEV)
    got = ops.demo_items(t, g, torch.from_numpy(idx).to(DEV), T, dtype=torch.float32, overflow=ovf)
    check_against_ref(got, want, S)
    assert np.array_equal(ovf.cpu().numpy(), want[4])
    pre = torch.ones_like(ovf)  # sticky: a set flag stays set
    ops.demo_items(t, g, torch.from_numpy(idx).to(DEV), T, overflow=pre)
    assert bool((pre == 1).all())


@pytest.mark.parametrize("S, R", [(4, 7), (9, 10), (16, 49), (25, 64)])
def test_bad_indices_are_zero_and_flagged_guards_intact(S, R):
    rng = np.random.default_rng(7 * S)
    n, T = 5, 2
    tok = rng.choice(np.array([0, 1, 2], np.int8), size=(n, R, 3 * S))
    tgt = rng.integers(-128, 128, size=(n, S, S, S)).astype(np.int8)
    idx = np.array([-1, 0, n * R, R - 1, 3 * R + 1, n * R - 1, -(2 ** 40)])
    N = idx.size
    tbuf, t = guarded((n, R, 3 * S), torch.int8)
    t.copy_(torch.from_numpy(tok))
    stride = S ** 3 + 16
    gbuf, g = guarded_states(n, S, stride)
    g.copy_(torch.from_numpy(tgt))
    ibuf, it = guarded((N,), torch.int64)
    it.copy_(torch.from_numpy(idx))
    fbuf, frames = guarded((N, T, S, S, S), torch.float32)
    sbuf, sc = guarded((N, 1), torch.float32)
    abuf, ac = guarded((N, 3 * S), torch.int8)
    rbuf, rw = guarded((N, 1), torch.float32)
    obuf, ovf = guarded((N,), torch.uint8)
    ovf.zero_()
    stbuf, status = guarded((1,), torch.uint32)
    status.zero_()
    ops.demo_items(t, g, it, T, out=frames, scalars=sc, actions=ac, rewards=rw, overflow=ovf, status=status)
    torch.cuda.synchronize()
    want = ref_items(tok, tgt, idx, T)
    check_against_ref((frames, sc, ac, rw), want, (S, R))
    assert int(status[0]) == 1 and want[5][0] == 1
    bad = [0, 2, 6]
    assert not frames[bad].any() and not sc[bad].any() and not ac[bad].any() and not rw[bad].any()
    for buf, what in [(tbuf, "tokens"), (ibuf, "idx"), (fbuf, "frames"), (sbuf, "scalars"), (abuf, "actions"),
                      (rbuf, "rewards"), (obuf, "overflow"), (stbuf, "status")]:
        check_flat(buf, what)
    check_states(gbuf, n, S, stride, "targets")
    # a call with good indices only leaves status alone
    status.zero_()
    ops.demo_items(t, g, it[1:2], T, status=status)
    assert int(status[0]) == 0


def test_graph_capture_replays_with_refilled_indices():
    demos = SyntheticDemos(20, 64, 2, 16, DEV, seed=4)
    N = 256
    rng = np.random.default_rng(1)
    static_idx = torch.from_numpy(rng.integers(0, len(demos), size=N)).to(DEV)
    frames = torch.empty((N, 2, 16, 16, 16), dtype=torch.bfloat16, device=DEV)
    sc = torch.empty((N, 1), device=DEV)
    ac = torch.empty((N, 48), dtype=torch.int8, device=DEV)
    rw = torch.empty((N, 1), device=DEV)

    def run():
        ops.demo_items(demos.action_seq, demos.target_tensor, static_idx, 2, dtype=torch.bfloat16, out=frames,
                       scalars=sc, actions=ac, rewards=rw)

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        run()  # warm-up (host caches) outside the capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for seed in (2, 3):
        static_idx.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, len(demos), size=N)))
        g.replay()
        torch.cuda.synchronize()
        want = demos.items(static_idx.clone(), dtype=torch.bfloat16)
        assert torch.equal(frames, want[0]) and torch.equal(sc, want[1]) and torch.equal(ac, want[2])
        assert torch.equal(rw, want[3])


def test_batches_cover_the_subset_once_in_a_seeded_order():
    demos = SyntheticDemos(7, 40, 2, 4, DEV, seed=12)
    indices = torch.from_numpy(np.random.default_rng(0).permutation(len(demos))[:150]).to(DEV)

    def epoch(seed, **kw):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        return list(demos.batches(32, generator=gen, indices=indices, **kw))

    b1 = epoch(5)
    assert [b[0].shape[0] for b in b1] == [32, 32, 32, 32, 22]
    order = indices[torch.randperm(150, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)]
    assert sorted(order.tolist()) == sorted(indices.tolist())
    for i, b in enumerate(b1):
        want = demos.items(order[32 * i: 32 * (i + 1)])
        for x, y in zip(b, want):
            assert torch.equal(x, y)
    # every item of the subset exactly once: (scalar, action, frames) of the epoch match those of the subset
    got = torch.cat([b[0] for b in b1]).flatten(1)
    ref = demos.items(indices)[0].flatten(1)
    key = lambda t: sorted(map(tuple, t.to(torch.int8).cpu().numpy().tolist()))
    assert key(got) == key(ref)
    b2 = epoch(5)
    assert all(torch.equal(x, y) for p, q in zip(b1, b2) for x, y in zip(p, q))
    assert [b[0].shape[0] for b in epoch(5, drop_last=True)] == [32] * 4
    unshuffled = list(demos.batches(64, shuffle=False, indices=indices))
    assert torch.equal(torch.cat([b[0] for b in unshuffled]), demos.items(indices)[0])
