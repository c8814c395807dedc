"""tg_symmetry_apply / tg_symmetry_sample, ops.symmetry_apply / symmetry_sample and Augment on the MI355X: the apply
kernel is bit-exact against the host restatement (tests/symmetry_ref.py) at every size class, dtype and alignment, each
part of the group alone, identity and inverse, the env step and the Strassen replay commute with the group, overflow and
bad rows follow the header, the sampler is the header's rule bit for bit, the ``augment=`` keyword of the datasets is
gather + apply, and sample + apply can be captured."""
import functools

import numpy as np
import pytest
import torch

import symmetry_ref as SR
from mat_mul_amd import Augment, FusedTrainer, SyntheticDemos, TensorGameData, TensorGameEnv, ops
from net_ref import CONFIGS, make_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.int8]
SIZES = [1, 2, 4, 5, 9, 16, 25, 32]


def i8(t):
    t = t.detach()
    return (t if t.dtype == torch.int8 else t.float()).cpu().numpy().astype(np.int8)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def n_items(S):
    return 37 if S <= 5 else 5  # 37: not a multiple of the sixteen items of a workgroup


@functools.lru_cache(maxsize=None)
def case(S, T, shift, flags=7):
    """Random items, their rows and what the restatement makes of them (computed once, never written)."""
    N = n_items(S)
    rng = np.random.default_rng(1000 * S + 10 * T + shift)
    frames = rng.integers(-127, 128, size=(N, T, S, S, S)).astype(np.int8)
    tokens = rng.integers(0, 2 * shift + 1, size=(N, 3 * S)).astype(np.int8)
    sym = SR.sample(N, S, seed=77 + S, item_offset=T, flags=flags)
    want_f, want_t, ov, st = SR.apply(frames, tokens, sym, shift)
    assert st == 0 and not ov.any()
    return frames, tokens, sym, want_f, want_t


# ---- 1. bit-exact apply ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("S", SIZES)
def test_apply_is_bit_exact(S, T, dtype, shift):
    frames, tokens, sym, want_f, want_t = case(S, T, shift)
    N = frames.shape[0]
    ov = torch.zeros((N,), dtype=torch.uint8, device=DEV)
    st = torch.zeros((1,), dtype=torch.uint32, device=DEV)
    out, act = ops.symmetry_apply(dev(frames), dev(tokens), dev(sym), dtype=dtype, shift=shift, overflow=ov, status=st)
    assert out.dtype == dtype and out.shape == frames.shape and act.dtype == torch.int8
    assert np.array_equal(i8(out), want_f)
    assert np.array_equal(act.cpu().numpy(), want_t)
    assert not ov.any() and int(st[0]) == 0
    only, none = ops.symmetry_apply(dev(frames), None, dev(sym), dtype=dtype, shift=shift)  # frames without actions
    assert none is None and torch.equal(only, out)


@pytest.mark.parametrize("S", SIZES)
def test_apply_at_odd_addresses(S):
    """frames_in one byte and frames_out one element behind an aligned allocation: the head / tail paths of both the
    16-byte loads and the 16-byte stores (a frame of 729 or 15 625 bytes starts anywhere besides)."""
    frames, tokens, sym, want_f, want_t = case(S, 3, 1)
    n = frames.size
    src = torch.zeros((n + 64,), dtype=torch.int8, device=DEV)
    x = src[1:1 + n].view(frames.shape)
    x.copy_(dev(frames))
    assert x.data_ptr() % 16 == 1
    for dtype in DTYPES:
        dst = torch.full((n + 64,), 99, dtype=dtype, device=DEV)
        out = dst[1:1 + n].view(frames.shape)
        assert out.data_ptr() % 16 == dst.element_size()
        got, act = ops.symmetry_apply(x, dev(tokens), dev(sym), dtype=dtype, out=out)
        assert got is out and np.array_equal(i8(out), want_f), dtype
        assert np.array_equal(act.cpu().numpy(), want_t)
        assert bool((dst[:1] == 99).all()) and bool((dst[1 + n:] == 99).all()), dtype  # nothing outside the view


# ---- 2. each part alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [SR.MODES, SR.PERMS, SR.SIGNS], ids=["modes", "perms", "signs"])
@pytest.mark.parametrize("S", [5, 16])
def test_each_part_alone(S, flags):
    frames, tokens, sym, want_f, want_t = case(S, 3, 2, flags)
    assert not np.array_equal(want_f, frames)
    out, act = ops.symmetry_apply(dev(frames), dev(tokens), dev(sym), dtype=torch.float32, shift=2)
    assert np.array_equal(i8(out), want_f) and np.array_equal(act.cpu().numpy(), want_t)


# ---- 3. identity and inverse -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 9, 25])
def test_identity_and_inverse(S):
    frames, tokens, sym, _, _ = case(S, 3, 2)
    N = frames.shape[0]
    x, a = dev(frames), dev(tokens)
    for dtype in DTYPES:
        out, act = ops.symmetry_apply(x, a, dev(SR.identity(N, S)), dtype=dtype, shift=2)
        assert np.array_equal(i8(out), frames) and torch.equal(act, a), dtype
    gx, ga = ops.symmetry_apply(x, a, dev(sym), dtype=torch.int8, shift=2)
    assert not torch.equal(gx, x)
    back, aback = ops.symmetry_apply(gx, ga, dev(SR.inverse(sym, S)), dtype=torch.int8, shift=2)
    assert torch.equal(back, x) and torch.equal(aback, a)


# ---- 4. the game commutes with the group ----------------------------------------------------------------------------
@pytest.mark.parametrize("S, B", [(4, 64), (9, 8), (16, 8), (25, 4)])
def test_the_step_commutes_with_the_group(S, B):
    rng = np.random.default_rng(S)
    x = rng.integers(-2, 3, size=(B, S, S, S)).astype(np.int8)
    a = rng.integers(0, 3, size=(B, 3 * S)).astype(np.int8)
    f = a.astype(np.int64) - 1
    last = f[:, :S, None, None] * f[:, None, S:2 * S, None] * f[:, None, None, 2 * S:]
    x[::2] = last[::2]  # every other game ends with this action
    x, a = dev(x), dev(a)
    sym = ops.symmetry_sample(B, S, DEV, seed=3)
    gx, ga = ops.symmetry_apply(x.unsqueeze(1), a, sym, dtype=torch.int8)
    left, done_left = ops.step(gx[:, 0], ga)
    stepped, done = ops.step(x, a)
    right, _ = ops.symmetry_apply(stepped.unsqueeze(1), None, sym, dtype=torch.int8)
    assert torch.equal(left, right[:, 0])
    assert torch.equal(done_left, done) and done.cpu().tolist() == [1, 0] * (B // 2)
    assert torch.equal(ops.done(gx[:, 0]), ops.done(x)) and torch.equal(ops.done(left), done)


# ---- 5. Strassen -----------------------------------------------------------------------------------------------------
def test_strassen_solves_every_symmetric_copy(golden):
    g = golden("strassen")
    tokens, shift, N = g["tokens"], 1, 16
    assert np.array_equal(tokens[:, :4] - shift, g["uu"])  # the fixture's tokens are factor + 1
    sym = ops.symmetry_sample(N, 4, DEV, seed=2)
    assert len({bytes(r) for r in sym.cpu().numpy()}) == N
    target = dev(np.broadcast_to(g["tensor"], (N, 1, 4, 4, 4)))
    start, _ = ops.symmetry_apply(target, None, sym, dtype=torch.int8, shift=shift)
    env = TensorGameEnv(N, 4, DEV, shift=shift)
    env.reset(start[:, 0])
    for k in range(7):
        _, act = ops.symmetry_apply(target, dev(np.broadcast_to(tokens[k], (N, 12))), sym, dtype=torch.int8, shift=shift)
        _, done = env.step(act)
        assert done.cpu().tolist() == [int(k == 6)] * N, k
    assert not bool(env.state.any())


# ---- 6. overflow and bad rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 9])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int8], ids=["float32", "int8"])
def test_overflow_and_bad_rows(S, dtype):
    N, T = 7, 2
    rng = np.random.default_rng(S)
    frames = rng.integers(-127, 128, size=(N, T, S, S, S)).astype(np.int8)
    tokens = rng.integers(0, 3, size=(N, 3 * S)).astype(np.int8)
    sym = SR.sample(N, S, seed=4)
    neg = lambda n, m, a: bool(sym[n, 1 + m * S + a] & 0x80)
    rho, pi, _ = SR.decode(sym[1], S)
    b = [0, 0, 0]
    for m in range(3):
        b[rho[m]] = int(pi[m][0])
    if not neg(1, 0, 0) ^ neg(1, 1, 0) ^ neg(1, 2, 0):
        sym[1, 1] ^= 0x80
    frames[1, 1, b[0], b[1], b[2]] = -128  # item 1: the entry that lands at (0,0,0), under an odd sign product
    sym[2, 1] |= 0x80                      # item 2: the token that lands at position 0 of block 0 is negated
    rho2, pi2, _ = SR.decode(sym[2], S)
    tokens[2, rho2[0] * S + pi2[0][0]] = -128
    frames[3, 0, 0, 0, 0] = -128           # item 3: -128 under an even sign product stays
    for m in range(3):
        sym[3, 1 + m * S:1 + (m + 1) * S] &= 0x7F
    sym[4, 1 + S + 1] = (sym[4, 1 + S + 1] & 0x80) | S  # item 4: an index S
    sym[5, 0] = 6                                        # item 5: a mode code 6
    want_f, want_t, want_ov, want_st = SR.apply(frames, tokens, sym)
    assert want_ov.tolist() == [0, 1, 1, 0, 0, 0, 0] and want_st == 1
    assert want_f[1, 1, 0, 0, 0] == -128 and want_t[2, 0] == -126 and (want_f[3] == -128).sum() == 1
    assert not want_f[4].any() and not want_t[5].any() and want_f[6].any()
    ov = torch.zeros((N,), dtype=torch.uint8, device=DEV)
    ov[6] = 1  # sticky: a call never clears it
    st = torch.zeros((1,), dtype=torch.uint32, device=DEV)
    out, act = ops.symmetry_apply(dev(frames), dev(tokens), dev(sym), dtype=dtype, overflow=ov, status=st)
    assert np.array_equal(i8(out), want_f) and np.array_equal(act.cpu().numpy(), want_t)
    assert ov.cpu().tolist() == [0, 1, 1, 0, 0, 0, 1] and int(st[0]) == 1


# ---- 7. the sampler --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_offset", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("seed", [7, 2 ** 40 + 3])
@pytest.mark.parametrize("S", [1, 4, 9, 25, 32])
def test_sampler_is_the_rule_bit_for_bit(S, seed, item_offset):
    N = 1000
    want = SR.sample(N, S, seed, item_offset)
    got = ops.symmetry_sample(N, S, DEV, seed=seed, item_offset=item_offset)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    halves = torch.cat([ops.symmetry_sample(400, S, DEV, seed=seed, item_offset=item_offset),
                        ops.symmetry_sample(600, S, DEV, seed=seed, item_offset=item_offset + 400)])
    assert torch.equal(halves, got)
    for modes, perms, signs in [(True, False, False), (False, True, False), (False, False, True), (False, False, False),
                                (True, False, True)]:
        part = ops.symmetry_sample(N, S, DEV, seed=seed, item_offset=item_offset, modes=modes, perms=perms, signs=signs)
        flags = (SR.MODES if modes else 0) | (SR.PERMS if perms else 0) | (SR.SIGNS if signs else 0)
        assert np.array_equal(part.cpu().numpy(), SR.sample(N, S, seed, item_offset, flags)), flags


# ---- 8. integration --------------------------------------------------------------------------------------------------
def mixed_data():
    """Synthetic, played and best rows in one epoch table (S = 4, T = 2)."""
    L = 6
    demos = SyntheticDemos(L, 32, 2, 4, DEV, seed=9)
    data = TensorGameData.from_demos(demos, 60, 0.5, seed=1, played_capacity=16, best_capacity=4)
    rng = np.random.default_rng(5)
    B = 6
    st = dev(rng.integers(-3, 4, size=(B, L, 2, 4, 4, 4)).astype(np.int8))
    po = dev(rng.random((B, L, 12, 3)).astype(np.float32))
    rw = dev(-rng.integers(1, 9, size=(B, L)).astype(np.float32))
    ln = dev(np.full(B, L, np.int64))
    data.played.add_games(st[:4], po[:4], rw[:4], ln[:4])
    data.best.add_games(st[4:], po[4:], rw[4:], ln[4:])
    data.set_fractions(0.5, 0.2)
    data.set_indexes(np.arange(60) < 30, np.arange(30) * 5, np.arange(20), np.arange(10))
    assert sorted(set(data.kind.cpu().tolist())) == [0, 1, 2]
    return demos, data


def check_augmented(items, N, S, dtype):
    """items(idx, augment=) == gather as int8, then the rows of a second augmenter in the same state."""
    aug, twin = Augment(5), Augment(5)
    for _ in range(2):  # the second batch continues the ids
        rows = twin.sym_for(N, S, DEV)
        assert twin.next_id == aug.next_id
        state, scalar, action, reward = items(dtype=dtype, augment=aug)
        p_state, p_scalar, p_action, p_reward = items(dtype=torch.int8)
        want_state, want_action = ops.symmetry_apply(p_state, p_action, rows, dtype=dtype)
        assert state.dtype == dtype and torch.equal(state, want_state) and torch.equal(action, want_action)
        assert torch.equal(scalar, p_scalar) and torch.equal(reward, p_reward)
        assert not torch.equal(i8_t(state), p_state)
        twin.next_id += N
        assert aug.next_id == twin.next_id
    resumed = Augment(0, signs=False)
    resumed.load_state_dict(aug.state_dict())
    a, b = items(dtype=dtype, augment=aug), items(dtype=dtype, augment=resumed)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and resumed.next_id == 3 * N


def i8_t(t):
    return t if t.dtype == torch.int8 else t.float().to(torch.int8)


def test_augmented_items_are_gather_then_apply():
    demos, data = mixed_data()
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, len(demos), size=50)).to(DEV)
    check_augmented(lambda **kw: demos.items(idx, **kw), 50, 4, torch.bfloat16)
    every = torch.arange(60, device=DEV)
    check_augmented(lambda **kw: data.items(every, **kw), 60, 4, torch.float32)
    moves = torch.arange(len(data.played), device=DEV)
    check_augmented(lambda **kw: data.played.items(moves, **kw), len(data.played), 4, torch.float16)
    assert int(data.status[0]) == 0 and int(data.played.status[0]) == 0


def test_batches_without_an_augmenter_are_unchanged_and_with_one_are_items():
    demos, data = mixed_data()
    for src in (demos, data):
        gen = lambda: torch.Generator(device=DEV).manual_seed(9)
        plain = list(src.batches(16, generator=gen()))
        same = list(src.batches(16, generator=gen(), augment=None))
        assert len(plain) == len(same) > 1
        assert all(torch.equal(x, y) for p, q in zip(plain, same) for x, y in zip(p, q))
        aug, twin = Augment(3), Augment(3)
        for got, p in zip(src.batches(16, generator=gen(), dtype=torch.int8, augment=aug), plain):
            N = p[0].shape[0]
            want_state, want_action = ops.symmetry_apply(i8_t(p[0]), p[2], twin.sym_for(N, 4, DEV), dtype=torch.int8)
            twin.next_id += N
            assert torch.equal(got[0], want_state) and torch.equal(got[2], want_action)
            assert torch.equal(got[1], p[1]) and torch.equal(got[3], p[3])
        assert aug.next_id == len(src)


def test_a_trainer_takes_an_augmented_batch():
    cfg = CONFIGS["a"]  # S = 4, T = 2, n_logits = 3: the vocabulary of shift 1
    tr = FusedTrainer.from_state_dict(make_weights(cfg, 40), dropout_p=0.0, seed=0, device=DEV)
    demos = SyntheticDemos(cfg["n_steps"] // 3 + 2, 16, cfg["dim_t"], cfg["dim_3d"], DEV, seed=3)
    aug = Augment(1, n_logits=cfg["n_logits"])
    batch = next(iter(demos.batches(32, augment=aug)))
    l_pol, l_val = tr.losses(*batch)
    assert np.isfinite(float(l_pol)) and np.isfinite(float(l_val)) and int(tr.status[0]) == 0


def test_augment_refuses_a_shift_that_is_not_the_datasets():
    demos = SyntheticDemos(4, 8, 1, 4, DEV, seed=3)
    with pytest.raises(Exception, match="shift"):
        demos.items(torch.arange(4, device=DEV), augment=Augment(1, shift=2))


# ---- 9. graph capture ------------------------------------------------------------------------------------------------
def test_captured_sample_and_apply_equal_eager():
    S, N, T = 4, 64, 2
    rng = np.random.default_rng(8)
    x = dev(rng.integers(-127, 128, size=(N, T, S, S, S)).astype(np.int8))
    a = dev(rng.integers(0, 3, size=(N, 3 * S)).astype(np.int8))
    sym = torch.zeros((N, 3 * S + 1), dtype=torch.uint8, device=DEV)
    out = torch.zeros((N, T, S, S, S), dtype=torch.bfloat16, device=DEV)
    act = torch.zeros((N, 3 * S), dtype=torch.int8, device=DEV)

    def run():  # one stream, one after the other: no parallel branches
        ops.symmetry_sample(N, S, DEV, seed=6, item_offset=100, out=sym)
        ops.symmetry_apply(x, a, sym, dtype=torch.bfloat16, out=out, actions=act)

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    want_sym = ops.symmetry_sample(N, S, DEV, seed=6, item_offset=100)
    want_out, want_act = ops.symmetry_apply(x, a, want_sym, dtype=torch.bfloat16)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        sym.zero_(), out.zero_(), act.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sym, want_sym) and torch.equal(out, want_out) and torch.equal(act, want_act)
