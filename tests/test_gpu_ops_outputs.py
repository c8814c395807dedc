"""Optional outputs of mat_mul_amd/ops.py on the MI355X: every entry that allocates an output when it is not given is
called twice on the same seeded inputs, once with the outputs left ``None`` and once with every output preallocated,
filled with the canary byte of guarded_buffers.py and surrounded by guard bytes.  The results are bit-identical, a given
output is the one returned, and the guards are untouched.  For the three masked calls the rows that the mask skips hold
zeros in the allocated outputs and the canary in the given ones.

The shapes are the smallest at which the argument rules differ: a dense game stride (S = 4: 64 bytes), a padded one
(S = 5 from ``alloc_states``: 128 bytes for 125), one game as a view into a wider buffer (its own stride is not read),
rings of one and of two frames, of one and of three games."""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, FusedTrainer, ops

from guarded_buffers import CANARY, check_flat, check_states, guarded, guarded_states
from net_ref import CONFIGS, make_inputs, make_weights
from train_ref import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
u8, i8, i32, i64, f32 = torch.uint8, torch.int8, torch.int32, torch.int64, torch.float32
FLOATS = (torch.float32, torch.float16, torch.bfloat16)
LAYOUTS = [(4, 3), (5, 3), (4, 1), (5, 1)]  # (S, B); B = 1 is game 1 of a buffer of three


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().reshape(-1).view(u8)


def same(a, b, what):
    """Two results of an entry: tensors of one shape, dtype and bit pattern; anything else equal."""
    if isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), what
    else:
        assert a == b, what


def stride_of(S):
    return -(-S ** 3 // 16) * 16


def states_in(st):
    """The games ``st`` (numpy int8 (B,S,S,S)) on the device in the layout of their LAYOUTS entry."""
    B, S = st.shape[:2]
    buf = ops.alloc_states(3 if B == 1 else B, S, DEV)
    view = buf[1:2] if B == 1 else buf
    view.copy_(dev(st))
    return view


class Flat:
    """A guarded output of ``shape`` / ``dtype`` whose payload holds the canary."""

    def __init__(self, shape, dtype):
        self.buf, self.t = guarded(shape, dtype)

    def check(self, what):
        check_flat(self.buf, what)


class Games:
    """A guarded state batch (..., S,S,S) with the game stride of ``alloc_states``: the games hold the canary too.  With
    ``lead = (1, ...)`` the output is game block 1 of three, and the other two must keep the canary."""

    def __init__(self, lead, S):
        self.single, self.S, self.stride = lead[0] == 1, S, stride_of(S)
        self.n = int(np.prod(lead))
        self.total = 3 * self.n if self.single else self.n
        self.buf, view = guarded_states(self.total, S, self.stride)
        self.all = view
        games = view[self.n:2 * self.n] if self.single else view
        self.t = games.unflatten(0, lead) if len(lead) > 1 else games

    def check(self, what):
        check_states(self.buf, self.total, self.S, self.stride, what)
        if self.single:
            rest = torch.cat((self.all[:self.n], self.all[2 * self.n:]))
            assert bool((rest.view(u8) == CANARY).all()), f"{what}: the games beside the view"


def twice(fn, make, outs, what):
    """``fn(**make())`` with the outputs left None and with the outputs ``outs`` (name -> Flat / Games) given: the same
    results bit for bit, the given tensors returned, the guards intact.  Returns (allocated results, given results)."""
    free = fn(**make())
    got = fn(**make(), **{name: o.t for name, o in outs.items()})
    torch.cuda.synchronize()
    free, got = (r if isinstance(r, tuple) else (r,) for r in (free, got))
    for name, o in outs.items():
        o.check(f"{what}: {name}")
    ptrs = {r.data_ptr() for r in got if isinstance(r, torch.Tensor)}
    assert all(o.t.data_ptr() in ptrs for o in outs.values()), f"{what}: a given output is not the one returned"
    assert len(free) == len(got)
    for i, (a, b) in enumerate(zip(free, got)):
        same(a, b, f"{what}: result {i}")
    return free, got


def inputs(S, B, K=None, seed=0):
    """(states numpy int8 (B,S,S,S) in {-2..2}, tokens numpy int8 (B,[K,]3S) in {-1,0,1})."""
    rng = np.random.default_rng(1000 * S + 10 * B + seed)
    st = rng.integers(-2, 3, size=(B, S, S, S)).astype(np.int8)
    shape = (B, 3 * S) if K is None else (B, K, 3 * S)
    return st, rng.choice([-1, 0, 1], p=[0.15, 0.7, 0.15], size=shape).astype(np.int8)


# ---- the state entries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B", LAYOUTS)
def test_step(S, B):
    st, ac = inputs(S, B)
    (out, _), _ = twice(ops.step, lambda: dict(state=states_in(st), actions=dev(ac)),
                        dict(out=Games((B,), S), done=Flat((B,), u8)), "step")
    wide = torch.zeros((B, 6 * S), dtype=i8, device=DEV)
    wide[:, ::2] = dev(ac)
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    for a, b in zip(ops.step(states_in(st), strided), ops.step(states_in(st), dev(ac))):
        same(a, b, "step: tokens as a non-contiguous view")
    same(out, ops.step(states_in(st), strided)[0], "step: the view and the guarded call")


@pytest.mark.parametrize("S,B", LAYOUTS)
def test_step_many_and_step_tracked(S, B):
    st, ac = inputs(S, B, K=3)
    twice(ops.step_many, lambda: dict(state=states_in(st), actions=dev(ac)),
          dict(out=Games((B,), S), done_step=Flat((B,), i32)), "step_many")

    def tracked():
        state = states_in(st)
        return dict(state=state, actions=dev(ac[:, 0]), nnz=ops.done(state, want_nnz=True)[1])

    twice(ops.step_tracked, tracked, dict(done=Flat((B,), u8)), "step_tracked")


@pytest.mark.parametrize("B", [3, 1])
def test_step_stream(B):
    st, ac = inputs(4, B, K=3)  # (the streamed stepper is built for S = 4, 16 and 25)
    steps = np.ascontiguousarray(ac.transpose(1, 0, 2))
    twice(ops.step_stream, lambda: dict(state=states_in(st), actions=dev(steps)), dict(done=Flat((3, B), u8)), "step_stream")


@pytest.mark.parametrize("S,B", LAYOUTS)
def test_expand(S, B):
    st, ac = inputs(S, B, K=3)
    make = lambda: dict(state=states_in(st), actions=dev(ac))  # noqa: E731
    flags = lambda: dict(out=Games((B, 3), S), done=Flat((B, 3), u8), changed=Flat((B, 3), u8))  # noqa: E731
    twice(ops.expand, make, flags(), "expand")
    twice(functools.partial(ops.expand, want_keys=True), make, flags(), "expand, keys allocated")
    twice(functools.partial(ops.expand, want_keys=True), make, dict(flags(), keys=Flat((B, 3), i64)), "expand, keys given")


@pytest.mark.parametrize("S,B", LAYOUTS)
def test_copy_states_change_basis_and_the_generators(S, B):
    st, ac = inputs(S, B, K=2)
    twice(ops.copy_states, lambda: dict(state=states_in(st)), dict(out=Games((B,), S)), "copy_states")
    basis = np.tile(np.eye(S, dtype=np.int32), (B, 3, 1, 1))
    basis[:, :, 0, S - 1] = 1
    basis[:, 1, 1, 0] = -1
    twice(ops.change_basis, lambda: dict(state=states_in(st), basis=dev(basis)), dict(out=Games((B,), S)), "change_basis")
    twice(ops.gen_from_factors, lambda: dict(actions=dev(ac), S=S), dict(out=Games((B,), S)), "gen_from_factors")
    twice(ops.gen_demos, lambda: dict(B=B, S=S, R=2, device=DEV, seed=11),
          dict(target=Games((B,), S), actions=Flat((B, 2, 3 * S), i8)), "gen_demos")


def test_seen():
    keys = torch.arange(1, 10, dtype=i64, device=DEV).reshape(3, 3)

    def make():
        table = ops.alloc_seen_table(64, DEV)
        ops.seen(keys[:2].contiguous(), table, insert=True)
        return dict(keys=keys, table=table, mask=torch.ones((3, 3), dtype=u8, device=DEV))

    (fresh,), _ = twice(ops.seen, make, dict(fresh=Flat((3, 3), u8)), "seen")
    assert fresh.cpu().tolist() == [[0, 0, 0], [0, 0, 0], [1, 1, 1]]


# ---- the history ring ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 5])
@pytest.mark.parametrize("T", [2, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_ring_entries(S, T, B):
    rng = np.random.default_rng(100 * S + 10 * T + B)
    frames = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    ac = rng.choice([-1, 0, 1], p=[0.15, 0.7, 0.15], size=(B, 3 * S)).astype(np.int8)

    def ring():
        r = ops.alloc_ring(B, S, T, DEV)
        r.copy_(dev(frames))
        return r

    for dtype in FLOATS:
        model_in = lambda: dict(out=Flat((B, T, S, S, S), dtype), scalars=Flat((B, 1), f32))  # noqa: E731
        (out, _), _ = twice(ops.emit_frames, lambda: dict(ring=ring(), head_slot=T - 1, t_step=2.0, dtype=dtype), model_in(),
                            f"emit_frames {dtype}")
        assert torch.equal(out[:, 0].to(i8), dev(frames[:, T - 1]))  # newest first: the head slot
        res, _ = twice(ops.step_emit, lambda: dict(ring=ring(), head_slot=T - 1, actions=dev(ac), t_step=2.0, dtype=dtype),
                       dict(model_in(), done=Flat((B,), u8)), f"step_emit {dtype}")
        assert res[3] == 0  # the new head slot, (T - 1 + 1) % T
        same(res[0][:, 0].to(i8), ops.step(dev(frames[:, T - 1]), dev(ac))[0], "step_emit: the new head")


# ---- items -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS + (torch.int8,))
def test_items(dtype):
    S, T, N = 4, 2, 5
    _, tokens = inputs(S, 3, K=3)  # n_demos = 3, R = 3
    tokens = dev(tokens)
    targets = ops.gen_from_factors(tokens, S)
    idx = torch.tensor([0, 8, 4, 2, 7], dtype=i64, device=DEV)
    outs = lambda: dict(out=Flat((N, T, S, S, S), dtype), scalars=Flat((N, 1), f32), actions=Flat((N, 3 * S), i8),  # noqa: E731
                        rewards=Flat((N, 1), f32))

    def flags():
        return dict(overflow=torch.zeros((N,), dtype=u8, device=DEV), status=torch.zeros((1,), dtype=torch.uint32, device=DEV))

    kept = []

    def demo():
        kept.append(flags())
        return dict(tokens=tokens, targets=targets, idx=idx, T=T, dtype=dtype, **kept[-1])

    def replay():
        kept.append(flags())
        return dict(idx=idx, T=T, S=S, device=DEV, tokens=tokens, targets=targets, direct_kind=0, dtype=dtype, **kept[-1])

    demo_free, _ = twice(ops.demo_items, demo, outs(), f"demo_items {dtype}")
    replay_free, _ = twice(ops.replay_items, replay, outs(), f"replay_items {dtype}")
    for a, b in zip(demo_free, replay_free):
        same(a, b, "demo_items and replay_items")
    for f in kept[1:]:
        same(f["overflow"], kept[0]["overflow"], "overflow")
        assert int(f["status"].view(i32)[0]) == 0
    assert demo_free[1].flatten().tolist() == [3.0, 1.0, 2.0, 1.0, 2.0]  # R - k of idx % R = 0, 2, 1, 2, 1


# ---- the network -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network():
    """(network of configuration a, frames int8 (3,T,4,4,4), scalars (3,dim_s)) -- shared, never written."""
    cfg = CONFIGS["a"]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 21), cfg["n_samples"], device=DEV)
    xx, ss = make_inputs(cfg, 3, 314)
    return cfg, net, dev(xx), dev(ss)


def skipped_rows(free, got, skipped, what):
    """Of the results of a masked call, the rows ``skipped`` hold zeros where the entry allocated and the canary where the
    output was given; the other rows are the same bits."""
    for i, (a, b) in enumerate(zip(free, got)):
        a, b = bits(a).reshape(a.shape[0], -1), bits(b).reshape(b.shape[0], -1)
        for row in range(a.shape[0]):
            if row in skipped:
                assert not a[row].any() and bool((b[row] == CANARY).all()), (what, i, row)
            else:
                assert torch.equal(a[row], b[row]), (what, i, row)


def test_net_torso_and_net_sample():
    cfg, net, xx, ss = network()
    B, k, S = 3, 2, cfg["dim_3d"]
    rows = torch.arange(B, dtype=i64, device=DEV)
    torso = lambda: dict(out=Flat((B, 3 * S * S, cfg["dim_c"]), f32))  # noqa: E731
    heads = lambda: dict(tokens=Flat((B, k, cfg["n_steps"]), i8), probs=Flat((B, k), f32), q=Flat((B,), f32))  # noqa: E731
    (ee,), _ = twice(ops.net_torso, lambda: dict(cfg=net.c, w=net.w, frames=xx, scalars=ss), torso(), "net_torso")
    sample = lambda: dict(cfg=net.c, w=net.w, ee=ee, rows=rows, k=k, seed=5, call_idx=7)  # noqa: E731
    plain, _ = twice(ops.net_sample, sample, heads(), "net_sample")

    flags = torch.tensor([1, 0, 1], dtype=u8, device=DEV)
    given = torso()
    free = ops.net_torso(net.c, net.w, xx, ss, flags=flags, need=1)
    got = ops.net_torso(net.c, net.w, xx, ss, flags=flags, need=1, **{n: o.t for n, o in given.items()})
    torch.cuda.synchronize()
    given["out"].check("net_torso masked")
    assert got.data_ptr() == given["out"].t.data_ptr()
    skipped_rows((free,), (got,), {1}, "net_torso masked")
    assert torch.equal(bits(free[0]), bits(ee[0])) and torch.equal(bits(free[2]), bits(ee[2]))

    given = heads()
    free = ops.net_sample(**sample(), flags=flags, need=1)
    got = ops.net_sample(**sample(), flags=flags, need=1, **{n: o.t for n, o in given.items()})
    torch.cuda.synchronize()
    for name, o in given.items():
        o.check(f"net_sample masked: {name}")
    assert [t.data_ptr() for t in got] == [given[n].t.data_ptr() for n in ("tokens", "probs", "q")]
    skipped_rows(free, got, {1}, "net_sample masked")
    for a, b in zip(free, plain):
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[2]), bits(b[2]))


def test_net_loss_grad():
    cfg = CONFIGS["a"]
    tr = FusedTrainer.from_state_dict(make_weights(cfg, 21), dropout_p=0.0, device=DEV)
    batch = tuple(dev(x) for x in make_batch(cfg, 3, 40))
    ws = tr.workspace(3)
    grads = []

    def make():
        grads.append(torch.zeros_like(tr.params.detach()))
        return dict(cfg=tr.c, theta=tr.params.detach(), pos_fix=tr.pos_fix, frames=batch[0], scalars=batch[1],
                    g_action=batch[2], g_value=batch[3], workspace=ws, grad=grads[-1])

    (losses, status), _ = twice(ops.net_loss_grad, make, dict(losses=Flat((2,), f32), status=Flat((1,), i32)), "net_loss_grad")
    assert int(status[0]) == 0 and bool(torch.isfinite(losses).all())
    same(grads[0], grads[1], "net_loss_grad: the gradient")


# ---- rollouts --------------------------------------------------------------------------------------------------------
def test_rollout_advance():
    S, T, n, B = 4, 2, 2, 4
    rng = np.random.default_rng(9)
    frames = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    tokens = rng.choice([-1, 0, 1], p=[0.15, 0.7, 0.15], size=(B, 3 * S)).astype(np.int8)
    kept = []

    def make(solved=False):
        rec = ops.rollout_records(B // n, S, DEV)
        if solved:
            rec[2][0] = 0  # group 0 was solved at step 0: its rows 0 and 1 are not stepped
        kept.append(dict(frames=dev(frames), tokens=dev(tokens), n=n, step=0, records=rec,
                         scalars=torch.ones((B, 1), dtype=f32, device=DEV)))
        return kept[-1]

    (nnz,), _ = twice(ops.rollout_advance, make, dict(nnz=Flat((B,), i32)), "rollout_advance")
    for name in ("frames", "scalars"):
        same(kept[0][name], kept[1][name], f"rollout_advance: {name}")
    for a, b in zip(kept[0]["records"], kept[1]["records"]):
        same(a, b, "rollout_advance: records")
    assert torch.equal(nnz, ops.done(kept[0]["frames"][:, 0].contiguous(), want_nnz=True)[1])

    def masked():
        return dict(make(solved=True), stop_solved=True, active=torch.ones((B,), dtype=u8, device=DEV))

    given = Flat((B,), i32)
    free = ops.rollout_advance(**masked())
    got = ops.rollout_advance(**masked(), nnz=given.t)
    torch.cuda.synchronize()
    given.check("rollout_advance masked: nnz")
    assert got.data_ptr() == given.t.data_ptr()
    skipped_rows((free,), (got,), {0, 1}, "rollout_advance masked")
    assert torch.equal(free[2:], nnz[2:])  # the group still unsolved is stepped as by the plain call
    same(kept[2]["frames"], kept[3]["frames"], "rollout_advance masked: frames")
    assert torch.equal(kept[2]["frames"][:2], dev(frames[:2]))  # the solved group's rows are not written
