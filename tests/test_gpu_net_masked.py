"""The row-masked network entries (tg_net_torso_masked, tg_net_sample_masked) and the self-play driver that uses them,
on the MI355X, at the configurations a, b (S = 4, 3), a9 (S = 9, the per-game torso kernel) and a16 (S = 16: a game is S
torso workgroups and, with k = 8 at R = 4, two decoder workgroups): active rows equal the plain call bit for bit,
inactive rows are not written, the mask is read on the device when a captured graph replays, self-play with
``policy(seed, masked=True)`` equals self-play with ``policy(seed)``, and so does the driver's retry path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import FusedAlphaTensor, SyntheticDemos, _lib, ops, search

from guarded_buffers import GUARD, check_flat, guarded
from net_ref import CONFIGS as CONFIGS_S4
from net_ref import make_inputs, make_weights
from net_s9_ref import CONFIGS as CONFIGS_S9
from net_s16_ref import CONFIGS as CONFIGS_S16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {"a": CONFIGS_S4["a"], "b": CONFIGS_S4["b"], "a9": CONFIGS_S9["a9"], "a16": CONFIGS_S16["a16"]}
CASES = list(CONFIGS)
PATTERN = 0xA5
SEED, CALL = 5, 7
EXPAND, RETRY, PENDING = search.EXPAND, search.RETRY, search.PENDING


@functools.lru_cache(maxsize=None)
def setup(name):
    """(configuration, network, frames int8 (6,T,S,S,S), scalars (6,dim_s)) -- shared, never written."""
    cfg = CONFIGS[name]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 21), cfg["n_samples"], device=DEV)
    xx, ss = make_inputs(cfg, 6, 314)
    return cfg, net, torch.from_numpy(xx).to(DEV), torch.from_numpy(ss).to(DEV)


@functools.lru_cache(maxsize=None)
def plain(name, B):
    """(ee, tokens, probs, q) of the plain entries for the first B states, rows keyed 0 .. B-1."""
    cfg, net, xx, ss = setup(name)
    ee = net.torso(xx[:B], ss[:B])
    return (ee,) + tuple(net.sample(ee, seed=SEED, call=CALL))


def patterned(shape, dtype):
    """A guarded buffer whose payload holds the byte PATTERN."""
    buf, t = guarded(shape, dtype)
    buf[GUARD:-GUARD].fill_(PATTERN)
    return buf, t


def raw(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


def run_masked(name, B, flags, need, via_abi=False):
    """Masked torso + sample on the first B states into patterned, guarded buffers: (ee, tokens, probs, q).  ``via_abi``
    calls the two C entries directly, which is the only way to hand them NULL flags."""
    cfg, net, xx, ss = setup(name)
    k, S = cfg["n_samples"], cfg["dim_3d"]
    shapes = (((B, 3 * S * S, cfg["dim_c"]), torch.float32), ((B, k, cfg["n_steps"]), torch.int8),
              ((B, k), torch.float32), ((B,), torch.float32))
    bufs, (ee, tokens, probs, q) = zip(*(patterned(s, d) for s, d in shapes))
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    x, s = xx[:B].contiguous(), ss[:B].contiguous()
    if via_abi:
        st = ops._stream(torch.device(DEV))
        _lib.call("tg_net_torso_masked", C.byref(net.c), ops._ptr(net.w), ops._ptr(x), 1, ops._ptr(s), ops._ptr(ee), B,
                  ops._ptr(fl), need, st)
        _lib.call("tg_net_sample_masked", C.byref(net.c), ops._ptr(net.w), ops._ptr(ee), ops._ptr(rows), B, k, SEED, CALL,
                  None, ops._ptr(tokens), ops._ptr(probs), ops._ptr(q), ops._ptr(fl), need, st)
    else:
        assert ops.net_torso(net.c, net.w, x, s, out=ee, flags=fl, need=need).data_ptr() == ee.data_ptr()
        ops.net_sample(net.c, net.w, ee, rows, k, SEED, CALL, tokens=tokens, probs=probs, q=q, flags=fl, need=need)
    torch.cuda.synchronize()
    for b, what in zip(bufs, ("ee", "tokens", "probs", "q")):
        check_flat(b, what)
    return ee, tokens, probs, q


def check(name, flags, need, via_abi=False):
    """Active rows hold the plain call's bits, inactive rows still hold PATTERN; returns the active rows."""
    B = len(flags)
    active = [g for g, f in enumerate(flags) if (f & need) == need]
    for got, want, what in zip(run_masked(name, B, flags, need, via_abi), plain(name, B), ("ee", "tokens", "probs", "q")):
        got, want = raw(got), raw(want)
        for g in range(B):
            if g in active:
                assert torch.equal(got[g], want[g]), (name, what, g)
            else:
                assert bool((got[g] == PATTERN).all()), (name, what, g)
    return active


@pytest.mark.parametrize("name", CASES)
def test_active_rows_equal_the_plain_call_and_inactive_rows_are_untouched(name):
    cfg, net, _, _ = setup(name)
    assert cfg["n_samples"] == 8 or name == "b"  # at a16, k = 8 is two decoder workgroups per game (R = 4)
    assert check(name, [129, 0, 1, 137, 128], 129) == [0, 3]


@pytest.mark.parametrize("name", CASES)
def test_null_flags_equal_the_plain_call(name):
    for got, want in zip(run_masked(name, 5, None, 0, via_abi=True), plain(name, 5)):
        assert torch.equal(raw(got), raw(want))
    assert check(name, [129, 0, 1, 137, 128], 129, via_abi=True) == [0, 3]  # and the same entries with a mask


@pytest.mark.parametrize("name", CASES)
def test_no_active_row_one_row_and_the_retry_bit_alone(name):
    assert check(name, [0, 1, 128, 127, 126], 129) == []              # nothing to do: returns 0, writes nothing
    assert check(name, [129], 129) == [0] and check(name, [128], 129) == []  # B = 1, active and inactive
    assert check(name, [8, 1, 9, 129, 136, 247], RETRY) == [0, 2, 4]   # need = 8 selects on the RETRY bit alone
    assert check(name, [255, 129, 137], 255) == [0]                    # every bit needed


def test_allocated_outputs_are_zero_where_inactive_and_need_is_checked():
    cfg, net, xx, ss = setup("a")
    fl = torch.tensor([129, 0, 1, 137, 128], dtype=torch.uint8, device=DEV)
    ee = net.torso(xx[:5], ss[:5], flags=fl, need=129)
    tokens, probs, q = net.sample(ee, seed=SEED, call=CALL, flags=fl, need=129)
    for got, want in zip((ee, tokens, probs, q), plain("a", 5)):
        assert torch.equal(raw(got)[[0, 3]], raw(want)[[0, 3]]) and not bool(raw(got)[[1, 2, 4]].any())
    with pytest.raises(_lib.TensorGameError, match="need=0"):
        net.torso(xx[:5], ss[:5], flags=fl, need=0)
    with pytest.raises(_lib.TensorGameError, match="flags"):
        net.torso(xx[:5], ss[:5], flags=fl[:4], need=1)


def test_a_captured_graph_follows_the_flags_tensor():
    """One chain of two launches, captured once: the mask is read when the kernels run."""
    cfg, net, xx, ss = setup("a")
    B, k = 6, cfg["n_samples"]
    x, s = xx[:B].contiguous(), ss[:B].contiguous()
    rows = torch.arange(B, device=DEV, dtype=torch.int64)
    fl = torch.zeros((B,), dtype=torch.uint8, device=DEV)
    ee = torch.empty((B, 48, cfg["dim_c"]), dtype=torch.float32, device=DEV)
    tokens = torch.empty((B, k, cfg["n_steps"]), dtype=torch.int8, device=DEV)
    probs = torch.empty((B, k), dtype=torch.float32, device=DEV)
    q = torch.empty((B,), dtype=torch.float32, device=DEV)

    def both():
        ops.net_torso(net.c, net.w, x, s, out=ee, flags=fl, need=129)
        ops.net_sample(net.c, net.w, ee, rows, k, SEED, CALL, tokens=tokens, probs=probs, q=q, flags=fl, need=129)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        both()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for flags in ([129, 0, 1, 137, 128, 255], [0, 129, 129, 2, 131, 128]):
        fl.copy_(torch.tensor(flags, dtype=torch.uint8, device=DEV))
        for t in (ee, tokens, probs, q):
            t.view(torch.uint8).fill_(PATTERN)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((ee, tokens, probs, q), run_masked("a", B, flags, 129)):
            assert torch.equal(raw(got), raw(want)), flags
        assert bool((raw(q)[1] == PATTERN).all()) != bool((raw(q)[0] == PATTERN).all())  # the two contents differ there


class Counting:
    """A masked policy that counts, from the flags it is handed, the rows it is asked for."""
    takes_flags = True

    def __init__(self, inner):
        self.inner, self.calls, self.retries, self.rows, self.total = inner, 0, 0, 0, 0

    def __call__(self, frames, scalars, games, flags, need, out):
        assert games.shape[0] == flags.shape[0] == frames.shape[0] and bool((games == torch.arange(len(games), device=DEV)).all())
        self.calls += 1
        self.retries += int(need == RETRY)
        self.rows += int(((flags & need) == need).sum())
        self.total += flags.shape[0]
        return self.inner(frames, scalars, games, flags=flags, need=need, out=out)


def self_play(name, start, n_sim, max_actions, masked):
    cfg = CONFIGS[name]
    net = FusedAlphaTensor.from_state_dict(make_weights(cfg, 21), cfg["n_samples"], device=DEV)  # a fresh counter
    B, T, S, k = start.shape[0], start.shape[1], start.shape[2], cfg["n_samples"]
    forest = search.SearchForest(B, S, T, k=k, max_actions=max_actions, n_sim=n_sim, device=DEV)
    pol = net.policy(seed=3, masked=True) if masked else net.policy(seed=3)
    if masked:
        pol = Counting(pol)
    out = search.actor_prediction(pol, start, max_actions, n_sim=n_sim, n_bar=100, n_logits=3, k=k, forest=forest)
    return [t.cpu() for t in out] + [forest.status.cpu(), forest.final_heads().cpu()], pol


@pytest.mark.parametrize("name, B, n_sim, max_actions, rank", [("a", 64, 8, 4, 3), ("a16", 4, 4, 2, 2)])
def test_self_play_with_the_masked_policy_equals_the_plain_policy(name, B, n_sim, max_actions, rank):
    cfg = CONFIGS[name]
    S, T = cfg["dim_3d"], cfg["dim_t"]
    assert T == 2 and cfg["n_samples"] == 8
    demos = SyntheticDemos(rank, B, 1, S, device=DEV, seed=3)
    start = torch.zeros((B, T, S, S, S), dtype=torch.int8, device=DEV)
    start[:, 0] = demos.target_tensor.reshape(B, S, S, S)
    want, _ = self_play(name, start, n_sim, max_actions, masked=False)
    got, pol = self_play(name, start, n_sim, max_actions, masked=True)
    for a, b, what in zip(got, want, ("states", "policy", "rewards", "lengths", "status", "final heads")):
        assert a.dtype == b.dtype and torch.equal(raw(a), raw(b)), (name, what)
    print(f"{name}: {pol.calls} policy calls ({pol.retries} retries), {pol.rows} of {pol.total} rows needed "
          f"({pol.rows / pol.total:.3f})")
    assert pol.calls >= n_sim and 0 < pol.rows <= pol.total
    if name == "a":  # the mask left rows out: the test cannot pass with a mask that selects everything
        assert pol.rows < pol.total


class FlaggedKeyed:
    """search.keyed_policy behind the masked calling convention: the rows with the needed bits go into ``out``."""
    takes_flags = True

    def __init__(self, inner):
        self.inner, self.retries = inner, 0

    def __call__(self, frames, scalars, games, flags, need, out):
        self.retries += int(need == RETRY)
        assert need in (EXPAND | PENDING, RETRY)
        tokens, _, q = self.inner(frames, scalars, games)
        act = (flags & need) == need
        out[0].copy_(torch.where(act[:, None, None], tokens, out[0]))
        out[1].copy_(torch.where(act, q, out[1]))
        return out[0], None, out[1]


class Copies(FlaggedKeyed):
    """Breaks the convention: returns copies instead of the buffers it was given."""

    def __call__(self, *args, **kw):
        tokens, _, q = super().__call__(*args, **kw)
        return tokens.clone(), None, q.clone()


def test_the_retry_path_of_the_masked_driver_equals_the_plain_driver():
    S, B, T, k, n_sim, max_actions = 4, 32, 1, 4, 8, 4
    rng = np.random.default_rng(32)
    st = np.zeros((B, T, S, S, S), np.int8)
    st[:, 0] = rng.choice([-1, 0, 1], p=[0.2, 0.6, 0.2], size=(B, S, S, S))
    start = torch.from_numpy(st).to(DEV)
    pool = torch.ones((6, 3 * S), dtype=torch.int8)  # token 1 is the value 0: every pool action is a null action
    runs = []
    for masked in (False, True):
        forest = search.SearchForest(B, S, T, k=k, max_actions=max_actions, n_sim=n_sim, device=DEV)
        pol = search.keyed_policy(forest, pool, seed=9)
        if masked:
            pol = FlaggedKeyed(pol)
        out = search.actor_prediction(pol, start, max_actions, n_sim=n_sim, n_bar=4, n_logits=3, k=k, forest=forest)
        runs.append([t.cpu() for t in out] + [t.cpu() for t in forest.root_stats()] + [forest.status.cpu()])
    assert pol.retries > 0  # some first attempt left no survivor
    for a, b in zip(*runs):
        assert torch.equal(raw(a), raw(b))
    with pytest.raises(_lib.TensorGameError, match="buffers of `out`"):  # the driver reads `out`, nothing else
        forest.play(Copies(search.keyed_policy(forest, pool, seed=9)), start, n_sim)
