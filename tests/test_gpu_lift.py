"""GPU checks of the sign lift (include/tensor_game_lift.h): ``ops.lift2_signs`` bit for bit against the host restatement
(lift_ref.py), all six outputs, on canary-guarded buffers with ``targets`` and ``tokens`` at odd addresses.  The Z_2
lists come from ``Mod2Walks`` on the device (which has its own bit-exact tests): walks from the standard <2,2,2> and
<3,3,3> lists; at S = 16, the workspace path, the standard <4,4,4> list and Strassen (x) Strassen built from a lifted
<2,2,2> result; S = 1, 5, 32 (bit 31 in use) and K = 128; planted errors; sharding by list0, independence of ws_lists,
more lists than workgroups, graph capture, W = 0; and end to end: what the walks reach enters a ``SolutionArchive``
through the archive's own proof."""
import numpy as np
import pytest
import torch

from mat_mul_amd import Mod2Walks, SolutionArchive, TensorGameError, flips, lift_signs, ops, reduce_archive_lifted

import flips_ref as FR
import lift_ref as LR
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0   # with it one walk of the S = 9 family needs a second try (asserted below); no other seed had to be looked for


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def odd(x, skew=1):
    """A copy of ``x`` ``skew`` bytes behind an aligned allocation (with canaries around it): (buffer, view)."""
    n = x.numel() * x.element_size()
    buf = torch.full((GUARD + skew + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + skew:GUARD + skew + n].view(x.dtype).view(x.shape)
    view.copy_(x)
    return buf, view


def check_odd(buf, n, what, skew=1):
    assert bool((buf[:GUARD + skew] == CANARY).all()) and bool((buf[GUARD + skew + n:] == CANARY).all()), what


class Outputs:
    """The six outputs in guarded buffers, ``tokens`` one byte behind a 16-byte boundary, filled with rubbish."""

    def __init__(self, W, K, S):
        self.n_tok = W * K * 3 * S
        self.tok_buf, self.tokens = odd(torch.full((W, K, 3 * S), 0x33, dtype=torch.int8, device=DEV))
        self.bufs, self.out = {}, {}
        for name in LR.OUT_NAMES:
            self.bufs[name], self.out[name] = guarded((W,), torch.int32)
            self.out[name].fill_(0x33333333)

    def check(self):
        check_odd(self.tok_buf, self.n_tok, "tokens")
        for name, buf in self.bufs.items():
            check_flat(buf, name)

    def numpy(self):
        return {"tokens": self.tokens.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.out.items()}}


def gpu_lift(targets, lists, ranks, S, shift=1, seed=SEED, list0=0, tries=32, ws_lists=None):
    """``ops.lift2_signs`` on unaligned inputs, guarded outputs and a guarded workspace of rubbish: dict of numpy."""
    W, K = lists.shape[0], lists.shape[1]
    o = Outputs(W, K, S)
    _, tgt = odd(dev(np.asarray(targets).astype(np.int8)))
    per_list = ops.lift2_workspace_bytes(K, S)
    ws_buf = ws = None
    if per_list:
        ws_lists = W if ws_lists is None else ws_lists
        ws_buf, ws = guarded((ws_lists * per_list,), torch.uint8)
        ws.fill_(0xA7)
        assert ws.data_ptr() % 16 == 0
    tokens, out = ops.lift2_signs(tgt, dev(lists), dev(np.asarray(ranks, dtype=np.int32)), tries=tries, seed=seed, list0=list0,
                                  shift=shift, workspace=ws, ws_lists=ws_lists if per_list else 0, tokens=o.tokens, **o.out)
    assert tokens is o.tokens and all(out[k] is o.out[k] for k in LR.OUT_NAMES)
    o.check()
    if ws_buf is not None:
        check_flat(ws_buf, "workspace")
    return o.numpy()


def assert_same(got, want, what=""):
    for k in ("status", "try_used", "unknowns", "sys_rank", "miss", "tokens"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k] if got[k].ndim == 1 else None, want[k] if want[k].ndim == 1 else None)


def assert_exact(out, targets, ranks, S, shift=1):
    """Independent of the restatement's elimination: every list with status 0 sums to its target exactly, has values in
    {-1, 0, 1} and zero rows behind its rank; every other list has all-zero rows."""
    for w in range(len(ranks)):
        if out["status"][w] == 0:
            R = int(ranks[w])
            assert np.array_equal(LR.tokens_sum(out["tokens"][w], R, S, shift), np.asarray(targets[w], dtype=np.int64)), w
            assert set(np.unique(out["tokens"][w, :R] - shift)) <= {-1, 0, 1} and not out["tokens"][w, R:].any()
        else:
            assert not out["tokens"][w].any(), w


# ---- the families (each computed once and shared; nobody changes them) ----------------------------------------------
_FAMILY = {}


def walked(n, steps):
    """(targets int8 (8,S,S,S), lists int32 (8,K,3), ranks int32 (8,)) of 8 device walks from the standard <n,n,n> list."""
    tokens, L = FR.standard_matmul(n)
    S = n * n
    walks = Mod2Walks.start(dev(tokens[None]), dev(np.array([L])), walks_per_list=8, seed=0).advance(steps)
    target = LR.tokens_sum(tokens, L, S, 1).astype(np.int8)
    assert not bool(walks.residual(dev(np.repeat(target[None], 8, 0))).any())
    return np.repeat(target[None], 8, 0), walks.best.cpu().numpy(), walks.best_rank.cpu().numpy()


def signed_lists(rng, S, K, W, L_of, density, bit31=False):
    """W random lists with values in {-1, 0, 1}: (exact targets, their masks mod 2, ranks).  The true signs are one
    lift; whether the sign system's tries find one is the restatement's to say."""
    targets = np.zeros((W, S, S, S), dtype=np.int64)
    lists = np.zeros((W, K, 3), dtype=np.int32)
    ranks = np.zeros(W, dtype=np.int32)
    for w in range(W):
        L = L_of(w)
        f = rng.choice([-1, 1], size=(L, 3, S)) * (rng.random((L, 3, S)) < density)
        f[:, :, 0] = np.where(f.any(axis=2), f[:, :, 0], 1)                     # no null term
        if bit31:
            f[:, :, S - 1] = rng.choice([-1, 1], size=(L, 3))
        tok = np.zeros((K, 3 * S), dtype=np.int8)
        tok[:L] = f.reshape(L, 3 * S) + 1
        targets[w] = LR.tokens_sum(tok, L, S, 1)
        lists[w] = LR.masks_of_tokens(tok, L, S, 1)
        ranks[w] = L
    assert np.abs(targets).max() <= 127
    return targets.astype(np.int8), lists, ranks


def family(name):
    """(targets, lists, ranks, S, the restatement's outputs at 32 tries, seed SEED, list0 0)"""
    if name in _FAMILY:
        return _FAMILY[name]
    rng = np.random.default_rng(21)
    if name == "S4":
        targets, lists, ranks = walked(2, 2000)
    elif name == "S9":
        targets, lists, ranks = walked(3, 4000)
    elif name == "S16":                                            # K = 64: the workspace path
        t4, L4 = FR.standard_matmul(4)
        target = LR.tokens_sum(t4, L4, 16, 1).astype(np.int8)
        s4_t, s4_l, s4_r, _, s4 = family("S4")
        seven = [w for w in range(8) if s4_r[w] == 7 and s4["status"][w] == 0]
        assert len(seven) >= 2
        lists = np.zeros((3, 64, 3), dtype=np.int32)
        lists[0] = LR.masks_of_tokens(t4, L4, 16, 1)
        wide = max(seven, key=lambda w: s4["unknowns"][w])         # the 7-term list with the largest support (14 a mode)
        for slot, (a, b) in ((1, (wide, wide)), (2, (seven[0], seven[0]))):              # Strassen (x) Strassen: 49 terms
            kron = LR.kron_lists(s4["tokens"][a], 7, 2, s4["tokens"][b], 7, 2, 1)
            assert np.array_equal(LR.tokens_sum(kron, 49, 16, 1), target)                # exact over the integers
            lists[slot, :49] = LR.masks_of_tokens(kron, 49, 16, 1)[:49]
        targets, ranks = np.repeat(target[None], 3, 0), np.array([64, 49, 49], dtype=np.int32)
    elif name == "S1":
        targets, lists, ranks = signed_lists(rng, 1, 4, 5, lambda w: w % 5, 1.0)
        targets[0, 0, 0, 0] += 2                                    # R = 0: a right-hand side that no column gives
    elif name == "S5":
        targets, lists, ranks = signed_lists(rng, 5, 7, 6, lambda w: 7 - w, 0.6)
    elif name == "S32":                                            # TG_MAX_S, bit 31 in every vector; the workspace path
        targets, lists, ranks = signed_lists(rng, 32, 6, 3, lambda w: 5 - w, 0.3, bit31=True)
        assert (lists[:, :3] < 0).all()
    elif name == "K128":                                           # more terms than a wavefront has lanes
        targets, lists, ranks = signed_lists(rng, 3, 128, 4, lambda w: (128, 100, 65, 64)[w], 0.7)
    S = targets.shape[1]
    _FAMILY[name] = (targets, lists, ranks, S, LR.lift(targets, lists, ranks, S, seed=SEED, tries=32))
    return _FAMILY[name]


# ---- the families against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S4", "S9", "S1", "S5", "K128"])
def test_lift_equals_the_restatement(name):
    targets, lists, ranks, S, want = family(name)
    print(name, {k: want[k].tolist() for k in LR.OUT_NAMES})
    assert ops.lift2_workspace_bytes(lists.shape[1], S) == 0      # the system lives in LDS
    got = gpu_lift(targets, lists, ranks, S)
    assert_same(got, want, name)
    assert_exact(got, targets, ranks, S)
    if name == "S4":                                               # the issue's condition: every walk's list lifts
        assert (got["status"] == 0).all() and ranks.min() == 7
    if name == "S9":
        assert set(got["status"]) == {0, 2} and (got["try_used"] > 0).any()
    if name == "S1":
        assert got["status"][0] == 2 and (got["unknowns"] == 3 * ranks).all()
    if name == "K128":
        assert got["unknowns"].max() > 500 and (got["sys_rank"] == 27).any()


@pytest.mark.parametrize("name, ws_lists", [("S16", 1), ("S16", 2), ("S16", 3), ("S32", 2)])
def test_lift_in_the_workspace_equals_the_restatement(name, ws_lists):
    targets, lists, ranks, S, want = family(name)
    print(name, {k: want[k].tolist() for k in LR.OUT_NAMES})
    assert ops.lift2_workspace_bytes(lists.shape[1], S) > 0 and ws_lists <= len(ranks)
    got = gpu_lift(targets, lists, ranks, S, ws_lists=ws_lists)    # ws_lists < W: a workgroup takes several lists
    assert_same(got, want, (name, ws_lists))                       # ... and the result does not depend on ws_lists
    assert_exact(got, targets, ranks, S)
    if name == "S16":
        assert (got["status"][0], got["try_used"][0], got["unknowns"][0]) == (0, 0, 192)     # b = 0: exact at try 0
        assert (got["status"][1], got["try_used"][1], got["unknowns"][1], got["sys_rank"][1]) == (0, 0, 588, 445)
        assert got["status"][2] == 3 and got["miss"][2] > 0        # ... and of another 7-term list does not, in 32 tries
    else:
        assert (lists < 0).any()                                   # bit 31 is in use


# ---- planted cases ---------------------------------------------------------------------------------------------------
def _planted():
    targets4, lists4, ranks4, _, ref4 = family("S4")
    w7 = int(np.flatnonzero(ranks4 == 7)[0])
    K, good_t, good_l = 8, targets4[w7].astype(np.int64), lists4[w7]
    n = 13
    targets = np.repeat(good_t[None], n, 0)
    lists = np.repeat(good_l[None], n, 0)
    ranks = np.full(n, 7, dtype=np.int32)
    targets[1, 1, 2, 3] += 1                                       # A: wrong mod 2
    targets[2, 1, 2, 3] += 4                                       # B: right mod 4, never exact
    targets[3, 1, 2, 3] += 2                                       # C: whatever the restatement says
    ranks[5], ranks[7] = -1, K + 1                                 # D: bad ranks between good rows
    for w in (9, 10, 11):                                          # E, F, G: R = 0
        ranks[w], targets[w] = 0, 0
    targets[10, 3, 0, 2], targets[11, 3, 0, 2] = 4, 2
    lists[12, 3:8] = good_l[2:7]                                   # H: a null term below R (slot 2), the rest moved up
    lists[12, 2] = (0, good_l[2, 1], good_l[2, 2])
    ranks[12] = 8
    return targets, lists, ranks


@pytest.mark.parametrize("tries", [32, 1])                         # I: tries = 1
def test_planted_errors_are_told_apart(tries):
    targets, lists, ranks = _planted()
    want = LR.lift(targets, lists, ranks, 4, seed=SEED, tries=tries)
    got = gpu_lift(targets, lists, ranks, 4, tries=tries)
    print({k: got[k].tolist() for k in LR.OUT_NAMES})
    assert_same(got, want, tries)
    assert_exact(got, targets, ranks, 4)
    st, miss = got["status"], got["miss"]
    assert (st[1], miss[1], got["unknowns"][1], got["sys_rank"][1]) == (1, 1, 0, 0)                    # A
    assert st[2] == 3 and miss[2] >= 1                                                                # B
    assert st[5] == st[7] == -1 and miss[5] == miss[7] == -1 and got["try_used"][5] == -1             # D
    for w in (0, 4, 6, 8):                                                                            # ... neighbours untouched
        assert st[w] == 0 and np.array_equal(got["tokens"][w], got["tokens"][0])
    assert (st[9], got["unknowns"][9], got["try_used"][9], miss[9]) == (0, 0, 0, 0)                   # E
    assert (st[10], miss[10]) == (3, 1) and (st[11], miss[11]) == (2, -1)                             # F, G
    assert st[12] == 0 and got["unknowns"][12] > got["unknowns"][0]                                   # H: its columns are free


# ---- properties ------------------------------------------------------------------------------------------------------
def test_rows_of_a_shard_equal_the_rows_of_the_whole():
    targets, lists, ranks, S, want = family("S9")
    assert (want["try_used"] > 0).any()                            # so the tries' draws, which depend on the id, matter
    g0 = 3
    part = gpu_lift(targets[g0:], lists[g0:], ranks[g0:], S, list0=g0)
    assert_same(part, {k: v[g0:] for k, v in want.items()}, "shard")
    moved = LR.lift(targets[:2], lists[:2], ranks[:2], S, seed=SEED + 1, list0=2 ** 40 + 5, tries=8)   # a 64-bit id, another seed
    assert_same(gpu_lift(targets[:2], lists[:2], ranks[:2], S, seed=SEED + 1, list0=2 ** 40 + 5, tries=8), moved, "moved")


def test_more_lists_than_workgroups():
    targets, lists, ranks, S, want = family("S4")
    assert (want["try_used"] == 0).all()                           # exact at try 0: the outputs do not depend on the id
    reps = 300                                                     # 2 400 lists: more than 8 workgroups on each of 256 CUs
    got = gpu_lift(np.tile(targets, (reps, 1, 1, 1)), np.tile(lists, (reps, 1, 1)), np.tile(ranks, reps), S, tries=2)
    assert_same(got, {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in want.items()}, "tiled")


@pytest.mark.parametrize("name", ["S9", "S16"])
def test_captured_graph_replays_to_the_same_outputs(name):
    targets, lists, ranks, S, want = family(name)
    W, K = lists.shape[0], lists.shape[1]
    o = Outputs(W, K, S)
    _, tgt = odd(dev(targets))
    dl, dr = dev(lists), dev(ranks)
    per_list = ops.lift2_workspace_bytes(K, S)
    ws = torch.empty((2 * per_list,), dtype=torch.uint8, device=DEV) if per_list else None

    def call():
        ops.lift2_signs(tgt, dl, dr, tries=32, seed=SEED, workspace=ws, ws_lists=2 if per_list else 0, tokens=o.tokens, **o.out)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(DEV).wait_stream(side)
    eager = o.numpy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    o.tokens.fill_(0x55)
    for k in LR.OUT_NAMES:
        o.out[k].fill_(0x55555555)
    graph.replay()
    torch.cuda.synchronize()
    o.check()
    assert_same(o.numpy(), eager, "eager")
    assert_same(o.numpy(), want, "restatement")


def test_no_lists_and_the_python_layer():
    empty = ops.lift2_signs(torch.zeros((0, 4, 4, 4), dtype=torch.int8, device=DEV),
                            torch.zeros((0, 8, 3), dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert empty[0].shape == (0, 8, 12) and all(v.shape == (0,) for v in empty[1].values())
    targets, lists, ranks, S, want = family("S16")
    with pytest.raises(TensorGameError, match="workspace must hold"):
        ops.lift2_signs(dev(targets), dev(lists), dev(ranks), workspace=torch.zeros(16, dtype=torch.uint8, device=DEV), ws_lists=1)
    with pytest.raises(TensorGameError, match="tries=0"):
        lift_signs(dev(lists), dev(ranks), dev(targets), tries=0)
    per_list = ops.lift2_workspace_bytes(64, 16)
    for cap in (1, 2 * per_list, 1 << 30):                        # one list at a time, two, all three
        res = lift_signs(dev(lists), dev(ranks), dev(targets), max_workspace_bytes=cap)
        assert res.tokens.dtype == torch.int8 and res.lengths.dtype == torch.int64
        assert_same({"tokens": res.tokens.cpu().numpy(), **{k: getattr(res, k).cpu().numpy() for k in LR.OUT_NAMES}}, want, cap)
        assert res.lengths.tolist() == np.where(want["status"] == 0, ranks, 0).tolist()
        assert res.lifted.tolist() == (want["status"] == 0).tolist()
    t9, l9, r9, _, want9 = family("S9")
    res = lift_signs(dev(l9), dev(r9).to(torch.int64), dev(t9))
    assert res.lifted.cpu().numpy().tolist() == (want9["status"] == 0).tolist()
    assert res.lengths.cpu().numpy().tolist() == np.where(want9["status"] == 0, r9, 0).tolist()


def test_mod2walks_lift_uses_the_walks_ids():
    tokens, L = FR.standard_matmul(3)
    walk0 = 2 ** 33 + 1
    walks = Mod2Walks.start(dev(tokens[None]), dev(np.array([L])), walks_per_list=8, seed=0, walk0=walk0).advance(1500)
    target = LR.tokens_sum(tokens, L, 9, 1).astype(np.int8)
    targets = np.repeat(target[None], 8, 0)
    res = walks.lift(dev(targets), tries=8)
    want = LR.lift(targets, walks.best.cpu().numpy(), walks.best_rank.cpu().numpy(), 9, seed=0, list0=walk0, tries=8)
    assert_same({"tokens": res.tokens.cpu().numpy(), **{k: getattr(res, k).cpu().numpy() for k in LR.OUT_NAMES}}, want)
    with pytest.raises(TensorGameError, match="'best' or 'cur'"):
        walks.lift(dev(targets), which="first")


# ---- end to end ------------------------------------------------------------------------------------------------------
def _archive_of_the_standard_list(n, capacity=64):
    std, L = FR.standard_matmul(n)
    lists, lengths = dev(std[None]), dev(np.array([L]))
    arch = SolutionArchive(S=n * n, max_rank=n ** 3, capacity=capacity, device=DEV, shift=1)
    rep = arch.add(flips.term_sum(lists, lengths, 1), lists, lengths)
    assert bool(rep.proven[0]) and int(arch.count) == 1 and int(arch.lowest_rank) == n ** 3
    return arch


def test_the_archive_holds_a_proven_7_term_list_after_walking_and_lifting():
    arch = _archive_of_the_standard_list(2)
    rep, mod2, res = reduce_archive_lifted(arch, 2_000)
    assert int(arch.lowest_rank) == 7                              # Strassen's rank, over the integers
    assert bool(mod2.proven.all()) and bool((res.lifted & (mod2.walks.best_rank == 7)).any())
    assert torch.equal(rep.proven, res.lifted)                     # proven by the archive itself, and nothing else is
    assert not bool(rep.residual_nnz[rep.fresh].any())
    tokens, rank, _, _ = arch.entries()
    assert int(arch.count) == 1 + int(rep.fresh.sum()) >= 2 and rank.min().item() == 7
    target = LR.tokens_sum(*FR.standard_matmul(2), 4, 1)
    for e in range(tokens.shape[0]):                               # and on the host, exactly
        assert np.array_equal(LR.tokens_sum(tokens[e].cpu().numpy(), int(rank[e]), 4, 1), target)
    assert reduce_archive_lifted(SolutionArchive(S=4, max_rank=8, capacity=4, device=DEV, shift=1), 10) is None


def test_the_3x3_archive_after_lifting_is_what_the_restatement_predicts():
    arch = _archive_of_the_standard_list(3)
    key0 = int(arch.entries()[2][0])
    rep, mod2, res = reduce_archive_lifted(arch, 4_000)
    walks = mod2.walks
    target = LR.tokens_sum(*FR.standard_matmul(3), 9, 1)
    targets = np.repeat(target[None], walks.W, 0)
    ranks = walks.best_rank.cpu().numpy()
    want = LR.lift(targets, walks.best.cpu().numpy(), ranks, 9, seed=0, list0=0, tries=32)
    assert_same({"tokens": res.tokens.cpu().numpy(), **{k: getattr(res, k).cpu().numpy() for k in LR.OUT_NAMES}}, want)
    lifted = want["status"] == 0
    assert lifted.any()
    assert rep.proven.cpu().numpy().tolist() == lifted.tolist()   # a list that did not lift proves nothing
    keys = rep.key.cpu().numpy()
    new = {int(k) for k in keys[lifted]} - {key0}                  # canonical forms the archive did not hold
    assert int(arch.count) == 1 + len(new) == 1 + int(rep.fresh.sum())
    assert int(arch.lowest_rank) == min(27, int(ranks[lifted].min()))
    assert not bool(rep.residual_nnz[rep.fresh].any())             # every added entry is proven
    tokens, rank, _, _ = arch.entries()
    for e in range(tokens.shape[0]):
        assert np.array_equal(LR.tokens_sum(tokens[e].cpu().numpy(), int(rank[e]), 9, 1), target)
