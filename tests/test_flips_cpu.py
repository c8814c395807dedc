"""CPU checks of the flip-graph walks (include/tensor_game_flips.h): the header, the exported symbols, the size checks and
the refusals of the host side of the library, and the host restatement's own invariants -- every step keeps the exact sum,
the bound and the stored form, the rank never rises, and from the standard <2,2,2> list walks reach Strassen's rank;
and that the gadget lists of flips_ref.py reach the rule events their slots name, which test_gpu_flips.py relies on."""
import ctypes as C
import re
import shutil
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import _lib, build, ops

import flips_ref as FR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_flips.h"
SEED = 0   # chosen on the CPU: with it 7 of the 16 walks below reach rank 7 (test_walks_reach_rank_7)


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_flips_header_is_plain_c_and_states_the_rules():
    text = HDR.read_text()
    for words in ("Stored form", "Reduce", "ascending (i, j) order", "ascending (i, j, m) order", "0x46000000",
                  "the higher slot first", "before it addresses", "slot j first", "keep their order"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_flip_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_flip_advance", "tg_flip_begin", "tg_flip_check"] == sorted(_lib.FLIP_SIGNATURES)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert (_lib.TG_FLIP_MAX_K, _lib.TG_FLIP_MAX_BOUND, _lib.TG_FLIP_MAX_STEPS) == (FR.MAX_K, 63, FR.MAX_STEPS)
    assert (_lib.TG_FLIP_BAD_LENGTH, _lib.TG_FLIP_BAD_RANGE, _lib.TG_FLIP_BAD_SRC) == (FR.BAD_LENGTH, FR.BAD_RANGE, FR.BAD_SRC)
    for name in ("flip_check", "flip_begin", "flip_advance"):
        assert name in ops.__all__
    assert "FlipWalks" in mat_mul_amd.__all__ and mat_mul_amd.flips.FlipWalks is mat_mul_amd.FlipWalks
    assert mat_mul_amd.reduce_archive is mat_mul_amd.flips.reduce_archive


# (M, W, K, S, shift, bound, step0, n_steps)
OK_SIZES = dict(M=4, W=4, K=8, S=4, shift=1, bound=1, step0=0, n_steps=16)
REFUSALS = [(dict(K=129), "K=129"), (dict(K=0), "K=0"), (dict(bound=0), "bound=0"), (dict(bound=64), "bound=64"),
            (dict(n_steps=0), "n_steps=0"), (dict(n_steps=65537), "n_steps=65537"),
            (dict(step0=2 ** 32 - 15), "step0 + n_steps"), (dict(step0=-1), "step0=-1"), (dict(S=33), "S=33"),
            (dict(S=0), "S=0"), (dict(shift=65), "shift=65"), (dict(shift=-1), "shift=-1"), (dict(W=-1), "W=-1")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_flip_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.flip_check(**{**OK_SIZES, **over})


def test_flip_check_takes_the_limits():
    ops.flip_check(0, 0, 128, 32, 64, 63, 2 ** 32 - 65536, 65536)
    ops.flip_check(1 << 20, 1 << 20, 1, 1, 0, 1, 0, 1)


def test_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    state = dict(cur=p(4099), cur_rank=p(8192), best=p(16387), best_rank=p(32768), best_step=p(65536), flips=p(131072),
                 state=p(262144))
    names = ("cur", "cur_rank", "best", "best_rank", "best_step", "flips", "state")
    begin, advance = _lib.lib.tg_flip_begin, _lib.lib.tg_flip_advance
    ok_b = dict(tokens=p(1), lengths=p(1024), M=4, src=None, W=4, K=8, S=4, shift=1, bound=1, **state, status=None)
    order_b = ("tokens", "lengths", "M", "src", "W", "K", "S", "shift", "bound", *names, "status")
    ok_a = dict(**state, W=4, K=8, S=4, shift=1, bound=1, seed=0, walk0=0, step0=0, n_steps=16)
    order_a = (*names, "W", "K", "S", "shift", "bound", "seed", "walk0", "step0", "n_steps")
    both = [(dict(K=129), b"K=129"), (dict(bound=0), b"bound=0"), (dict(bound=64), b"bound=64"), (dict(S=33), b"S=33"),
            (dict(shift=65), b"shift=65"), (dict(cur=None), b"null cur"), (dict(best_step=None), b"null best_step"),
            (dict(best=p(4099)), b"cur == best"), (dict(flips=p(131076)), b"flips not 8-byte"),
            (dict(state=p(262145)), b"state not 4-byte")]
    for over, words in both + [(dict(tokens=None), b"null tokens"), (dict(lengths=None), b"null lengths"),
                               (dict(W=5), b"W=5 != M=4"), (dict(tokens=p(4099)), b"in-place"),
                               (dict(src=p(12), W=9), b"src not 8-byte")]:
        kw = {**ok_b, **over}
        assert begin(*[kw[k] for k in order_b], None) == -1 and words in _lib.lib.tg_last_error(), over
    for over, words in both + [(dict(n_steps=0), b"n_steps=0"), (dict(n_steps=65537), b"n_steps=65537"),
                               (dict(step0=2 ** 32 - 15), b"step0 + n_steps"), (dict(step0=-1), b"step0=-1")]:
        kw = {**ok_a, **over}
        assert advance(*[kw[k] for k in order_a], None) == -1 and words in _lib.lib.tg_last_error(), over
    none = [None] * 7
    assert begin(None, None, 0, None, 0, 8, 4, 1, 1, *none, None, None) == 0      # W = 0 returns at once
    assert advance(*none, 0, 8, 4, 1, 1, 0, 0, 0, 16, None) == 0


def test_bindings_refuse_cpu_tensors():
    tok = torch.zeros((3, 4, 12), dtype=torch.int8)
    lengths = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip_begin(tok, lengths)
    st = {k: torch.zeros((3, 4, 12) if k in ("cur", "best") else (3,), dtype=torch.int8) for k in FR.STATE_NAMES}
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip_advance(st, 4)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FlipWalks.start(tok, lengths)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FlipWalks.from_state_dict({"version": 1}, "cpu")


def test_term_sum_is_exact_and_refuses_a_sum_outside_int8():
    rng = np.random.default_rng(3)
    tokens = rng.integers(-1, 4, size=(5, 6, 9)).astype(np.int8)         # values -2 .. 2 at shift 1
    lengths = np.array([0, 6, 3, 1, 5])
    got = mat_mul_amd.flips.term_sum(torch.from_numpy(tokens), torch.from_numpy(lengths), 1)
    assert got.dtype == torch.int8 and tuple(got.shape) == (5, 3, 3, 3)
    for m in range(5):
        assert np.array_equal(got[m].numpy(), FR.term_sum(tokens[m], int(lengths[m]), 3, 1))
    big = np.full((1, 6, 9), 5, dtype=np.int8)                           # 6 * 4^3 = 384
    with pytest.raises(_lib.TensorGameError, match="outside int8"):
        mat_mul_amd.flips.term_sum(torch.from_numpy(big), torch.tensor([6]), 1)


# ---- the restatement's invariants ------------------------------------------------------------------------------------
def _check_list(terms, S, bound, total):
    rows = FR.to_rows(terms, len(terms) + 1, S, 0)
    assert np.abs(rows.astype(int)).max(initial=0) <= bound
    assert np.array_equal(FR.term_sum(rows, len(terms), S, 0), total)                 # the exact sum
    for n0, n1, n2, s in terms:                                                       # the stored form
        for v in (n0, n1, n2):
            assert next(x for x in v if x) > 0
        assert s in (-1, 1)
    assert not rows[len(terms):].any()


@pytest.mark.parametrize("S, K, L, bound, shift, pool", [(4, 8, 8, 1, 1, 0), (9, 27, 27, 1, 1, 0), (5, 20, 17, 2, 2, 3)])
def test_every_step_keeps_the_sum_the_bound_and_the_stored_form(S, K, L, bound, shift, pool):
    rng = np.random.default_rng(S)
    tokens, L = FR.pool_list(rng, S, K, L, pool, shift) if pool else FR.standard_matmul(int(round(S ** 0.5)), shift)
    total = FR.term_sum(tokens, L, S, shift)
    st, status = FR.begin(tokens[None], [L], np.zeros(3, dtype=np.int64), bound, shift)
    assert status == 0 and (st["cur_rank"] <= L).all()
    last, trace = {}, []

    def on_step(w, t, terms):
        _check_list(terms, S, bound, total)
        assert len(terms) <= last.get(w, K)                                           # the rank never rises
        last[w] = len(terms)

    for step0 in range(0, 120, 40):                                                   # three launches
        FR.advance(st, SEED + 5, 10, step0, 40, bound, shift, trace=trace, on_step=on_step)
    for w in range(3):
        assert np.array_equal(FR.term_sum(st["cur"][w], st["cur_rank"][w], S, shift), total)
        assert np.array_equal(FR.term_sum(st["best"][w], st["best_rank"][w], S, shift), total)
        assert st["best_rank"][w] <= st["cur_rank"][w] and st["flips"][w] == sum(a for ww, _, _, a in trace if ww == w)
    assert len({(w, t) for w, t, _, _ in trace}) == len(trace) and trace      # one draw per step of a walking walk


def test_walks_from_the_standard_2x2_algorithm_reach_rank_7_and_are_then_stuck():
    tokens, L = FR.standard_matmul(2)
    total = FR.term_sum(tokens, L, 4, 1)
    st, status = FR.begin(tokens[None], [L], np.zeros(16, dtype=np.int64), 1, 1)
    assert status == 0 and (st["cur_rank"] == 8).all()                 # nothing merges in the standard algorithm
    FR.advance(st, SEED, 0, 0, 3000, 1, 1)
    won = st["best_rank"] == 7
    assert won.sum() >= 1, "no walk reached rank 7: the rules were restated wrongly"
    assert (st["best_rank"] >= 7).all() and np.array_equal(np.flatnonzero(won), [2, 5, 6, 7, 10, 13, 15])
    for w in np.flatnonzero(won):                                      # a Strassen-type list: no flip is left
        assert st["state"][w] == 1 and st["cur_rank"][w] == 7 and 0 < st["best_step"][w] <= 3000
        assert FR.matches(FR.from_rows(st["cur"][w], 7, 4, 1)) == []
        assert np.array_equal(FR.term_sum(st["best"][w], 7, 4, 1), total)
    assert (st["state"][~won] == 0).all() and (st["best_step"][~won] == 0).all()
    before = FR.copy_state(st)
    FR.advance(st, SEED, 0, 3000, 50, 1, 1)                            # a stuck walk stays as it is
    for k in FR.STATE_NAMES:
        assert np.array_equal(st[k][won], before[k][won]), k


def test_begin_restated_drops_normalises_and_reduces():
    S, K, shift = 3, 8, 1
    u, v, w = np.array([1, 0, -1]), np.array([0, 1, 1]), np.array([1, 1, 0])
    e0, e2, z = np.array([1, 0, 0]), np.array([0, 0, 1]), np.zeros(3, dtype=np.int64)
    rows = np.stack([np.concatenate(r) for r in (
        (u, z, w),                       # null
        (-u, v, e0), (u, -v, -e2),       # = -(u v e0) and +(u v e2): share (u, v), merge to u v (e2 - e0)
        (e0, e2, w), (e0, e2, -w),       # cancel
        (e2, e0, w), (e2, e0, w),        # would merge to 2w: leaves bound 1, stays
    )])
    tokens = np.zeros((1, K, 9), dtype=np.int8)
    tokens[0, :7] = rows + shift
    st, status = FR.begin(tokens, [7], None, 1, shift)
    assert status == 0 and st["cur_rank"][0] == 3 and st["state"][0] == 0
    got = st["cur"][0, :3].astype(int) - shift
    # slot 0: the merged term (the null term was dropped first); slot 1, 2: the pair that may not merge, moved in as the
    # cancelling pair left (slot j first, then slot i)
    assert np.array_equal(got[0], np.concatenate([u, v, e2 - e0]))
    assert np.array_equal(got[1], np.concatenate([e2, e0, w])) and np.array_equal(got[2], got[1])
    assert np.array_equal(FR.term_sum(st["cur"][0], 3, S, shift), FR.term_sum(tokens[0], 7, S, shift))
    st2, status2 = FR.begin(tokens, [7], None, 2, shift)               # bound 2: the last pair merges too
    assert st2["cur_rank"][0] == 2 and np.array_equal(st2["cur"][0, 1].astype(int) - shift, np.concatenate([e2, e0, 2 * w]))
    for lengths, src, bit in (([9], None, FR.BAD_LENGTH), ([-1], None, FR.BAD_LENGTH), ([7], [0, 1, -1], FR.BAD_SRC)):
        st3, status3 = FR.begin(tokens, lengths, src, 1, shift)
        assert status3 == bit and (st3["state"] == -1).sum() == (2 if src else 1) and not st3["cur"][st3["state"] == -1].any()
    tokens[0, 0, 0] = 2 + shift                                        # a value outside the bound, in a null term
    assert FR.begin(tokens, [7], None, 1, shift)[1] == FR.BAD_RANGE


# ---- the gadget lists reach the rule events their slots name ---------------------------------------------------------
def test_event_counters_change_nothing():
    tokens, L = FR.pool_list(np.random.default_rng(1), 5, 20, 17, 3, 2)
    plain, _ = FR.begin(tokens[None], [L], np.zeros(3, dtype=np.int64), 2, 2)
    counted = FR.copy_state(plain)
    events = Counter()
    FR.advance(plain, 4, 0, 0, 60, 2, 2)
    FR.advance(counted, 4, 0, 0, 60, 2, 2, events=events)
    for k in FR.STATE_NAMES:
        assert np.array_equal(plain[k], counted[k]), k
    assert set(events) <= set(FR.EVENTS) and events["accepted"] == plain["flips"].sum() > 0


def test_gadget_list_is_inert_but_for_its_gadgets():
    S, K, L, bound = FR.GADGET_S, 128, 100, FR.GADGET_BOUND
    slots = (64, 99, 98, 3, 63, 65, 97, 96)
    tokens, L = FR.gadget_list(np.random.default_rng(0), S, K, L, bound, bound, slots[:2], slots[2:4], slots[4:])
    terms = FR.from_rows(tokens, L, S, bound)
    ms = FR.matches(terms)
    assert ms and all(i in slots and j in slots for i, j, _ in ms)                    # every match is between gadgets
    assert sorted(m for i, j, m in ms if (i, j) == (64, 99)) == [0, 1, 2]             # the duplicate shares all three
    assert [m for i, j, m in ms if (i, j) == (3, 98)] == [0]                          # the hidden pair: mode 0 alone
    before = [list(t) for t in terms]
    FR.reduce(terms, bound)
    assert terms == before                                                            # begin's reduce merges nothing
    assert np.abs(tokens[:L].astype(int) - bound).max() == bound and not tokens[L:].any()


@pytest.mark.parametrize("name", list(FR.GADGET_CASES))
def test_gadget_walks_reach_the_events_of_their_slots(name):
    K, L, dup, hidden, quad, W, n_steps, by_slots = FR.GADGET_CASES[name]
    assert W <= 64 or L <= 64
    tokens, L, W, n_steps, st, events = FR.gadget_ref(name)
    print(name, {k: events[k] for k in FR.EVENTS})
    for e in FR.ALWAYS + by_slots:
        assert events[e] >= FR.MIN_EVENTS, (e, events[e])
    # both derived from the rules (NOTES.md): after a reduce no flip can null both terms, and a pair that cancels
    # inside a walk is the pair the flip just wrote
    assert events["null_both"] == 0 and events["cancel_with_third"] == 0
    total = FR.term_sum(tokens, L, FR.GADGET_S, FR.GADGET_BOUND)
    for w in range(W):
        assert np.array_equal(FR.term_sum(st["cur"][w], st["cur_rank"][w], FR.GADGET_S, FR.GADGET_BOUND), total)
        assert np.array_equal(FR.term_sum(st["best"][w], st["best_rank"][w], FR.GADGET_S, FR.GADGET_BOUND), total)


def test_gadget_cases_cover_the_placements():
    """Every slot pattern the kernel's two-terms-per-lane layout distinguishes is in some case."""
    cases = list(FR.GADGET_CASES.values())
    assert {(K, L) for K, L, *_ in cases} == {(8, 8), (64, 64), (128, 128), (128, 100)}
    dups = {(d, L) for _, L, d, *_ in cases}
    assert any(d == (0, 1) for d, L in dups) and any(d == (0, L - 1) for d, L in dups)
    assert any(d == (L - 2, L - 1) for d, L in dups) and {((63, 64), 128), ((62, 127), 128)} <= dups
    assert any(d == (64, L - 1) for d, L in dups)
    hidden = [(min(h), max(h), L) for _, L, _, h, *_ in cases]
    assert any(lo < 64 <= hi for lo, hi, L in hidden) and any(lo >= 64 for lo, hi, L in hidden)
    assert any(hi == L - 2 and L > 64 for lo, hi, L in hidden) and any(hi == L - 2 and L <= 64 for lo, hi, L in hidden)


@pytest.mark.parametrize("K", list(FR.ANTIPAIR_CASES))
def test_only_a_hand_written_unreduced_list_reaches_both_null(K):
    st, want, events = FR.antipair_ref(K)
    print(K, {k: events[k] for k in FR.EVENTS})
    n = FR.ANTIPAIR_WALKS
    for c, (L, p0, p1) in enumerate(FR.ANTIPAIR_CASES[K]):
        rows = slice(c * n, (c + 1) * n)
        # the walks whose one accepted flip removed the pair (two flips: the pair was doubled and cancelled later)
        both = (want["cur_rank"][rows] == L - 2) & (want["flips"][rows] == 1)
        assert both.sum() >= 4 and (want["state"][rows][both] == 1).all()
        start = st["cur"][c * n]
        # the higher slot first: the last term into p1, then the new last into p0.  (Removing p0 first would give other
        # rows, unless p1 is slot L-2: the inert terms are pairwise different.)
        moved = start.copy()
        for p in (p1, p0):
            L -= 1
            moved[p] = moved[L]
            moved[L] = 0
        for w in np.flatnonzero(both):
            assert np.array_equal(want["cur"][rows][w], moved)
    assert events["null_both"] >= FR.MIN_EVENTS
