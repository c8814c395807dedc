"""CPU checks of the flip-graph walks over Z_2 (include/tensor_game_flips_mod2.h): the header, the exported symbols, the
size checks and refusals of the host side of the library, and the host restatement's own invariants -- every step of
every walk keeps the XOR of its terms, over traces that hold flips of all four variants, plus steps of all twelve,
merges, cancelling pairs and a stuck walk -- and the seed with which walks from the standard <2,2,2> list reach rank 7."""
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

import flips_mod2_ref as F2
import flips_ref as FR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_flips_mod2.h"
SEED = 0          # chosen here: with it 13 of the 16 walks below reach rank 7 inside STEPS_TO_7 steps of the restatement
STEPS_TO_7 = 2000


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_mod2_header_is_plain_c_and_states_the_rules():
    text = HDR.read_text()
    for words in ("Reduce", "ascending (i, j) order", "(i, j, d) order", "0x46320000", "the higher slot first",
                  "the highest slot first", "before it addresses", "slot j first", "keep their order", "never refused",
                  "Steps are consecutive", "never changes", "plus_after == 0", "plus_slack == 0"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_mod2_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_flip2_advance", "tg_flip2_begin", "tg_flip2_check", "tg_flip2_residual"] == sorted(_lib.FLIP2_SIGNATURES)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert _lib.TG_FLIP2_DOMAIN == F2.DOMAIN == 0x46320000 and "0x46320000u" in HDR.read_text()
    assert (_lib.TG_FLIP_BAD_LENGTH, _lib.TG_FLIP_BAD_SRC) == (F2.BAD_LENGTH, F2.BAD_SRC)
    for name in ("flip2_check", "flip2_begin", "flip2_advance", "flip2_residual"):
        assert name in ops.__all__
    assert [n for n, _ in ops._FLIP2_STATE] == list(F2.STATE_NAMES)
    assert "Mod2Walks" in mat_mul_amd.__all__ and mat_mul_amd.flips_mod2.Mod2Walks is mat_mul_amd.Mod2Walks
    assert mat_mul_amd.reduce_archive_mod2 is mat_mul_amd.flips_mod2.reduce_archive_mod2
    assert mat_mul_amd.reduce_mod2 is mat_mul_amd.flips_mod2.reduce_mod2
    assert "walks over Z_2" not in (mat_mul_amd.flips.__doc__ or "")


# (M, W, K, S, shift, step0, n_steps, plus_after, plus_slack)
OK_SIZES = dict(M=4, W=4, K=8, S=4, shift=1, step0=0, n_steps=16, plus_after=0, plus_slack=1)
REFUSALS = [(dict(K=129), "K=129"), (dict(K=0), "K=0"), (dict(S=33), "S=33"), (dict(S=0), "S=0"),
            (dict(n_steps=0), "n_steps=0"), (dict(n_steps=65537), "n_steps=65537"),
            (dict(step0=2 ** 32 - 15), "step0 + n_steps"), (dict(step0=-1), "step0=-1"),
            (dict(plus_after=-1), "plus_after=-1"), (dict(plus_after=2 ** 31), "plus_after=2147483648"),
            (dict(plus_slack=-1), "plus_slack=-1"), (dict(plus_slack=129), "plus_slack=129"),
            (dict(shift=65), "shift=65"), (dict(shift=-1), "shift=-1"), (dict(W=-1), "W=-1"), (dict(M=-1), "M=-1")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_flip2_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.flip2_check(**{**OK_SIZES, **over})


def test_flip2_check_takes_the_limits():
    ops.flip2_check(0, 0, 128, 32, 64, 2 ** 32 - 65536, 65536, 2 ** 31 - 1, 128)
    ops.flip2_check(1 << 20, 1 << 20, 1, 1, 0, 0, 1, 0, 0)


def test_mod2_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    names = F2.STATE_NAMES
    state = dict(cur=p(4096), cur_rank=p(8192), best=p(16384), best_rank=p(32768), best_step=p(65536), flips=p(131072),
                 state=p(262144), since=p(524288), pluses=p(1048576))
    begin, advance, residual = _lib.lib.tg_flip2_begin, _lib.lib.tg_flip2_advance, _lib.lib.tg_flip2_residual
    ok_b = dict(tokens=p(1), lengths=p(1024), M=4, src=None, W=4, K=8, S=4, shift=1, **state, status=None)
    order_b = ("tokens", "lengths", "M", "src", "W", "K", "S", "shift", *names, "status")
    ok_a = dict(**state, W=4, K=8, S=4, seed=0, walk0=0, step0=0, n_steps=16, plus_after=0, plus_slack=1)
    order_a = (*names, "W", "K", "S", "seed", "walk0", "step0", "n_steps", "plus_after", "plus_slack")
    both = [(dict(K=129), b"K=129"), (dict(S=33), b"S=33"), (dict(cur=None), b"null cur"), (dict(since=None), b"null since"),
            (dict(pluses=None), b"null pluses"), (dict(best=p(4096)), b"cur == best"), (dict(cur=p(4098)), b"cur not 4-byte"),
            (dict(flips=p(131076)), b"flips not 8-byte"), (dict(since=p(524289)), b"since not 4-byte"),
            (dict(pluses=p(1048580)), b"pluses not 8-byte")]
    for over, words in both + [(dict(tokens=None), b"null tokens"), (dict(lengths=None), b"null lengths"),
                               (dict(W=5), b"W=5 != M=4"), (dict(shift=65), b"shift=65"),
                               (dict(src=p(12), W=9), b"src not 8-byte")]:
        kw = {**ok_b, **over}
        assert begin(*[kw[k] for k in order_b], None) == -1 and words in _lib.lib.tg_last_error(), over
    for over, words in both + [(dict(n_steps=0), b"n_steps=0"), (dict(n_steps=65537), b"n_steps=65537"),
                               (dict(step0=2 ** 32 - 15), b"step0 + n_steps"), (dict(plus_after=-1), b"plus_after=-1"),
                               (dict(plus_slack=129), b"plus_slack=129")]:
        kw = {**ok_a, **over}
        assert advance(*[kw[k] for k in order_a], None) == -1 and words in _lib.lib.tg_last_error(), over
    ok_r = dict(targets=p(1), lists=p(4096), ranks=p(8192), M=4, K=8, S=4, residual=p(16384))
    order_r = ("targets", "lists", "ranks", "M", "K", "S", "residual")
    for over, words in [(dict(K=0), b"K=0"), (dict(S=33), b"S=33"), (dict(targets=None), b"null targets"),
                        (dict(lists=None), b"null lists"), (dict(ranks=None), b"null ranks"),
                        (dict(residual=None), b"null residual"), (dict(lists=p(4097)), b"lists not 4-byte"),
                        (dict(residual=p(16386)), b"residual not 4-byte")]:
        kw = {**ok_r, **over}
        assert residual(*[kw[k] for k in order_r], None) == -1 and words in _lib.lib.tg_last_error(), over
    none = [None] * 9
    assert begin(None, None, 0, None, 0, 8, 4, 1, *none, None, None) == 0      # W = 0 returns at once
    assert advance(*none, 0, 8, 4, 0, 0, 0, 16, 0, 1, None) == 0
    assert residual(None, None, None, 0, 8, 4, None, None) == 0


def test_mod2_bindings_refuse_cpu_tensors():
    tok = torch.zeros((3, 4, 12), dtype=torch.int8)
    lengths = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip2_begin(tok, lengths)
    st = {k: torch.zeros((3, 4, 3) if k in ("cur", "best") else (3,), dtype=dt) for k, dt in ops._FLIP2_STATE}
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip2_advance(st, 4, 4)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip2_residual(torch.zeros((3, 4, 4, 4), dtype=torch.int8), st["cur"], st["cur_rank"])
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.Mod2Walks.start(tok, lengths)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.Mod2Walks.from_state_dict({"version": 1}, "cpu")


# ---- the restatement's invariants ------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(5)
    # (tokens, L, S, shift, W, steps per launch, plus_after, plus_slack)
    return {"2x2": (*FR.standard_matmul(2), 4, 1, 8, 700, 0, 1),
            "2x2 plus": (*FR.standard_matmul(2, K=9), 4, 1, 12, 300, 1, 2),
            "3x3 plus": (*FR.standard_matmul(3, K=28), 9, 1, 2, 60, 7, 1),
            "pool": (*FR.pool_list(rng, 5, 20, 20, 3, 2), 5, 2, 4, 80, 0, 1),
            "pool plus": (*FR.pool_list(rng, 3, 13, 12, 4, 1), 3, 1, 6, 80, 3, 2)}


def _walk(tokens, L, S, shift, W, n, plus_after, plus_slack, seed):
    total = F2.target_of(tokens, L, S, shift) & 1
    st, status = F2.begin(tokens[None], [L], np.zeros(W, dtype=np.int64), shift)
    assert status == 0
    K = tokens.shape[0]
    for w in range(W):                                                                # begin keeps the XOR too
        assert np.array_equal(F2.xor_sum(F2.from_rows(st["cur"][w], st["cur_rank"][w]), S), total)
    trace, events, seen = [], Counter(), Counter()

    def on_step(w, t, terms):
        assert np.array_equal(F2.xor_sum(terms, S), total)                            # the XOR of all terms never changes
        assert len(terms) <= K and all(all(0 < m < 2 ** S for m in term) for term in terms)
        assert not any(sum(a[d] == b[d] for d in range(3)) >= 2 for i, a in enumerate(terms) for b in terms[i + 1:])
        seen[w] += 1

    for step0 in (0, n, 2 * n):                                                       # three launches
        F2.advance(st, seed, 10, step0, n, plus_after, plus_slack, trace=trace, on_step=on_step, events=events)
    for w in range(W):
        assert np.array_equal(F2.xor_sum(F2.from_rows(st["best"][w], st["best_rank"][w]), S), total)
        assert not st["cur"][w, st["cur_rank"][w]:].any() and not st["best"][w, st["best_rank"][w]:].any()
        assert st["best_rank"][w] <= st["cur_rank"][w]
        assert st["flips"][w] == sum(1 for ww, _, kind, _ in trace if ww == w and kind == "flip")
        assert st["pluses"][w] == sum(1 for ww, _, kind, _ in trace if ww == w and kind == "plus")
        assert seen[w] == st["flips"][w] + st["pluses"][w]
    assert len({(w, t) for w, t, _, _ in trace}) == len(trace) and trace              # one action per step of a walking walk
    res = F2.residual(np.repeat(total[None].astype(np.int8), W, 0), st["best"], st["best_rank"])
    assert not res.any()
    return st, trace, events


_TRACES = {}


def traces(name):
    if name not in _TRACES:
        _TRACES[name] = _walk(*_cases()[name], SEED + 3)
    return _TRACES[name]


@pytest.mark.parametrize("name", list(_cases()))
def test_every_step_keeps_the_xor_of_the_terms(name):
    st, trace, events = traces(name)
    print(name, dict(events), Counter(kind for _, _, kind, _ in trace))
    assert (st["pluses"].sum() > 0) == (_cases()[name][6] > 0)


def test_the_traces_hold_every_kind_of_step():
    """Flips of all four variants, plus steps of all twelve, merges, cancelling pairs (both terms removed), a plus that
    leaves a null term, and a stuck walk: what the XOR invariant above was checked over."""
    flips, pluses, events, stuck = set(), set(), Counter(), 0
    for name in _cases():
        st, trace, ev = traces(name)
        flips |= {v for _, _, kind, v in trace if kind == "flip"}
        pluses |= {v for _, _, kind, v in trace if kind == "plus"}
        events += ev
        stuck += int((st["state"] == 1).sum())
    assert flips == set(range(4)) and pluses == set(range(12))
    assert events["merge"] > 0 and events["cancel"] > 0 and stuck > 0
    assert events["plus_null1"] + events["plus_null2"] + events["plus_null3"] > 0


def test_walks_from_the_standard_2x2_algorithm_reach_rank_7_and_are_then_stuck():
    tokens, L = FR.standard_matmul(2)
    total = F2.target_of(tokens, L, 4, 1) & 1
    st, status = F2.begin(tokens[None], [L], np.zeros(16, dtype=np.int64), 1)
    assert status == 0 and (st["cur_rank"] == 8).all()                 # nothing merges in the standard algorithm
    F2.advance(st, SEED, 0, 0, STEPS_TO_7)
    won = st["best_rank"] == 7
    assert won.sum() >= 1, "no walk reached rank 7: the rules were restated wrongly"
    assert (st["best_rank"] >= 7).all() and np.array_equal(np.flatnonzero(~won), [4, 6, 11])
    for w in np.flatnonzero(won):                                      # a Strassen-type list: no flip is left
        assert st["state"][w] == 1 and st["cur_rank"][w] == 7 and 0 < st["best_step"][w] <= STEPS_TO_7
        assert F2.matches(F2.from_rows(st["cur"][w], 7)) == []
        assert np.array_equal(F2.xor_sum(F2.from_rows(st["best"][w], 7), 4), total)
    assert (st["state"][~won] == 0).all() and (st["best_step"][~won] == 0).all()
    assert (st["flips"][~won] == STEPS_TO_7).all()                     # no flip is ever refused
    before = F2.copy_state(st)
    F2.advance(st, SEED, 0, STEPS_TO_7, 50)                            # a stuck walk stays as it is
    for k in F2.STATE_NAMES:
        assert np.array_equal(st[k][won], before[k][won]), k


def test_begin_restated_takes_parities_drops_and_reduces():
    S, K, shift = 3, 8, 2
    u, v, w = np.array([1, 0, -1]), np.array([0, 1, 1]), np.array([1, -3, 0])          # parities 101, 011, 110
    e0, e2, z, two = np.array([1, 0, 0]), np.array([0, 0, 1]), np.zeros(3, dtype=np.int64), np.array([2, 0, -2])
    rows = np.stack([np.concatenate(r) for r in (
        (u, two, w),                     # null mod 2
        (-u, v, e0), (u, -v, -e2),       # share (u, v) mod 2: merge to u v (e0 ^ e2)
        (e0, e2, w), (e0, e2, -w),       # cancel: both removed
        (e2, e0, w), (e2, z, w),         # the second is null
    )])
    tokens = np.zeros((1, K, 9), dtype=np.int8)
    tokens[0, :7] = rows + shift
    tokens[0, 7] = 99                                                  # behind the length: not read
    st, status = F2.begin(tokens, [7], None, shift)
    assert status == 0 and st["cur_rank"][0] == 2 and st["state"][0] == 0
    assert F2.from_rows(st["cur"][0], 2) == [[0b101, 0b110, 0b101], [0b100, 0b001, 0b011]]
    assert np.array_equal(F2.xor_sum(F2.from_rows(st["cur"][0], 2), S), F2.target_of(tokens[0], 7, S, shift) & 1)
    for lengths, src, bit in (([9], None, F2.BAD_LENGTH), ([-1], None, F2.BAD_LENGTH), ([7], [0, 1, -1], F2.BAD_SRC)):
        st3, status3 = F2.begin(tokens, lengths, src, shift)
        assert status3 == bit and (st3["state"] == -1).sum() == (2 if src else 1) and not st3["cur"][st3["state"] == -1].any()


def test_plus_slack_0_takes_no_plus_and_a_full_list_takes_none():
    tokens, L = FR.standard_matmul(2, K=9)
    a, _ = F2.begin(tokens[None], [L], np.zeros(4, dtype=np.int64), 1)
    b = F2.copy_state(a)
    F2.advance(a, SEED, 0, 0, 300, plus_after=0)
    F2.advance(b, SEED, 0, 0, 300, plus_after=1, plus_slack=0)
    for k in F2.STATE_NAMES:
        assert np.array_equal(a[k], b[k]), k                          # since included: both maintain it
    full, _ = F2.begin(FR.standard_matmul(2)[0][None], [8], np.zeros(4, dtype=np.int64), 1)   # L = K = 8
    F2.advance(full, SEED, 0, 0, 100, plus_after=1, plus_slack=4)
    assert not full["pluses"].any() and (full["flips"] == 100).all()


def test_residual_restated_counts_the_cells_that_differ():
    tokens, L = FR.standard_matmul(2)
    target = F2.target_of(tokens, L, 4, 1)
    st, _ = F2.begin(tokens[None], [L], None, 1)
    lists = np.repeat(st["cur"], 4, 0)
    lists[1, 3, 2] ^= 0b0110                                           # two bits of one m_2: m_0 and m_1 hold one bit each
    ranks = np.array([8, 8, 9, -1], dtype=np.int32)
    assert list(F2.residual(np.repeat(target[None], 4, 0), lists, ranks)) == [0, 2, -1, -1]
