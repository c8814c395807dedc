"""CPU checks of the plus transitions (include/tensor_game_flips_plus.h): the header, the exported symbols, every refusal
of the host side by name, and the host restatement's own invariants -- every step keeps the exact sum and the bound,
the rank stays under the step's cap, plus_slack = 0 gives the plain walks -- and the table of events, which
test_gpu_flips_plus.py relies on.  The table is flips_plus_ref.CASES (both files run its cases): per case the events the
restatement must show at least MIN_EVENTS times; test_cases_reach_the_events_of_the_table prints every count."""
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
import flips_plus_ref as PR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_flips_plus.h"


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_plus_header_is_plain_c_and_states_the_rule():
    text = HDR.read_text()
    for words in ("cap = min(K, best_rank + plus_slack)", "want = (C == 0) || (since >= plus_after)",
                  "can = (L >= 2) && (L < cap)", "(o.y * P) >> 32", "(o.z * 24) >> 32", "012, 021, 102, 120, 201, 210",
                  "the highest slot", "Steps are consecutive", "plus_slack == 0", "flips does not count a plus"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_plus_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_flip_advance_plus", "tg_flip_plus_check"] == sorted(_lib.FLIP_PLUS_SIGNATURES)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert _lib.TG_FLIP_MAX_PLUS_AFTER == PR.INT32_MAX
    for name in ("flip_plus_check", "flip_advance_plus"):
        assert name in ops.__all__


OK_SIZES = dict(W=4, K=8, S=4, shift=1, bound=1, step0=0, n_steps=16, plus_after=3, plus_slack=1)
REFUSALS = [(dict(K=129), "K=129"), (dict(K=0), "K=0"), (dict(bound=0), "bound=0"), (dict(bound=64), "bound=64"),
            (dict(n_steps=0), "n_steps=0"), (dict(n_steps=65537), "n_steps=65537"),
            (dict(step0=2 ** 32 - 15), "step0 + n_steps"), (dict(step0=-1), "step0=-1"), (dict(S=33), "S=33"),
            (dict(S=0), "S=0"), (dict(shift=65), "shift=65"), (dict(shift=-1), "shift=-1"), (dict(W=-1), "W=-1"),
            (dict(plus_after=0), "plus_after=0"), (dict(plus_after=-5), "plus_after=-5"),
            (dict(plus_after=2 ** 31), "plus_after=2147483648"), (dict(plus_slack=-1), "plus_slack=-1"),
            (dict(plus_slack=129), "plus_slack=129")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_plus_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.flip_plus_check(**{**OK_SIZES, **over})


def test_plus_check_takes_the_limits():
    ops.flip_plus_check(0, 128, 32, 64, 63, 2 ** 32 - 65536, 65536, 2 ** 31 - 1, 128)
    ops.flip_plus_check(1 << 20, 1, 1, 0, 1, 0, 1, 1, 0)


def test_the_entry_refuses_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    names = PR.STATE_NAMES
    state = dict(cur=p(4099), cur_rank=p(8192), best=p(16387), best_rank=p(32768), best_step=p(65536), flips=p(131072),
                 state=p(262144), since=p(524288), pluses=p(1048576))
    ok = dict(**state, W=4, K=8, S=4, shift=1, bound=1, seed=0, walk0=0, step0=0, n_steps=16, plus_after=3, plus_slack=1)
    order = (*names, "W", "K", "S", "shift", "bound", "seed", "walk0", "step0", "n_steps", "plus_after", "plus_slack")
    advance = _lib.lib.tg_flip_advance_plus
    for over, words in [(dict(K=129), b"K=129"), (dict(bound=0), b"bound=0"), (dict(bound=64), b"bound=64"),
                        (dict(S=33), b"S=33"), (dict(shift=65), b"shift=65"), (dict(cur=None), b"null cur"),
                        (dict(best_step=None), b"null best_step"), (dict(best=p(4099)), b"cur == best"),
                        (dict(flips=p(131076)), b"flips not 8-byte"), (dict(state=p(262145)), b"state not 4-byte"),
                        (dict(n_steps=0), b"n_steps=0"), (dict(n_steps=65537), b"n_steps=65537"),
                        (dict(step0=2 ** 32 - 15), b"step0 + n_steps"), (dict(step0=-1), b"step0=-1"),
                        (dict(plus_after=0), b"plus_after=0"), (dict(plus_slack=129), b"plus_slack=129"),
                        (dict(plus_slack=-1), b"plus_slack=-1"), (dict(since=None), b"null since"),
                        (dict(pluses=None), b"null pluses"), (dict(since=p(524290)), b"since not 4-byte"),
                        (dict(pluses=p(1048580)), b"pluses not 8-byte")]:
        kw = {**ok, **over}
        assert advance(*[kw[k] for k in order], None) == -1, over
        msg = _lib.lib.tg_last_error()
        assert words in msg and b"tg_flip_advance_plus" in msg, (over, msg)
    assert advance(*[None] * 9, 0, 8, 4, 1, 1, 0, 0, 0, 16, 3, 1, None) == 0      # W = 0 returns at once


def test_bindings_refuse_cpu_tensors():
    tok = torch.zeros((3, 4, 12), dtype=torch.int8)
    lengths = torch.zeros(3, dtype=torch.int64)
    st = {k: torch.zeros((3, 4, 12) if k in ("cur", "best") else (3,), dtype=torch.int8) for k in PR.STATE_NAMES}
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.flip_advance_plus(st, 4, 2, 1)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FlipWalks.start(tok, lengths, plus_after=5)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.FlipWalks.from_state_dict({"version": 2}, "cpu")
    with pytest.raises(_lib.TensorGameError, match="version 3"):
        mat_mul_amd.FlipWalks.from_state_dict({"version": 3}, "cuda")


# ---- the restatement's invariants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in PR.CASES if n != "inert full"])           # (that one takes no step)
def test_every_step_keeps_the_sum_and_the_bound_and_stays_under_the_cap(name):
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, _ = PR.CASES[name]
    tokens, L, st = PR.start_state(name)
    st = PR.copy_state(st)
    W = min(W, 4)                                                 # (the per-step sum is the slow side)
    st = {k: v[:W] for k, v in st.items()}
    total = FR.term_sum(tokens, L, S, bound)
    seen = Counter()

    def on_step(w, t, terms, cap):
        rows = FR.to_rows(terms, len(terms) + 1, S, 0)
        assert np.abs(rows.astype(int)).max(initial=0) <= bound
        assert np.array_equal(FR.term_sum(rows, len(terms), S, 0), total)
        assert len(terms) <= cap <= K and all(t[3] in (-1, 1) for t in terms)
        seen["steps"] += 1

    half = n_steps // 2                                           # two calls: since and pluses carry
    PR.advance(st, seed, 0, 0, half, bound, bound, plus_after, plus_slack, on_step=on_step)
    PR.advance(st, seed, 0, half, n_steps - half, bound, bound, plus_after, plus_slack, on_step=on_step)
    whole = PR.case_ref(name)[3]
    for k in PR.STATE_NAMES:
        assert np.array_equal(st[k], whole[k][:W]), k             # and equal the one call of case_ref
    assert seen["steps"] == W * n_steps and (st["pluses"] > 0).all()
    for w in range(W):
        assert np.array_equal(FR.term_sum(st["best"][w], st["best_rank"][w], S, bound), total)


@pytest.mark.parametrize("plus_after", [1, 2 ** 31 - 1])
def test_plus_slack_0_is_the_plain_walk(plus_after):
    tokens, L = FR.standard_matmul(2)
    plain, status = FR.begin(tokens[None], [L], np.zeros(16, dtype=np.int64), 1, 1)
    assert status == 0
    st = PR.with_plus(FR.copy_state(plain))
    st["pluses"][:] = 7
    FR.advance(plain, 0, 0, 0, 3000, 1, 1)
    PR.advance(st, 0, 0, 0, 3000, 1, 1, plus_after, 0)
    assert (plain["state"] == 1).sum() == 7                        # stuck walks included
    for k in FR.STATE_NAMES:
        assert np.array_equal(st[k], plain[k]), k
    assert (st["pluses"] == 7).all()


def test_a_huge_plus_after_is_the_plain_walk_while_nothing_gets_stuck():
    tokens, L = FR.standard_matmul(3)
    plain, _ = FR.begin(tokens[None], [L], np.zeros(4, dtype=np.int64), 1, 1)
    st = PR.with_plus(FR.copy_state(plain))
    FR.advance(plain, 5, 0, 0, 200, 1, 1)
    PR.advance(st, 5, 0, 0, 200, 1, 1, 2 ** 31 - 1, 3)
    assert (plain["state"] == 0).all() and not st["pluses"].any()
    for k in FR.STATE_NAMES:
        assert np.array_equal(st[k], plain[k]), k
    assert (st["since"] > 0).all() and (st["since"] <= 200).all()


def test_since_saturates_and_counts_refused_steps():
    tokens, L, st = PR.start_state("inert full")
    st = PR.copy_state(st)
    st["cur_rank"][:] = 1                                          # one term: no match, no pair -- stuck, since kept
    st["since"][:] = PR.INT32_MAX
    PR.advance(st, 0, 0, 0, 2, 2, 2, 1, 1)
    assert (st["state"] == 1).all() and (st["since"] == PR.INT32_MAX).all()
    tokens, L = FR.standard_matmul(2)                              # K = 8 = L: no plus ever; a flip step at INT32_MAX stays there
    st, _ = FR.begin(tokens[None], [L], np.zeros(2, dtype=np.int64), 1, 1)
    st = PR.with_plus(st)
    st["since"][:] = PR.INT32_MAX - 1
    PR.advance(st, 0, 0, 0, 3, 1, 1, 1, 5)
    assert (st["since"] == PR.INT32_MAX).all() and (st["cur_rank"] == 8).all()


# ---- the table of events ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.CASES))
def test_cases_reach_the_events_of_the_table(name):
    kind, S, K, L, bound, W, n_steps, plus_after, plus_slack, seed, must = PR.CASES[name]
    tokens, L, st, want, events = PR.case_ref(name)
    print(name, {k: events[k] for k in PR.PLUS_EVENTS})
    assert (st["cur_rank"] == L).all()                             # begin kept every term
    for e in must:
        assert e in PR.PLUS_EVENTS and events[e] >= PR.MIN_EVENTS, (e, events[e])
    assert events["plus_accepted"] == want["pluses"].sum()
    assert events["plus_accepted"] + events["plus_refused"] == events["plus_forced"] + events["plus_timed"]
    assert (want["cur_rank"] <= K).all()
    if name in ("cap K64", "last K128"):
        assert (want["cur_rank"] == K).all()                       # the very last slot was filled in every walk
    if name == "inert full":
        assert (want["state"] == 1).all() and not want["pluses"].any()
    total = FR.term_sum(tokens, L, S, bound)
    for w in range(W):
        assert np.array_equal(FR.term_sum(want["cur"][w], want["cur_rank"][w], S, bound), total)
        assert np.array_equal(FR.term_sum(want["best"][w], want["best_rank"][w], S, bound), total)


def test_the_cases_together_reach_every_event():
    reached = {e for case in PR.CASES.values() for e in case[10]}
    assert reached == set(PR.PLUS_EVENTS), set(PR.PLUS_EVENTS) - reached
    assert not set(PR.PLUS_EVENTS) & set(FR.EVENTS)


def test_stuck_walks_of_the_plain_entry_move_on():
    """From the standard <2,2,2> list the plain walks that reach 7 terms are stuck for good; with plus transitions the
    same walks take forced pluses there and keep walking."""
    tokens, L = FR.standard_matmul(2, K=9)
    plain, _ = FR.begin(tokens[None], [L], np.zeros(16, dtype=np.int64), 1, 1)
    st = PR.with_plus(FR.copy_state(plain))
    FR.advance(plain, 0, 0, 0, 3000, 1, 1)
    events = Counter()
    PR.advance(st, 0, 0, 0, 3000, 1, 1, 10 ** 6, 2, events=events)   # never timed: a plus only where C == 0
    stuck = plain["state"] == 1
    assert stuck.sum() == 7 and (st["state"] == 0).all()
    assert (st["pluses"][stuck] > 0).all() and not st["pluses"][~stuck].any() and events["plus_timed"] == 0
    assert np.array_equal(st["best_rank"], plain["best_rank"]) and np.array_equal(st["best_step"], plain["best_step"])
