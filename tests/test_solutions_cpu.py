"""CPU checks of the solution archive (include/tensor_game_solutions.h): the host restatement's own algebra -- the
Strassen known answer and its invariance, sum preservation, the edge cases and the bad rows -- the archive's add rule,
and the host side of the library: the header, the exported symbols and the size checks."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import _lib, build, ops

import solutions_ref as SR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_solutions.h"


# ---- the restatement's algebra ---------------------------------------------------------------------------------------
def test_strassen_known_answer_and_200_variants(golden):
    g = golden("strassen")
    S, shift, K = 4, 1, 12
    tokens = np.zeros((1, K, 12), dtype=np.int8)
    tokens[0, :7] = g["tokens"]
    cn, rank, key, res, status = SR.canon(g["tensor"][None], tokens, [7], shift)
    assert (int(res[0]), int(rank[0]), status) == (0, 7, 0)
    assert not cn[0, 7:].any() and int(key[0]) == SR.stream_key(cn[0, :7].tobytes())
    assert np.array_equal(SR.term_sum(cn[0], 7, S, shift), g["tensor"])
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        vt, vl = SR.variant(rng, tokens[0], 7, K, S, shift)
        assert vl == 10
        c2, r2, k2, s2, st2 = SR.canon(g["tensor"][None], vt[None], [vl], shift)
        assert (int(s2[0]), int(r2[0]), st2) == (0, 7, 0)
        assert np.array_equal(c2, cn) and k2[0] == key[0]


@pytest.mark.parametrize("shift", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 4, 5, 9])
def test_canonical_terms_sum_to_the_original_terms(S, shift):
    rng = np.random.default_rng(1000 * S + shift)
    K, M = 12, 26
    tokens, lengths = SR.random_lists(rng, M, K, S, shift, np.arange(M) % (K + 1))   # every length from 0 to K
    cn, rank, key, res, status = SR.canon(None, tokens, lengths, shift)
    assert res is None and status == 0
    merged = 0
    for m in range(M):
        L = int(lengths[m])
        assert 0 <= rank[m] <= L and not cn[m, rank[m]:].any()
        assert np.array_equal(SR.term_sum(cn[m], int(rank[m]), S, shift), SR.term_sum(tokens[m], L, S, shift))
        f = cn[m, :rank[m]].astype(np.int64) - shift
        for x in (0, 1):                           # u and v first non-zero positive; w carries a run's sign
            firsts = [row[x * S:(x + 1) * S][np.flatnonzero(row[x * S:(x + 1) * S])[0]] for row in f]
            assert all(v > 0 for v in firsts)
        merged += int(rank[m] < L)
    assert merged > M // 2                         # the planted duplicates and null terms did something


def _tok(rows, shift, K):
    out = np.zeros((K, rows.shape[1] if len(rows) else 0), dtype=np.int8)
    out[:len(rows)] = (rows + shift).astype(np.int8)
    return out


def test_full_cancellation_and_multiplicity_runs():
    S, shift, K = 2, 1, 6
    term = np.array([1, -1, 0, 1, 1, 1])
    neg = term * np.array([1, 1, -1, -1, 1, 1])              # v negated: minus the term
    target = np.arange(8, dtype=np.int8).reshape(2, 2, 2)    # 7 non-zero entries
    cancel = _tok(np.stack([term, neg]), shift, K)
    cn, rank, key, res, status = SR.canon(target[None], cancel[None], [2], shift)
    assert (int(rank[0]), int(key[0]), int(res[0]), status) == (0, SR.stream_key(b""), 7, 0) and not cn.any()
    assert SR.stream_key(b"") == 0
    runs = _tok(np.stack([term, term, neg, term]), shift, K)  # three times the term and its negative once
    cn, rank, key, res, status = SR.canon(None, runs[None], [4], shift)
    assert int(rank[0]) == 2 and np.array_equal(cn[0, 0], cn[0, 1]) and not cn[0, 2:].any()
    assert np.array_equal(SR.term_sum(cn[0], 2, S, shift), 2 * SR.term_sum(runs, 1, S, shift))
    minus = _tok(np.stack([neg, term, neg, neg]), shift, K)   # net minus two: w carries the sign
    c2, r2, _, _, _ = SR.canon(None, minus[None], [4], shift)
    assert int(r2[0]) == 2 and np.array_equal(c2[0, :2, :4], cn[0, :2, :4])
    assert np.array_equal(c2[0, :2, 4:].astype(int) - shift, -(cn[0, :2, 4:].astype(int) - shift))


def test_bad_rows_leave_their_neighbours_alone():
    rng = np.random.default_rng(7)
    S, K = 2, 5
    tokens, lengths = SR.random_lists(rng, 5, K, S, 0, [3, 0, 4, 0, 2])
    lengths[[1, 3]] = -1, K + 1
    targets = SR.targets_for(rng, tokens, np.clip(lengths, 0, K), S, 0)
    good = SR.canon(targets[[0, 2, 4]], tokens[[0, 2, 4]], lengths[[0, 2, 4]], 0)
    cn, rank, key, res, status = SR.canon(targets, tokens, lengths, 0)
    assert status == SR.BAD_LENGTH
    for m in (1, 3):
        assert (int(rank[m]), int(key[m]), int(res[m])) == (0, 0, -1) and not cn[m].any()
    for got, want in zip((cn, rank, key, res), good[:4]):
        assert np.array_equal(got[[0, 2, 4]], want)
    # a negation that leaves int8: shift 0, u = (-128, 1) has its first non-zero negative and 128 is no token
    tokens[2, 0] = [-128, 1, 1, 0, 1, 0]
    cn, rank, key, res, status = SR.canon(targets, tokens, lengths, 0)
    assert status == SR.BAD_LENGTH | SR.BAD_NEGATION
    assert (int(rank[2]), int(key[2]), int(res[2])) == (0, 0, -1) and not cn[2].any()
    for got, want in zip((cn, rank, key, res), good[:4]):
        assert np.array_equal(got[[0, 4]], want[[0, 2]])
    # the same vector inside a null term is dropped before any negation
    tokens[2, 0] = [-128, 1, 0, 0, 1, 0]
    assert SR.canon(targets, tokens, lengths, 0)[4] == SR.BAD_LENGTH
    # a run with a negative sum negates w: w = (1, -128) is normalised, its negative is no token
    t = np.zeros((1, 2, 6), dtype=np.int8)
    t[0, 0] = [-1, 0, 1, 0, 1, -128]
    assert SR.canon(None, t, [1], 0)[4] == SR.BAD_NEGATION


def test_archive_restatement():
    rng = np.random.default_rng(11)
    S, K, shift = 3, 6, 1
    tokens, lengths = SR.random_lists(rng, 12, K, S, shift, rng.integers(1, K + 1, size=12))
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    vt, vl = SR.variant(rng, tokens[0], min(int(lengths[0]), 3), K, S, shift)   # row 3 := row 0 written differently
    tokens[0, int(lengths[0]):] = 0
    lengths[0] = min(int(lengths[0]), 3)
    tokens[3], lengths[3] = vt, vl
    targets[0] = targets[3] = SR.term_sum(tokens[0], int(lengths[0]), S, shift).astype(np.int8)
    a = SR.Archive(S, max_rank=K, capacity=64, shift=shift)
    proven, rank, key, fresh = a.add(targets, tokens, lengths)
    assert key[0] == key[3] and proven[0] and proven[3] and fresh[0] and not fresh[3]   # intra-batch duplicate
    assert not fresh[~proven].any() and a.count == int(fresh.sum()) > 0
    assert a.lowest_rank == min(int(r) for r, f in zip(rank, fresh) if f)
    assert not a.add(targets, tokens, lengths)[3].any() and a.status == 0               # nothing new the second time
    for tk, r, tkey in zip(a.tokens, a.rank, a.target_key):                             # an entry sums to its target
        assert any(SR.state_key(t) == tkey and np.array_equal(SR.term_sum(tk, r, S, shift), t) for t in targets)
    # the capacity cut
    n_new = a.count
    assert n_new >= 3
    b = SR.Archive(S, max_rank=K, capacity=2, shift=shift)
    fresh_b = b.add(targets, tokens, lengths)[3]
    assert b.count == 2 and b.status == 1 and int(fresh_b.sum()) == 2
    assert np.array_equal(np.flatnonzero(fresh_b), np.flatnonzero(fresh)[:2])
    # a round trip answers as the original
    c = SR.Archive.from_state_dict(b.state_dict())
    for arch in (b, c):
        assert not arch.add(targets, tokens, lengths)[3].any() and arch.count == 2
    # rank above max_rank is not stored
    d = SR.Archive(S, max_rank=1, capacity=64, shift=shift)
    pr, rk, _, fr = d.add(targets, tokens, lengths)
    assert not fr[rk > 1].any() and all(r <= 1 for r in d.rank)


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_solutions_header_is_plain_c_and_states_the_semantics():
    text = HDR.read_text()
    for words in ("cannot wrap", "ORIGINAL", "rescalings", "symmetries of the target", "fmix64", "before it addresses"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_solution_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_solution_canon", "tg_solution_check"] == sorted(_lib.SOLUTION_SIGNATURES)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert (_lib.TG_SOL_MAX_K, _lib.TG_SOL_BAD_LENGTH, _lib.TG_SOL_BAD_NEGATION) == (256, SR.BAD_LENGTH, SR.BAD_NEGATION)
    assert "solution_canon" in ops.__all__ and "solution_check" in ops.__all__
    assert "SolutionArchive" in mat_mul_amd.__all__ and mat_mul_amd.solutions.SolutionArchive is mat_mul_amd.SolutionArchive


@pytest.mark.parametrize("args, words", [
    ((8, 8, 0, 1), "S=0"), ((8, 8, 33, 1), "S=33"), ((8, 0, 4, 1), "K=0"), ((8, 257, 4, 1), "K=257"),
    ((8, 8, 4, -1), "shift=-1"), ((8, 8, 4, 65), "shift=65"), ((-1, 8, 4, 1), "M=-1"),
])
def test_solution_check_refuses_each_bound(args, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.solution_check(*args)


def test_solution_canon_refuses_before_any_launch():
    ops.solution_check(0, 256, 32, 64)
    ops.solution_check(4096, 1, 1, 0)
    canon = _lib.lib.tg_solution_canon
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    ok = dict(targets=p(1), tokens=p(4099), lengths=p(8192), M=4, K=8, S=4, shift=1, canon=p(16387), rank=p(32768),
              key=p(65536), res=p(131072), status=None)
    order = ("targets", "tokens", "lengths", "M", "K", "S", "shift", "canon", "rank", "key", "res", "status")
    for over, words in ((dict(tokens=None), b"null tokens"), (dict(lengths=None), b"null lengths"),
                        (dict(canon=None), b"null canon"), (dict(rank=None), b"null rank"), (dict(key=None), b"null key"),
                        (dict(targets=None), b"residual_nnz needs targets"), (dict(key=p(65540)), b"key not 8-byte"),
                        (dict(canon=p(4099)), b"in-place"), (dict(K=257), b"K=257"), (dict(S=33), b"S=33"),
                        (dict(shift=65), b"shift=65"), (dict(M=-1), b"M=-1")):
        kw = {**ok, **over}
        assert canon(*[kw[k] for k in order], None) == -1 and words in _lib.lib.tg_last_error(), over
    assert canon(None, None, None, 0, 8, 4, 1, None, None, None, None, None, None) == 0   # M = 0 returns at once


def test_ops_and_archive_refuse_cpu_tensors():
    tok = torch.zeros((3, 4, 12), dtype=torch.int8)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.solution_canon(None, tok, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.SolutionArchive(S=4, max_rank=16, capacity=64, device="cpu")
