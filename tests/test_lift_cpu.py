"""CPU checks of the sign lift (include/tensor_game_lift.h): the header, the exported symbols, the size checks and
refusals of the host side of the library and of the Python layer, and the host restatement's own invariants -- the pivot
rule and the rank against brute force over every assignment, status 0 means an exact sum, and the walks from the standard
<2,2,2> list all lift."""
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

import flips_mod2_ref as F2
import flips_ref as FR
import lift_ref as LR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_lift.h"


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_lift_header_is_plain_c_and_states_the_rules():
    text = HDR.read_text()
    for words in ("before it addresses", "ascending (r, d, e) order", "arithmetic shift", "span of the columns c' < c",
                  "0x4C320000u", "TG_LIFT2_DOMAIN + (f >> 7)", "(f >> 5) & 3", "cannot", "min_t miss_t",
                  "free in its method", "do not depend on ws_lists", "TG_LIFT2_NOT_MOD2", "TG_LIFT2_INCONSISTENT",
                  "TG_LIFT2_NOT_EXACT"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_lift_symbols_are_declared_and_exported():
    syms = sorted(set(re.findall(r"^(?:int|int64_t)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_lift2_check", "tg_lift2_signs", "tg_lift2_workspace_bytes"] == sorted(_lib.LIFT2_SIGNATURES)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert _lib.lib.tg_abi_version() == _lib.TG_ABI_VERSION == 4
    assert _lib.lib.tg_lift2_workspace_bytes.restype is C.c_int64
    text = HDR.read_text()
    assert _lib.TG_LIFT2_DOMAIN == LR.DOMAIN == 0x4C320000
    assert f"TG_LIFT2_MAX_TRIES {_lib.TG_LIFT2_MAX_TRIES}" in text and _lib.TG_LIFT2_MAX_TRIES == LR.MAX_TRIES >= 1024
    assert f"TG_LIFT2_MAX_WS_LISTS {_lib.TG_LIFT2_MAX_WS_LISTS}" in text
    for name, v in (("OK", 0), ("NOT_MOD2", 1), ("INCONSISTENT", 2), ("NOT_EXACT", 3)):
        assert getattr(_lib, "TG_LIFT2_" + name) == getattr(LR, name) == v and f"TG_LIFT2_{name} {v}" in text
    for name in ("lift2_check", "lift2_workspace_bytes", "lift2_signs"):
        assert name in ops.__all__
    for name in ("lift_signs", "LiftResult", "reduce_archive_lifted", "lift"):
        assert name in mat_mul_amd.__all__
    assert mat_mul_amd.lift_signs is mat_mul_amd.lift.lift_signs
    assert mat_mul_amd.reduce_archive_lifted is mat_mul_amd.lift.reduce_archive_lifted
    assert mat_mul_amd.LiftResult is mat_mul_amd.lift.LiftResult
    assert callable(mat_mul_amd.Mod2Walks.lift)


OK_SIZES = dict(W=4, K=8, S=4, shift=1, tries=32, ws_lists=1)
REFUSALS = [(dict(K=129), "K=129"), (dict(K=0), "K=0"), (dict(S=33), "S=33"), (dict(S=0), "S=0"), (dict(shift=65), "shift=65"),
            (dict(shift=-1), "shift=-1"), (dict(W=-1), "W=-1"), (dict(tries=0), "tries=0"), (dict(tries=1025), "tries=1025"),
            (dict(ws_lists=-1), "ws_lists=-1"), (dict(ws_lists=65537), "ws_lists=65537"),
            (dict(K=64, S=16, ws_lists=0), "ws_lists=0")]


@pytest.mark.parametrize("over, words", REFUSALS)
def test_lift2_check_refuses_each_limit_by_name(over, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.lift2_check(**{**OK_SIZES, **over})


def test_lift2_check_takes_the_limits_and_the_workspace_size_is_zero_where_lds_holds_the_system():
    ops.lift2_check(0, 128, 32, 64, 1024, 65536)
    ops.lift2_check(1 << 20, 1, 1, 0, 1, 0)                         # no workspace needed: ws_lists = 0 is taken
    for S in range(1, 10):
        for K in (1, 8, 27, 32):
            assert ops.lift2_workspace_bytes(K, S) == 0, (K, S)      # the least the header promises
    for K, S in ((64, 16), (49, 16), (128, 25), (128, 32), (6, 32)):
        n = ops.lift2_workspace_bytes(K, S)
        words = S ** 3 * ((3 * K * S + 1 + 31) // 32) + 3 * K * S    # the packed system and a pivot per column
        assert n >= 4 * words and n % 256 == 0, (K, S, n)
    for K, S, words in ((0, 4, "K=0"), (129, 4, "K=129"), (8, 0, "S=0"), (8, 33, "S=33")):
        with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
            ops.lift2_workspace_bytes(K, S)


def test_lift_entry_refuses_before_any_launch():
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    signs = _lib.lib.tg_lift2_signs
    ok = dict(targets=p(1), lists=p(4096), ranks=p(8192), W=4, K=8, S=4, shift=1, seed=0, list0=0, tries=32, tokens=p(3),
              status=p(16384), try_used=p(32768), unknowns=p(65536), sys_rank=p(131072), miss=p(262144), workspace=None,
              ws_lists=0)
    order = tuple(ok)
    big = dict(K=64, S=16, ws_lists=2, workspace=p(1 << 20))
    cases = [(dict(K=129), b"K=129"), (dict(S=33), b"S=33"), (dict(shift=65), b"shift=65"), (dict(W=-1), b"W=-1"),
             (dict(tries=0), b"tries=0"), (dict(tries=1025), b"tries=1025"), (dict(ws_lists=-1), b"ws_lists=-1"),
             (dict(targets=None), b"null targets"), (dict(lists=None), b"null lists"), (dict(ranks=None), b"null ranks"),
             (dict(tokens=None), b"null tokens"), (dict(status=None), b"null status"), (dict(try_used=None), b"null try_used"),
             (dict(unknowns=None), b"null unknowns"), (dict(sys_rank=None), b"null sys_rank"), (dict(miss=None), b"null miss"),
             (dict(lists=p(4098)), b"lists not 4-byte"), (dict(ranks=p(8193)), b"ranks not 4-byte"),
             (dict(status=p(16386)), b"status not 4-byte"), (dict(try_used=p(32769)), b"try_used not 4-byte"),
             (dict(unknowns=p(65538)), b"unknowns not 4-byte"), (dict(sys_rank=p(131073)), b"sys_rank not 4-byte"),
             (dict(miss=p(262146)), b"miss not 4-byte"),
             ({**big, "ws_lists": 0}, b"ws_lists=0"), ({**big, "workspace": None}, b"null workspace"),
             ({**big, "workspace": p((1 << 20) + 4)}, b"workspace not 16-byte")]
    for over, words in cases:
        kw = {**ok, **over}
        assert signs(*[kw[k] for k in order], None) == -1 and words in _lib.lib.tg_last_error(), over
    kw = {**ok, "W": 0, **{k: None for k in ("targets", "lists", "ranks", "tokens", "status", "try_used", "unknowns",
                                             "sys_rank", "miss")}}
    assert signs(*[kw[k] for k in order], None) == 0                 # W = 0 returns at once


def test_lift_bindings_refuse_cpu_tensors():
    lists = torch.zeros((3, 4, 3), dtype=torch.int32)
    ranks = torch.zeros(3, dtype=torch.int32)
    targets = torch.zeros((3, 4, 4, 4), dtype=torch.int8)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.lift2_signs(targets, lists, ranks)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.lift_signs(lists, ranks, targets)
    st = {k: torch.zeros((3, 4, 3) if k in ("cur", "best") else (3,), dtype=dt) for k, dt in ops._FLIP2_STATE}
    walks = mat_mul_amd.Mod2Walks(st, torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 4, 0, 0)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        walks.lift(targets)
    with pytest.raises(_lib.TensorGameError, match="'best' or 'cur'"):
        walks.lift(targets, which="other")


# ---- the restatement's own checks ------------------------------------------------------------------------------------
def _span_sets(A):
    """Brute force: span[c] = the set of all sums of the columns below c (cells packed into a Python integer), one
    element per assignment of those columns' unknowns, duplicates merged."""
    cols = [sum(int(v) << i for i, v in enumerate(A[:, c])) for c in range(A.shape[1])]
    spans = [{0}]
    for col in cols:
        spans.append(spans[-1] | {s ^ col for s in spans[-1]})
    return cols, spans


def test_pivots_and_rank_agree_with_brute_force_over_every_assignment():
    rng = np.random.default_rng(11)
    S, K, seen_free, seen_bad, seen_ok = 2, 3, 0, 0, 0
    for trial in range(60):
        R = int(rng.integers(0, K + 1))
        lists = np.zeros((K, 3), dtype=np.int32)
        lists[:R] = rng.integers(0 if trial % 5 == 0 else 1, 2 ** S, size=(R, 3))           # now and then a null term
        X0 = LR.x0_of(lists, R, S)
        signs = rng.choice([-1, 1], size=X0.shape)
        target = LR.term_sum(X0 * signs) if trial % 3 else LR.term_sum(X0) + 2 * rng.integers(0, 2, size=(S, S, S))
        detail = {}
        tok, status, used, N, P, miss = LR.lift_one(target, lists, R, S, 1, 5, trial, 8, detail)
        assert status in (LR.OK, LR.INCONSISTENT, LR.NOT_EXACT) and N == int(X0.sum()) <= 18
        cols, spans = _span_sets(detail["A"])
        assert detail["pivots"] == [c for c in range(N) if cols[c] not in spans[c]]          # the header's rule
        assert P == len(detail["pivots"]) and 2 ** P == len(spans[N])                        # the rank is the image's size
        b = sum(int(v) << i for i, v in enumerate(detail["b"]))
        assert (status == LR.INCONSISTENT) == (b not in spans[N])
        seen_free += N > P
        seen_bad += status == LR.INCONSISTENT
        if status == LR.OK:
            seen_ok += 1
            assert np.array_equal(LR.tokens_sum(tok, R, S, 1), target) and miss == 0 and detail["misses"][used] == 0
            assert all(m > 0 for m in detail["misses"][:used])
        elif status == LR.NOT_EXACT:
            assert miss == min(detail["misses"]) > 0 and not tok.any()
    assert seen_free > 10 and seen_bad > 3 and seen_ok > 10


def test_free_bits_follow_the_header():
    from oracle import tensor_game as O
    seed, g, t = 0x123456789ABCDEF, (7 << 32) | 9, 3
    bits = LR.free_bits(seed, g, t, 300)
    assert not LR.free_bits(seed, g, 0, 300).any()
    for f in (0, 31, 32, 127, 128, 299):
        ctr = np.array([[9, 7, t, 0x4C320000 + (f >> 7)]], dtype=np.uint32)
        key = np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint32)
        o = O.philox4x32_10(ctr, key)[0]
        assert bits[f] == (int(o[(f >> 5) & 3]) >> (f & 31)) & 1, f


def _walked_2x2():
    """The S = 4 family: 8 walks of the restatement from the standard <2,2,2> list, 2 000 steps, seed 0."""
    tokens, L = FR.standard_matmul(2)
    st, status = F2.begin(tokens[None], [L], np.zeros(8, dtype=np.int64), 1)
    assert status == 0
    F2.advance(st, 0, 0, 0, 2000)
    return F2.target_of(tokens, L, 4, 1), st


def test_every_walk_from_the_standard_2x2_list_lifts_and_planted_errors_are_told_apart():
    target, st = _walked_2x2()
    assert list(st["best_rank"]) == [7, 7, 7, 7, 8, 7, 8, 7]
    targets = np.repeat(target[None], 8, 0)
    out = LR.lift(targets, st["best"], st["best_rank"], 4, tries=4)
    assert (out["status"] == 0).all() and (out["try_used"] == 0).all() and (out["miss"] == 0).all()
    for w in range(8):
        R = int(st["best_rank"][w])
        assert np.array_equal(LR.tokens_sum(out["tokens"][w], R, 4, 1), target)
        assert set(np.unique(out["tokens"][w, :R])) <= {0, 1, 2} and not out["tokens"][w, R:].any()
        assert np.array_equal(LR.masks_of_tokens(out["tokens"][w], R, 4, 1), st["best"][w])   # the support is kept
    planted = np.repeat(target[None], 4, 0).astype(np.int64)
    planted[0, 1, 2, 3] += 1                                         # A: wrong mod 2
    planted[1, 1, 2, 3] += 4                                         # B: right mod 4, never exact
    ranks = np.array([7, 7, -1, 9], dtype=np.int32)
    out = LR.lift(planted, np.repeat(st["best"][:1], 4, 0), ranks, 4, tries=4)
    assert list(out["status"]) == [1, 3, -1, -1] and list(out["miss"][:2]) == [1, out["miss"][1]] and out["miss"][1] >= 1
    assert list(out["try_used"]) == [-1] * 4 and not out["tokens"].any()
    zero = np.zeros((3, 4, 4, 4), dtype=np.int64)
    zero[1, 0, 0, 0], zero[2, 0, 0, 0] = 4, 2                        # E, F, G: R = 0
    out = LR.lift(zero, np.zeros((3, 8, 3), dtype=np.int32), np.zeros(3, dtype=np.int32), 4, tries=2)
    assert list(out["status"]) == [0, 3, 2] and list(out["unknowns"]) == [0, 0, 0] and list(out["miss"]) == [0, 1, -1]


def test_kron_of_two_matmul_lists_is_a_matmul_list():
    t2, L2 = FR.standard_matmul(2)
    t4, L4 = FR.standard_matmul(4)
    kron = LR.kron_lists(t2, L2, 2, t2, L2, 2, 1)
    assert kron.shape == (64, 48)
    assert np.array_equal(LR.tokens_sum(kron, 64, 16, 1), LR.tokens_sum(t4, L4, 16, 1))
