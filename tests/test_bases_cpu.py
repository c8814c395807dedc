"""CPU checks of the way back from a changed basis (include/tensor_game_bases.h): the host restatement against the
oracle's own inverse and factor transform, the round trip on tokens, the input conditions the GPU tests rely on, and the
host side of the library: the header, the exported symbols, the size checks and the wrappers' refusals."""
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
from oracle import tensor_game as O

import bases_ref as BR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_bases.h"
SIZES = [1, 2, 4, 9, 16, 25, 32]


def oracle_bases(N, S, seed=3):
    p = min(0.15, 0.4 / S)
    return O.sample_basis(N, S, O.categorical_thresholds((p, 1 - 2 * p, p)), (-1, 0, 1), seed)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_inverse_restatement_equals_the_oracle_and_inverts(S):
    rng = np.random.default_rng(S)
    dense = BR.random_factors(rng, 3, S, (0.2, 0.6, 0.2) if S <= 9 else None)
    P, L, U = oracle_bases(3, S)
    for lower, upper in (dense, (L, U)):
        inv, bad, status = BR.basis_inverse(lower, upper)
        assert status == 0 and not bad.any()
        assert np.array_equal(inv, O.unimodular_inverse(lower, upper))
        prod = lower.astype(np.int64) @ upper.astype(np.int64) @ inv.astype(np.int64)
        assert np.array_equal(prod, np.broadcast_to(np.eye(S, dtype=np.int64), prod.shape))
    assert np.array_equal(L.astype(np.int64) @ U.astype(np.int64), P)


def test_inverse_restatement_bad_rules():
    rng = np.random.default_rng(5)
    S = 32
    lower, upper = BR.random_factors(rng, 5, S)
    good = BR.basis_inverse(lower, upper)[0]
    lower[1, 2, 7, 7] = 0                                       # a diagonal entry 0
    upper[3, 0, 0, 0] = 2                                       # and one 2
    lower[0, 1][np.triu_indices(S, 1)] = 99                     # junk in the triangle that is not read
    inv, bad, status = BR.basis_inverse(lower, upper)
    assert status == BR.BASIS_BAD_DIAGONAL and bad.tolist() == [0, 1, 0, 1, 0]
    assert not inv[1].any() and not inv[3].any() and np.array_equal(inv[[0, 2, 4]], good[[0, 2, 4]])
    lower[2, 0][np.tril_indices(S, -1)] = 127                   # entries of L^-1 grow like 128^k
    inv, bad, status = BR.basis_inverse(lower, upper)
    assert status == BR.BASIS_BAD_DIAGONAL | BR.BASIS_BAD_RANGE and bad.tolist() == [0, 1, 1, 1, 0]
    assert not inv[2].any() and np.array_equal(inv[[0, 4]], good[[0, 4]])
    # the bound itself: a subdiagonal of -128 gives X[r][0] = 128^r, which reaches 2^28 exactly at r = 4
    X = BR.inv_lower(np.eye(5, dtype=np.int64) - 128 * np.eye(5, k=-1, dtype=np.int64))
    assert X[3, 0] == 128 ** 3 < BR.LIMIT == X[4, 0]


@pytest.mark.parametrize("S", [1, 2, 4, 9, 16])
def test_rebase_restatement_equals_transform_factors_and_round_trips(S):
    rng = np.random.default_rng(10 + S)
    M, K, shift = 4, 5, 1
    P, L, U = oracle_bases(M, S)
    tokens, lengths = BR.random_lists(rng, M, K, S, shift, [K, 0, 3, K])
    moved, len2, bad, status = BR.solution_rebase(tokens, lengths, P, None, shift)
    assert status == 0 and not bad.any() and np.array_equal(len2, lengths)
    factors = (tokens.astype(np.int64) - shift).reshape(M, K, 3, S)
    want = O.transform_factors(factors, P).reshape(M, K, 3 * S) + shift
    for m in range(M):
        assert np.array_equal(moved[m, :lengths[m]], want[m, :lengths[m]]) and not moved[m, lengths[m]:].any()
    # basis followed by inverse is the identity on tokens (the rows behind a list come back as zero bytes)
    inv = BR.basis_inverse(L, U)[0]
    back, len3, bad, status = BR.solution_rebase(moved, len2, inv, np.arange(M), shift)
    assert status == 0 and np.array_equal(len3, lengths)
    for m in range(M):
        assert np.array_equal(back[m, :lengths[m]], tokens[m, :lengths[m]]) and not back[m, lengths[m]:].any()


def test_rebase_restatement_bad_rules():
    S, K, shift = 2, 3, 1
    rng = np.random.default_rng(3)
    tokens, lengths = BR.random_lists(rng, 6, K, S, shift, [2, -1, K + 1, 1, 1, 3])
    mats = np.broadcast_to(np.eye(S, dtype=np.int32), (2, 3, S, S)).copy()
    mats[1, 0, 0, 1] = 100
    tokens[5, 0, :S] = np.array([0, 2]) + shift                  # 100 * 2 leaves int8
    tokens[0, 2, :S] = np.array([0, 2]) + shift                  # the same behind the list's end: not read
    tokens[0, :2, 1] = shift                                     # (and nothing of it inside the list)
    index = np.array([1, 0, 0, -1, 2, 1])
    out, lens, bad, status = BR.solution_rebase(tokens, lengths, mats, index, shift)
    assert status == 7 and bad.tolist() == [0, 1, 1, 1, 1, 1] and lens.tolist() == [2, 0, 0, 0, 0, 0]
    assert not out[1:].any() and not out[0, 2:].any() and out[0, :2].any()
    assert BR.rebase_row(tokens[5], 3, mats, 1, shift)[2] == BR.REBASE_BAD_RANGE
    assert BR.rebase_row(tokens[5], 4, mats, 2, shift)[2] == BR.REBASE_BAD_LENGTH | BR.REBASE_BAD_INDEX


@pytest.mark.parametrize("S", [2, 4, 9, 16, 25, 32])
def test_sampled_bases_keep_the_way_back_inside_int8(S):
    """The input conditions of the GPU tests: 256 default bases of seed 3 have small inverses, factors from {-2..2}
    come back far inside int8, and the matmul tensors do not overflow under them."""
    P, L, U = oracle_bases(256, S)
    inv = O.unimodular_inverse(L, U)
    assert np.abs(inv).max() <= 4
    # |A^-1 f| <= 2 * the largest absolute row sum for ANY f from {-2..2}; with the shifts the tests use (<= 2) a token
    assert (2 * np.abs(inv).sum(axis=-1)).max() + 2 <= 127      # that comes back cannot leave int8
    n = {4: 2, 9: 3, 16: 4, 25: 5}.get(S)
    if n:
        T = np.zeros((S, S, S), dtype=np.int8)
        for i in range(n):
            for j in range(n):
                for k in range(n):
                    T[i * n + j, j * n + k, k * n + i] = 1
        moved, overflow = O.change_basis_i8(np.broadcast_to(T, (256, S, S, S)), P)
        assert not overflow.any() and np.abs(moved.astype(np.int64)).max() <= 8


# ---- header and bindings -----------------------------------------------------------------------------------------------
def test_bases_header_is_plain_c_and_states_the_derivation():
    text = HDR.read_text()
    for words in ("NOT READ", "2^28", "2^40", "2^61", "cannot wrap", "2^44", "before they address", "never wraps"):
        assert words in text, words
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_bases_symbols_are_declared_registered_and_exported():
    decls = dict(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", HDR.read_text(), flags=re.M | re.S))
    assert sorted(decls) == ["tg_basis_inverse_check", "tg_basis_inverse_i32", "tg_solution_rebase",
                             "tg_solution_rebase_check"] == sorted(_lib.BASES_SIGNATURES)
    for name, params in decls.items():                          # matching arity, pointers where the header has them
        params = [p.strip() for p in params.split(",")]
        sig = _lib.BASES_SIGNATURES[name]
        assert len(sig) == len(params), name
        for p, ty in zip(params, sig):
            want = C.c_void_p if "*" in p or p.startswith("tg_stream_t") else C.c_int64 if p.startswith("int64_t") else C.c_int
            assert ty is want, (name, p)
        assert getattr(_lib.lib, name).argtypes == sig
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "BASES_SIGNATURES"]
    assert not any(set(decls) & set(o) for o in others)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in decls:
            assert hasattr(lib, s), (path, s)
    assert (_lib.TG_BASIS_BAD_DIAGONAL, _lib.TG_BASIS_BAD_RANGE) == (BR.BASIS_BAD_DIAGONAL, BR.BASIS_BAD_RANGE)
    assert (_lib.TG_REBASE_BAD_LENGTH, _lib.TG_REBASE_BAD_INDEX, _lib.TG_REBASE_BAD_RANGE) == \
        (BR.REBASE_BAD_LENGTH, BR.REBASE_BAD_INDEX, BR.REBASE_BAD_RANGE)
    for name in ("basis_inverse", "solution_rebase", "basis_inverse_check", "solution_rebase_check"):
        assert name in ops.__all__
    assert _lib.lib.tg_abi_version() == 4
    assert "BasisSet" in mat_mul_amd.__all__ and mat_mul_amd.bases.BasisSet is mat_mul_amd.BasisSet
    assert mat_mul_amd.bases.solve_in_bases is mat_mul_amd.solve_in_bases


@pytest.mark.parametrize("args, words", [((8, 0), "S=0"), ((8, 33), "S=33"), ((-1, 4), "N=-1")])
def test_basis_inverse_check_refuses_each_bound(args, words):
    ops.basis_inverse_check(0, 32)
    ops.basis_inverse_check(1 << 20, 1)
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.basis_inverse_check(*args)


@pytest.mark.parametrize("args, words", [
    ((8, 8, 0, 8, 1), "S=0"), ((8, 8, 33, 8, 1), "S=33"), ((8, 0, 4, 8, 1), "K=0"), ((8, 257, 4, 8, 1), "K=257"),
    ((8, 8, 4, 8, -1), "shift=-1"), ((8, 8, 4, 8, 65), "shift=65"), ((-1, 8, 4, 8, 1), "M=-1"),
    ((8, 8, 4, 0, 1), "G=0"), ((8, 8, 4, -1, 1), "G=-1"), ((0, 8, 4, -1, 1), "G=-1"),
])
def test_solution_rebase_check_refuses_each_bound(args, words):
    ops.solution_rebase_check(0, 256, 32, 0, 64)                 # M = 0 needs no triple
    ops.solution_rebase_check(4096, 1, 1, 1, 0)
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.solution_rebase_check(*args)


def test_entries_refuse_before_any_launch():
    p = lambda x: C.c_void_p(x)  # noqa: E731  (never dereferenced: validation fails first)
    inverse = _lib.lib.tg_basis_inverse_i32
    ok = dict(lower=p(1), upper=p(4099), N=4, S=4, inv=p(8192), bad=p(3), status=None)
    order = ("lower", "upper", "N", "S", "inv", "bad", "status")
    for over, words in ((dict(lower=None), b"null lower"), (dict(upper=None), b"null upper"), (dict(inv=None), b"null inv_out"),
                        (dict(inv=p(8194)), b"inv_out not 4-byte"), (dict(status=p(6)), b"status not 4-byte"),
                        (dict(S=33), b"S=33"), (dict(N=-1), b"N=-1")):
        kw = {**ok, **over}
        assert inverse(*[kw[k] for k in order], None) == -1 and words in _lib.lib.tg_last_error(), over
    assert inverse(None, None, 0, 4, None, None, None, None) == 0             # N = 0 returns at once
    rebase = _lib.lib.tg_solution_rebase
    ok = dict(tokens=p(4099), lengths=p(8192), mats=p(16384), index=p(32768), M=4, K=8, S=4, G=2, shift=1, out=p(65537),
              lengths_out=p(131072), bad=p(5), status=None)
    order = ("tokens", "lengths", "mats", "index", "M", "K", "S", "G", "shift", "out", "lengths_out", "bad", "status")
    for over, words in ((dict(tokens=None), b"null tokens"), (dict(lengths=None), b"null lengths"),
                        (dict(mats=None), b"null mats"), (dict(out=None), b"null tokens_out"),
                        (dict(lengths_out=None), b"null lengths_out"), (dict(index=None), b"needs G == M"),
                        (dict(out=p(4099)), b"in-place"), (dict(lengths=p(8196)), b"lengths not 8-byte"),
                        (dict(index=p(32772)), b"index not 8-byte"), (dict(lengths_out=p(131076)), b"lengths_out not 8-byte"),
                        (dict(mats=p(16386)), b"mats not 4-byte"), (dict(status=p(6)), b"status not 4-byte"),
                        (dict(K=257), b"K=257"), (dict(S=33), b"S=33"), (dict(shift=65), b"shift=65"), (dict(M=-1), b"M=-1"),
                        (dict(G=0), b"G=0")):
        kw = {**ok, **over}
        assert rebase(*[kw[k] for k in order], None) == -1 and words in _lib.lib.tg_last_error(), over
    assert rebase(None, None, None, None, 0, 8, 4, 0, 1, None, None, None, None, None) == 0   # M = 0 returns at once


def test_ops_wrappers_refuse_dtype_shape_and_device():
    i8 = lambda *s: torch.zeros(s, dtype=torch.int8)  # noqa: E731
    with pytest.raises(_lib.TensorGameError, match="lower must be int8"):
        ops.basis_inverse(torch.zeros((2, 3, 4, 4), dtype=torch.int32), i8(2, 3, 4, 4))
    with pytest.raises(_lib.TensorGameError, match="upper must be int8"):
        ops.basis_inverse(i8(2, 3, 4, 4), i8(2, 3, 4, 5))
    with pytest.raises(_lib.TensorGameError, match="upper must have the shape"):
        ops.basis_inverse(i8(2, 3, 4, 4), i8(3, 3, 4, 4))
    with pytest.raises(_lib.TensorGameError, match="lower must live on a ROCm device.*no CPU path"):
        ops.basis_inverse(i8(2, 3, 4, 4), i8(2, 3, 4, 4))
    tok, lens = i8(3, 5, 12), torch.zeros(3, dtype=torch.int64)
    mats = torch.zeros((3, 3, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.TensorGameError, match="tokens must be int8"):
        ops.solution_rebase(tok.to(torch.int32), lens, mats)
    with pytest.raises(_lib.TensorGameError, match="tokens must be int8"):
        ops.solution_rebase(i8(3, 5, 13), lens, mats)
    with pytest.raises(_lib.TensorGameError, match="mats must be int32"):
        ops.solution_rebase(tok, lens, mats.to(torch.int8))
    with pytest.raises(_lib.TensorGameError, match="mats must be int32"):
        ops.solution_rebase(tok, lens, torch.zeros((3, 3, 5, 5), dtype=torch.int32))
    with pytest.raises(_lib.TensorGameError, match="lengths must be int64"):
        ops.solution_rebase(tok, lens.to(torch.int32), mats)
    with pytest.raises(_lib.TensorGameError, match="lengths must be int64"):
        ops.solution_rebase(tok, lens[:2], mats)
    with pytest.raises(_lib.TensorGameError, match="index must be given"):
        ops.solution_rebase(tok, lens, mats[:2])
    with pytest.raises(_lib.TensorGameError, match="index must be int64"):
        ops.solution_rebase(tok, lens, mats[:2], index=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(_lib.TensorGameError, match="index must be int64"):
        ops.solution_rebase(tok, lens, mats[:2], index=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.TensorGameError, match="tokens must live on a ROCm device.*no CPU path"):
        ops.solution_rebase(tok, lens, mats)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        mat_mul_amd.BasisSet(mats, mats, torch.zeros(3, dtype=torch.uint8), True)
