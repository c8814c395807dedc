"""CPU checks of the symmetry augmentation (include/tensor_game_symmetry.h): the host restatement's own algebra (the
inverse element, the step commuting with the group), its sampler (permutations, flags, id splits, uniformity of the
rule at a fixed seed -- the GPU sampler is pinned to the restatement bit for bit, so no statistics run there), the
header and the bindings, the argument checks, and ``Augment``'s bookkeeping."""
import ctypes as C
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import symmetry_ref as SR
from mat_mul_amd import Augment, _lib, build, ops

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_symmetry.h"


def random_items(rng, N, T, S, shift=1):
    frames = rng.integers(-127, 128, size=(N, T, S, S, S)).astype(np.int8)
    tokens = rng.integers(0, 2 * shift + 1, size=(N, 3 * S)).astype(np.int8)
    return frames, tokens


@pytest.mark.parametrize("S", [3, 4, 5])
def test_apply_then_inverse_is_the_identity(S):
    rng = np.random.default_rng(S)
    frames, tokens = random_items(rng, 40, 2, S, shift=2)
    sym = SR.sample(40, S, seed=11 + S)
    f1, t1, ov, st = SR.apply(frames, tokens, sym, shift=2)
    assert st == 0 and not ov.any()
    assert not np.array_equal(f1, frames) and not np.array_equal(t1, tokens)
    f2, t2, ov, st = SR.apply(f1, t1, SR.inverse(sym, S), shift=2)
    assert st == 0 and not ov.any()
    assert np.array_equal(f2, frames) and np.array_equal(t2, tokens)
    fi, ti, _, _ = SR.apply(frames, tokens, SR.identity(40, S), shift=2)
    assert np.array_equal(fi, frames) and np.array_equal(ti, tokens)


@pytest.mark.parametrize("S", [3, 4, 5])
def test_the_step_commutes_with_the_group(S):
    rng = np.random.default_rng(50 + S)
    x = rng.integers(-3, 4, size=(30, S, S, S)).astype(np.int8)
    a = rng.integers(0, 3, size=(30, 3 * S)).astype(np.int8)
    sym = SR.sample(30, S, seed=5)
    gx, ga, _, _ = SR.apply(x, a, sym)
    left, _ = SR.step(gx, ga)
    right, _, _, _ = SR.apply(SR.step(x, a)[0].astype(np.int8), None, sym)
    assert np.array_equal(left, right)


def test_apply_flags_overflow_and_bad_rows():
    S = 3
    x = np.zeros((4, 1, S, S, S), np.int8)
    x[:, 0, 0, 0, 0] = -128
    tok = np.full((4, 3 * S), 1, np.int8)
    tok[2, 0] = -128
    sym = SR.identity(4, S)
    sym[1, 1] |= 0x80        # item 1: entry (0,0,0) negated
    sym[2, 1] |= 0x80        # item 2 too, and its token 0
    sym[3, 2] = S            # item 3: a bad index
    f, t, ov, st = SR.apply(x, tok, sym)
    assert ov.tolist() == [0, 1, 1, 0] and st == 1
    assert f[1, 0, 0, 0, 0] == -128 and t[2, 0] == np.int8(np.int64(130).astype(np.int8))
    assert not f[3].any() and not t[3].any()


@pytest.mark.parametrize("S", [1, 4, 9, 32])
def test_sampler_gives_permutations_and_keeps_the_stream(S):
    N = 200
    full = SR.sample(N, S, seed=3)
    assert full.shape == (N, 3 * S + 1) and full[:, 0].max() <= 5
    idx = (full[:, 1:] & 0x7F).reshape(N, 3, S)
    assert (np.sort(idx, axis=2) == np.arange(S)).all()
    ident = SR.identity(N, S)
    for flag, cols in ((SR.MODES, slice(0, 1)), (SR.PERMS, None), (SR.SIGNS, None)):
        part = SR.sample(N, S, seed=3, flags=flag)
        if flag == SR.MODES:
            assert np.array_equal(part[:, 0], full[:, 0]) and np.array_equal(part[:, 1:], ident[:, 1:])
        elif flag == SR.PERMS:
            assert not part[:, 0].any() and np.array_equal(part[:, 1:], full[:, 1:] & 0x7F)
        else:
            assert not part[:, 0].any() and np.array_equal(part[:, 1:] & 0x80, full[:, 1:] & 0x80)
            assert np.array_equal(part[:, 1:] & 0x7F, ident[:, 1:])
    assert np.array_equal(SR.sample(N, S, seed=3, flags=0), ident)
    off = 2 ** 32 - 70  # the ids cross 2^32
    whole = SR.sample(N, S, seed=3, item_offset=off)
    halves = np.concatenate([SR.sample(90, S, seed=3, item_offset=off), SR.sample(N - 90, S, seed=3, item_offset=off + 90)])
    assert np.array_equal(whole, halves) and not np.array_equal(whole, full)


def test_the_rule_is_uniform_at_a_fixed_seed():
    """chi^2 of pi_0 over the 24 permutations of S = 4 and of the mode code over its 6 values, 24 000 ids, against the
    p = 1e-3 critical values (49.7 at 23 degrees of freedom, 20.5 at 5)."""
    N, S = 24000, 4
    rows = SR.sample(N, S, seed=2024)
    perms = {p: i for i, p in enumerate(itertools.permutations(range(S)))}
    pi0 = rows[:, 1:1 + S] & 0x7F
    counts = np.bincount([perms[tuple(p)] for p in pi0.tolist()], minlength=24)
    chi_pi = float(((counts - N / 24) ** 2 / (N / 24)).sum())
    codes = np.bincount(rows[:, 0], minlength=6)
    chi_rho = float(((codes - N / 6) ** 2 / (N / 6)).sum())
    signs = (rows[:, 1:] >> 7).mean()
    print(f"chi2 pi_0 = {chi_pi:.2f} (23 dof), chi2 rho = {chi_rho:.2f} (5 dof), negative signs = {signs:.4f}")
    assert chi_pi < 49.7 and chi_rho < 20.5
    assert abs(signs - 0.5) < 5 * 0.5 / np.sqrt(N * 3 * S)


# ---- header and bindings ---------------------------------------------------------------------------------------------
def declared_symbols():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))


def test_symmetry_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_symmetry_symbols_are_declared_and_exported():
    syms = declared_symbols()
    assert syms == ["tg_symmetry_apply", "tg_symmetry_sample"] == sorted(_lib.SYMMETRY_SIGNATURES)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "SYMMETRY_SIGNATURES"]
    assert not any(set(syms) & set(o) for o in others)
    assert HDR in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    assert (_lib.TG_SYM_MODES, _lib.TG_SYM_PERMS, _lib.TG_SYM_SIGNS) == (SR.MODES, SR.PERMS, SR.SIGNS)
    assert "symmetry_apply" in ops.__all__ and "symmetry_sample" in ops.__all__


def _apply(**over):
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    kw = dict(fin=p(16), ain=p(1024), sym=p(2048), N=8, T=2, S=4, shift=1, dtype=0, fout=p(4096), aout=p(8192),
              overflow=None, status=None)
    kw.update(over)
    return _lib.lib.tg_symmetry_apply(kw["fin"], kw["ain"], kw["sym"], kw["N"], kw["T"], kw["S"], kw["shift"],
                                      kw["dtype"], kw["fout"], kw["aout"], kw["overflow"], kw["status"], None)


@pytest.mark.parametrize("over, words", [
    (dict(S=0), b"S=0"), (dict(S=33), b"S=33"), (dict(T=0), b"T=0"), (dict(T=4097), b"T=4097"),
    (dict(dtype=4), b"out_dtype"), (dict(dtype=-1), b"out_dtype"), (dict(N=-1), b"N=-1"),
    (dict(sym=None), b"null"), (dict(fin=None), b"null"), (dict(fout=None), b"null"),
    (dict(fout=C.c_void_p(16)), b"in-place"), (dict(aout=C.c_void_p(1024)), b"in-place"),
    (dict(aout=None), b"together"), (dict(ain=None), b"together"),
    (dict(fout=C.c_void_p(4098)), b"aligned"),
])
def test_tg_symmetry_apply_refuses_invalid_arguments(over, words):
    assert _apply(**over) == -1  # TG_ERR_INVALID
    assert words in _lib.lib.tg_last_error()


def test_tg_symmetry_sample_refuses_invalid_arguments_and_empty_calls_are_noops():
    sample = _lib.lib.tg_symmetry_sample
    for args, words in (((C.c_void_p(16), 8, 0, 1, 0, 7, None), b"S=0"), ((C.c_void_p(16), 8, 33, 1, 0, 7, None), b"S=33"),
                        ((C.c_void_p(16), 8, 4, 1, 0, 8, None), b"flags"), ((C.c_void_p(16), -1, 4, 1, 0, 7, None), b"N=-1"),
                        ((None, 8, 4, 1, 0, 7, None), b"null")):
        assert sample(*args) == -1 and words in _lib.lib.tg_last_error()
    assert sample(None, 0, 4, 1, 0, 7, None) == 0
    assert _apply(N=0, fin=None, fout=None, sym=None, ain=None, aout=None) == 0


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    x = torch.zeros((3, 2, 4, 4, 4), dtype=torch.int8)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.symmetry_apply(x, torch.zeros((3, 12), dtype=torch.int8), torch.zeros((3, 13), dtype=torch.uint8))
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.symmetry_sample(3, 4, "cpu")
    with pytest.raises(_lib.TensorGameError, match=r"S=33"):
        ops.symmetry_sample(3, 33, "cuda")


def test_augment_checks_the_vocabulary_and_keeps_its_ids():
    with pytest.raises(_lib.TensorGameError, match="n_logits"):
        Augment(1, signs=True, n_logits=4, shift=1)
    Augment(1, signs=False, n_logits=4, shift=1)
    Augment(1, signs=True, n_logits=5, shift=2)
    aug = Augment(7, modes=False, shift=2, n_logits=5)
    assert aug.state_dict() == {"seed": 7, "flags": 6, "next_id": 0, "shift": 2}
    aug.next_id = 12345678901
    other = Augment(0)
    other.load_state_dict(aug.state_dict())
    assert other.state_dict() == aug.state_dict() and all(type(v) is int for v in other.state_dict().values())
    import mat_mul_amd

    assert "Augment" in mat_mul_amd.__all__ and mat_mul_amd.augment.Augment is Augment
