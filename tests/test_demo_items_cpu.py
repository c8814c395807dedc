"""CPU checks of the demo-items boundary (include/tensor_game_demos.h, tg_demo_items, ops.demo_items): the header is
plain C, the ctypes table covers it and both libraries export it, arguments are refused before any device work, and
the oracle helper of the GPU tests reproduces what the reference's __getitem__ recorded."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from mat_mul_amd import _lib, build, ops
from demo_items_ref import ref_items

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_demos.h"


def declared_symbols():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))


def test_demos_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_demos_header_symbols_exported_by_both_libraries():
    syms = declared_symbols()
    assert syms == ["tg_demo_items"]
    assert sorted(_lib.DEMO_SIGNATURES) == syms
    assert not set(syms) & set(_lib.SIGNATURES)
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)


def _call(**over):
    one = C.c_void_p(16)  # never dereferenced: validation fails first
    kw = dict(tokens=one, targets=one, n_demos=4, R=7, S=4, stride=64, idx=one, N=8, T=2, dtype=0, frames=one,
              scalars=None, actions=None, rewards=None, overflow=None, status=None, shift=1)
    kw.update(over)
    return _lib.lib.tg_demo_items(kw["tokens"], kw["targets"], kw["n_demos"], kw["R"], kw["S"], kw["stride"], kw["idx"],
                                  kw["N"], kw["T"], kw["dtype"], kw["frames"], kw["scalars"], kw["actions"],
                                  kw["rewards"], kw["overflow"], kw["status"], kw["shift"], None)


@pytest.mark.parametrize("over, words", [
    (dict(S=0), b"S=0"), (dict(S=33, stride=33 ** 3), b"S=33"),
    (dict(R=0), b"R=0"), (dict(R=4097), b"R=4097"),
    (dict(T=0), b"T=0"), (dict(T=4097), b"T=4097"),
    (dict(stride=63), b"target_stride_bytes"),
    (dict(dtype=-1), b"out_dtype"), (dict(dtype=4), b"out_dtype"),
    (dict(n_demos=-1), b"n_demos"), (dict(N=-1), b"N=-1"),
    (dict(idx=None), b"null"), (dict(frames=None), b"null"),
    (dict(tokens=None), b"null"), (dict(targets=None), b"null"),
    (dict(frames=C.c_void_p(17)), b"aligned"),
])
def test_tg_demo_items_refuses_invalid_arguments(over, words):
    assert _call(**over) == -1  # TG_ERR_INVALID
    assert words in _lib.lib.tg_last_error()


def test_tg_demo_items_empty_calls_are_noops():
    assert _call(N=0, tokens=None, targets=None, idx=None, frames=None) == 0
    assert _call(n_demos=0, tokens=None, targets=None, N=0) == 0


def test_demo_items_refuses_cpu_tensors():
    tok = torch.zeros((2, 7, 12), dtype=torch.int8)
    tgt = torch.zeros((2, 4, 4, 4), dtype=torch.int8)
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.demo_items(tok, tgt, torch.zeros((3,), dtype=torch.int64), 2)


def test_helper_reproduces_the_recorded_reference_items(golden):
    g = golden("reference_dataset_getitem")
    frames, sc, ac, rw, ovf, st = ref_items(g["tokens"], g["target"], np.arange(21), 2)
    assert np.array_equal(frames, g["frames"]) and np.array_equal(ac, g["action"])
    assert np.array_equal(np.concatenate([sc, rw], 1), g["meta"].astype(np.float32))
    assert not ovf.any() and st[0] == 0


def _ds_groups(g):
    for key in g.files:
        m = re.fullmatch(r"ds_S(\d+)_R(\d+)_T(\d+)_(\d+)_tokens", key)
        if m:
            yield key[:-len("tokens")], int(m[1]), int(m[2]), int(m[3])


def test_helper_reproduces_every_recorded_dataset_item(golden):
    g = golden("synthetic_demos")
    groups = list(_ds_groups(g))
    assert len(groups) == 7
    for pre, S, R, T in groups:
        frames, sc, ac, rw, ovf, st = ref_items(g[pre + "tokens"][None], g[pre + "target"][None], np.arange(R), T)
        for k in range(R):
            assert np.array_equal(frames[k], g[f"{pre}item{k}_frames"]), (pre, k)
            assert [sc[k, 0], rw[k, 0]] == g[f"{pre}item{k}_meta"].tolist(), (pre, k)
            assert np.array_equal(ac[k], g[f"{pre}item{k}_action"]), (pre, k)
        assert not ovf.any() and st[0] == 0


def test_helper_bad_indices_and_overflow():
    tok = np.full((1, 2, 3), 1 + 12, np.int8)  # S = 1, factors 12: tensor(a) = 1728
    tgt = np.zeros((1, 1, 1, 1), np.int8)
    frames, sc, ac, rw, ovf, st = ref_items(tok, tgt, [-1, 0, 1, 2], 2)
    assert st[0] == 1 and ovf.tolist() == [0, 1, 0, 0]
    assert not frames[[0, 3]].any() and not sc[[0, 3]].any() and not ac[[0, 3]].any()
    assert frames[1, 0, 0, 0, 0] == np.int8(np.int64(-1728).astype(np.int8))
