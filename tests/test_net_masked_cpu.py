"""CPU checks of the row-masked network entries (tg_net_torso_masked, tg_net_sample_masked of
include/tensor_game_net.h): both libraries export them and the ctypes table lists them, the header declares them and
still compiles as plain C, the arguments are validated before any launch, and ``FusedAlphaTensor.policy`` marks its
masked policy with ``takes_flags``.  No GPU needed."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from mat_mul_amd import _lib, build, net, ops

from net_ref import CONFIGS, dims
from net_s16_ref import CONFIGS as CONFIGS_S16

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "tensor_game_net.h"
MASKED = ("tg_net_torso_masked", "tg_net_sample_masked")


def test_both_libraries_export_the_masked_entries():
    declared = set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", HEADER.read_text(), flags=re.M))
    assert set(MASKED) <= declared
    assert declared == set(_lib.NET_SIGNATURES)  # the ctypes table covers the header exactly
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in MASKED:
            assert hasattr(lib, s), (path, s)
    # the plain signature, then flags and need in front of the stream
    for plain, masked in zip(("tg_net_torso", "tg_net_sample"), MASKED):
        sig = _lib.NET_SIGNATURES[plain]
        assert _lib.NET_SIGNATURES[masked] == sig[:-1] + [C.c_void_p, C.c_int] + sig[-1:]
    assert _lib.lib.tg_abi_version() == 4  # an addition only


def test_the_header_is_still_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror", str(HEADER)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


@pytest.mark.parametrize("name", ["a", "a16"])
def test_argument_validation_without_gpu(name):
    lib = _lib.lib
    m = dims({**CONFIGS, **CONFIGS_S16}[name])
    cfg = net.check_config(m)
    bad = _lib.NetConfig(**dict(m, S=11))
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch
    torso, sample = lib.tg_net_torso_masked, lib.tg_net_sample_masked
    # need = 0 (or outside a byte) with flags given
    assert torso(C.byref(cfg), p, p, 0, p, p, 4, p, 0, None) == -1
    assert b"need=0" in lib.tg_last_error()
    assert torso(C.byref(cfg), p, p, 0, p, p, 4, p, 256, None) == -1
    assert sample(C.byref(cfg), p, p, p, 4, 8, 0, 0, None, None, None, None, p, 0, None) == -1
    assert b"need=0" in lib.tg_last_error()
    assert sample(C.byref(cfg), p, p, p, 4, 8, 0, 0, None, None, None, None, p, -1, None) == -1
    # the plain entries' checks, with and without a mask
    for flags, need in ((p, 129), (None, 0)):
        assert torso(C.byref(cfg), None, p, 0, p, p, 4, flags, need, None) == -1
        assert b"null weights" in lib.tg_last_error()
        assert torso(C.byref(cfg), p, None, 0, p, p, 4, flags, need, None) == -1  # null frames
        assert torso(C.byref(cfg), p, p, 0, p, None, 4, flags, need, None) == -1  # null ee
        assert torso(C.byref(cfg), p, p, 2, p, p, 4, flags, need, None) == -1
        assert torso(C.byref(cfg), p, p, 0, p, C.c_void_p(66), 4, flags, need, None) == -1  # misaligned ee
        assert torso(C.byref(cfg), p, p, 0, p, p, -1, flags, need, None) == -1
        assert torso(C.byref(cfg), p, None, 0, None, None, 0, flags, need, None) == 0  # B = 0 is a no-op
        assert sample(C.byref(cfg), p, None, p, 4, 8, 0, 0, None, None, None, None, flags, need, None) == -1  # null ee
        assert sample(C.byref(cfg), p, p, None, 4, 8, 0, 0, None, None, None, None, flags, need, None) == -1
        assert sample(C.byref(cfg), p, p, p, 4, 65, 0, 0, None, None, None, None, flags, need, None) == -2
        assert b"TG_NET_MAX_SAMPLES" in lib.tg_last_error()
        assert sample(C.byref(cfg), p, p, p, 4, 0, 0, 0, None, None, None, None, flags, need, None) == -2
        assert sample(C.byref(cfg), p, None, None, 0, 8, 0, 0, None, None, None, None, flags, need, None) == 0
        assert torso(C.byref(bad), p, p, 0, p, p, 4, flags, need, None) == -2
        assert b"TG_NET_MAX_S" in lib.tg_last_error()
        assert sample(C.byref(bad), p, p, p, 4, 8, 0, 0, None, None, None, None, flags, need, None) == -2
        assert b"TG_NET_MAX_S" in lib.tg_last_error()
    # the order is the plain entry's: the configuration and k come before the mask
    assert torso(C.byref(bad), p, p, 0, p, p, 4, p, 0, None) == -2
    assert sample(C.byref(cfg), p, p, p, 4, 65, 0, 0, None, None, None, None, p, 0, None) == -2


def test_the_masked_policy_says_that_it_takes_flags():
    cfg = net.check_config(dims(CONFIGS["a"]))
    # no device is touched before the first call: a host blob of the right size is enough to make the two policies
    fused = net.FusedAlphaTensor(dims(CONFIGS["a"]), torch.zeros(ops.net_weights_size(cfg)), 8)
    assert getattr(fused.policy(seed=3, masked=True), "takes_flags", False) is True
    assert not hasattr(fused.policy(seed=3), "takes_flags")
    assert not hasattr(fused.policy(seed=3, masked=False), "takes_flags")
