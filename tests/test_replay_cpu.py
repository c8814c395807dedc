"""CPU checks of the replay buffers (include/tensor_game_replay.h, mat_mul_amd.replay): the host restatement
(tests/replay_ref.py) reproduces what the reference's own PlayedGamesDataset, act_step loop and TensorGameDataset
recorded (tests/golden/replay_cases.npz, make_golden_replay.py); the header is plain C; both libraries export exactly
its symbols; the ctypes struct matches it; arguments are refused before any device work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import replay_ref as RR
from mat_mul_amd import _lib, build

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_replay.h"
RINGS = ["S4_T2", "S16_T1"]


def ring_games(g, name):
    return [g[f"ring_{name}_{k}"] for k in ("states", "policy", "rewards", "lengths")]


@pytest.mark.parametrize("name", RINGS)
def test_restatement_reproduces_the_reference_ring(golden, name):
    g = golden("replay_cases")
    states, policy, rewards, lengths = ring_games(g, name)
    ring = RR.Ring(3, states.shape[1])
    assert len(lengths) > 3  # the ring wraps
    for a in range(len(lengths)):
        assert ring.add(states[a:a + 1], policy[a:a + 1], rewards[a:a + 1], lengths[a:a + 1]) == 0
        items = [ring.getitem(i) for i in range(len(ring))]
        assert np.array_equal(np.stack([it[0] for it in items]), g[f"ring_{name}_snap{a}_frames"])
        assert np.array_equal(np.array([it[1] for it in items]), g[f"ring_{name}_snap{a}_scalar"])
        assert np.array_equal(np.stack([it[2] for it in items]), g[f"ring_{name}_snap{a}_action"])
        assert np.array_equal(np.array([it[3] for it in items]), g[f"ring_{name}_snap{a}_reward"])
    # one call with more games than the ring holds leaves what the sequential calls left
    once = RR.Ring(3, states.shape[1])
    once.add(states, policy, rewards, lengths)
    assert all(np.array_equal(x, y) for s in range(3) for x, y in zip(once.slots[s], ring.slots[s]))


def test_fixture_policies_have_ties_and_nans(golden):
    g = golden("replay_cases")
    pol = g["ring_S4_T2_policy"]
    top = pol.max(-1, keepdims=True)
    assert ((pol == top).sum(-1) > 1).any() and np.isnan(pol).any()
    assert (RR.argmax_tokens(pol) == 1).any() and (RR.argmax_tokens(pol) == 2).any()


def test_restatement_reproduces_the_best_game_rule(golden):
    g = golden("replay_cases")
    picks = []
    for i in range(4):
        rw, ln = g[f"best_{i}_rewards"], g[f"best_{i}_lengths"]
        picks.append(RR.best_pick(rw, ln, rw.shape[1]))
        assert picks[-1] == g[f"best_{i}_pick"].item(), i
    assert -1 in picks and 0 in picks and 1 in picks  # none, a tie won by the first, a later game


def mix_sources(g):
    tokens = g["mix_tokens"].astype(np.int8)
    targets = g["mix_targets"].astype(np.int8)
    played, best = RR.Ring(10000, 4), RR.Ring(100, 4)
    st, po, rw, ln = (g[f"mix_{k}"] for k in ("states", "policy", "rewards", "lengths"))
    played.add(st[:3], po[:3], rw[:3], ln[:3])
    best.add(st[3:], po[3:], rw[3:], ln[3:])
    return tokens, targets, played, best


def mix_state(g, k):
    return (g[f"mix_{k}_is_synth"], g[f"mix_{k}_index_synth"],
            g[f"mix_{k}_index_played"] if g[f"mix_{k}_has_played"] else None,
            g[f"mix_{k}_index_best"] if g[f"mix_{k}_has_best"] else None, float(g[f"mix_{k}_fract"][1]))


@pytest.mark.parametrize("k", range(4))
def test_restatement_reproduces_the_reference_mixture(golden, k):
    g = golden("replay_cases")
    tokens, targets, played, best = mix_sources(g)
    kind, src = RR.route(*mix_state(g, k))
    assert (kind != RR.BAD).all()
    frames, sc, ac, rw, status = RR.mixed_items(kind, src, tokens, targets, played, best, 2)
    assert status == 0
    assert np.array_equal(frames.astype(np.float32), g[f"mix_{k}_frames"])
    assert np.array_equal(sc[:, 0], g[f"mix_{k}_scalar"]) and np.array_equal(rw[:, 0], g[f"mix_{k}_reward"])
    assert np.array_equal(ac.astype(np.int64), g[f"mix_{k}_action"])


def test_mixture_fixture_covers_the_states(golden):
    g = golden("replay_cases")
    kinds = [RR.route(*mix_state(g, k))[0] for k in range(4)]
    assert (kinds[0] == RR.SYNTH).all()                                       # played buffer empty
    assert set(kinds[1].tolist()) == {RR.SYNTH, RR.PLAYED}                   # played only
    assert set(kinds[2].tolist()) == {RR.SYNTH, RR.BEST}                     # the reference's split: no played item
    ip = g["mix_3_index_played"]
    assert len(ip) > len(np.unique(ip)) and len(ip) > int(g["mix_lengths"][:3].sum())  # drawn with replacement
    assert len(np.unique(g["mix_1_index_played"])) == len(g["mix_1_index_played"])   # drawn without


def test_replay_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_replay_header_symbols_exported_by_both_libraries():
    syms = sorted(set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_replay_add", "tg_replay_items"]
    assert sorted(_lib.REPLAY_SIGNATURES) == syms
    assert not set(syms) & (set(_lib.SIGNATURES) | set(_lib.DEMO_SIGNATURES) | set(_lib.SEARCH_SIGNATURES))
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)


def test_descriptor_layout_matches_header():
    text = HDR.read_text()
    body = text[text.index("typedef struct tg_replay_buffer {"):text.index("} tg_replay_buffer;")]
    names = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*(?:u?int\d+_t|float)\*?\s+([A-Za-z_][A-Za-z0-9_, ]*?)\s*;", line)
        if m:
            names += [n.strip() for n in m.group(1).split(",")]
    assert names == [f[0] for f in _lib.ReplayBufferDesc._fields_]
    assert C.sizeof(_lib.ReplayBufferDesc) == 16 + 6 * 8
    for name in ("MAX_CAPACITY", "MAX_ACTIONS", "MAX_T", "MAX_LOGITS"):
        assert int(re.search(rf"#define TG_REPLAY_{name} (\d+)", text).group(1)) == getattr(_lib, f"TG_REPLAY_{name}")


def _desc(**over):
    d = _lib.ReplayBufferDesc(C=8, L=4, T=2, S=4)
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        setattr(d, name, 4096)  # never dereferenced: validation fails first
    for key, val in over.items():
        setattr(d, key, val)
    return d


def _add(d=None, **over):
    one = C.c_void_p(4096)
    kw = dict(states=one, policy=one, n_logits=3, rewards=one, lengths=one, B=2, select=0)
    kw.update(over)
    return _lib.lib.tg_replay_add(None if d is None else C.byref(d), kw["states"], kw["policy"], kw["n_logits"],
                                  kw["rewards"], kw["lengths"], kw["B"], kw["select"], None, None)


def _items(played=None, best=None, **over):
    one = C.c_void_p(4096)
    kw = dict(tokens=one, targets=one, n_demos=4, R=4, S=4, stride=64, kind=None, src=None, len_data=0, direct=1,
              idx=one, N=8, T=2, dtype=0, frames=one)
    kw.update(over)
    return _lib.lib.tg_replay_items(kw["tokens"], kw["targets"], kw["n_demos"], kw["R"], kw["S"], kw["stride"], 1,
                                    None if played is None else C.byref(played), None if best is None else C.byref(best),
                                    kw["kind"], kw["src"], kw["len_data"], kw["direct"], kw["idx"], kw["N"], kw["T"],
                                    kw["dtype"], kw["frames"], None, None, None, None, None, None)


@pytest.mark.parametrize("over, words", [
    (dict(C=0), b"C=0"), (dict(C=65537), b"C=65537"), (dict(L=0), b"L=0"), (dict(L=4097), b"L=4097"),
    (dict(T=0), b"T=0"), (dict(T=17), b"T=17"), (dict(S=0), b"S=0"), (dict(S=33), b"S=33"),
    (dict(frames=None), b"null"), (dict(ring=None), b"null"), (dict(offset=4100), b"aligned"),
])
def test_buffer_validation_without_gpu(over, words):
    lib = _lib.lib
    assert _add(_desc(**over)) == -1 and words in lib.tg_last_error(), lib.tg_last_error()
    assert _items(played=_desc(**over)) == -1 and words in lib.tg_last_error(), lib.tg_last_error()


def test_add_validation_without_gpu():
    lib = _lib.lib
    d = _desc()
    assert _add(None) == -1 and b"null buffer" in lib.tg_last_error()
    for over, words in ((dict(n_logits=0), b"n_logits=0"), (dict(n_logits=129), b"n_logits=129"),
                        (dict(select=2), b"select=2"), (dict(select=-1), b"select=-1"), (dict(B=-1), b"B=-1"),
                        (dict(states=None), b"null"), (dict(policy=None), b"null"), (dict(lengths=None), b"null"),
                        (dict(rewards=C.c_void_p(4098)), b"aligned"), (dict(lengths=C.c_void_p(4100)), b"aligned")):
        assert _add(d, **over) == -1 and words in lib.tg_last_error(), (over, lib.tg_last_error())
    assert _add(d, B=0, states=None, policy=None) == 0  # an empty batch is a no-op


def test_items_validation_without_gpu():
    lib = _lib.lib
    d = _desc()
    for kw, words in ((dict(played=_desc(T=1)), b"T=1"), (dict(best=_desc(S=3)), b"S=3"),
                      (dict(direct=3), b"direct_kind=3"), (dict(direct=-1), b"direct_kind=-1"),
                      (dict(kind=C.c_void_p(4096)), b"null src"),
                      (dict(kind=C.c_void_p(4096), src=C.c_void_p(4096), len_data=-1), b"len_data"),
                      (dict(frames=C.c_void_p(4098)), b"aligned"), (dict(dtype=4), b"out_dtype"),
                      (dict(T=0), b"T=0"), (dict(S=0), b"S=0"), (dict(R=0), b"R=0"),
                      (dict(idx=None), b"null"), (dict(tokens=None), b"null"), (dict(stride=63), b"target_stride")):
        args = dict(played=d)
        args.update(kw)
        assert _items(**args) == -1 and words in lib.tg_last_error(), (kw, lib.tg_last_error())
    assert _items(played=d, N=0, idx=None, frames=None) == 0
    assert _items(played=d, n_demos=0, tokens=None, targets=None, N=0) == 0


def test_buffers_refuse_the_cpu():
    from mat_mul_amd import replay

    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        replay.GameBuffer(4, 4, 1, 4, device="cpu")


def test_golden_generator_is_byte_identical(tmp_path):
    """make_golden_replay.py, rerun against the reference, writes the committed fixture byte for byte."""
    import importlib.util
    import os
    import sys

    gen = ROOT / "tests" / "golden" / "make_golden_replay.py"
    spec = importlib.util.spec_from_file_location("make_golden_replay", gen)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not Path(mod.REF).exists():
        pytest.skip("the reference checkout the generator drives is not present")
    out = tmp_path / "replay_cases.npz"
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    res = subprocess.run([sys.executable, str(gen), str(out)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    assert out.read_bytes() == (ROOT / "tests" / "golden" / "replay_cases.npz").read_bytes()
