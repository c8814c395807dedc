"""CPU checks of the batched search (include/tensor_game_search.h, mat_mul_amd.search): the header is plain C, the
ctypes table covers it and both libraries export it, arguments are refused before any device work, and the host
restatement (tests/search_ref.py) reproduces every game the reference's own actor_prediction played
(tests/golden/search_games.npz, make_golden_search.py)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib, build, search
from oracle import tensor_game as O
import search_ref as R

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_search.h"
CASES = ["S4_T1", "S4_T2", "S4_T2_lowrank", "S3_T1", "S5_T2", "S16_T1"]


def test_search_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_search_header_symbols_exported_by_both_libraries():
    syms = sorted(set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == ["tg_search_advance", "tg_search_commit", "tg_search_policy", "tg_search_reset", "tg_search_select"]
    assert sorted(_lib.SEARCH_SIGNATURES) == syms
    assert not set(syms) & (set(_lib.SIGNATURES) | set(_lib.DEMO_SIGNATURES))
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)


def test_descriptor_layout_matches_header():
    """The ctypes struct has the header's fields in the header's order (sizes first, then 28 device pointers)."""
    text = HDR.read_text()
    body = text[text.index("typedef struct tg_search_forest {"):text.index("} tg_search_forest;")]
    names = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*(?:u?int\d+_t|float)\*?\s+([A-Za-z_][A-Za-z0-9_, ]*?)\s*;", line)
        if m:
            names += [n.strip() for n in m.group(1).split(",")]
    assert names == [f[0] for f in _lib.SearchForestDesc._fields_]
    assert C.sizeof(_lib.SearchForestDesc) == 48 + 28 * 8


def _desc(**over):
    d = _lib.SearchForestDesc(B=4, S=4, T=2, k=8, M=33, index_capacity=128, max_actions=4, horizon=5, max_depth=64,
                              shift=1)
    for name, _ in _lib.SearchForestDesc._fields_[10:]:
        if name != "child_prior":
            setattr(d, name, 4096)  # never dereferenced: validation fails first
    for key, val in over.items():
        setattr(d, key, val)
    return d


@pytest.mark.parametrize("over, words", [
    (dict(S=0), b"S=0"), (dict(S=33), b"S=33"), (dict(T=0), b"T=0"), (dict(T=17), b"T=17"),
    (dict(k=0), b"k=0"), (dict(k=65), b"k=65"), (dict(M=0), b"M=0"),
    (dict(index_capacity=96), b"index_capacity=96"), (dict(index_capacity=1), b"index_capacity=1"),
    (dict(max_actions=0), b"max_actions=0"), (dict(max_depth=0), b"max_depth=0"), (dict(horizon=-1), b"horizon=-1"),
    (dict(node_frames=4104), b"16-byte"), (dict(child_key=4100), b"8-byte"), (dict(flags=None), b"null forest array"),
])
def test_forest_validation_without_gpu(over, words):
    lib = _lib.lib
    d = _desc(**over)
    one = C.c_void_p(16)
    for rc in (lib.tg_search_reset(C.byref(d), one, 4, None), lib.tg_search_select(C.byref(d), None, 0, None, None),
               lib.tg_search_commit(C.byref(d), one, one, None, None, None), lib.tg_search_advance(C.byref(d), 4, None),
               lib.tg_search_policy(C.byref(d), one, 3, 2, None)):
        assert rc == -1
        assert words in lib.tg_last_error(), lib.tg_last_error()


def test_call_validation_without_gpu():
    lib = _lib.lib
    d = _desc()
    one = C.c_void_p(16)
    assert lib.tg_search_reset(None, one, 4, None) == -1 and b"null forest" in lib.tg_last_error()
    assert lib.tg_search_reset(C.byref(d), one, -1, None) == -1 and b"n_sim" in lib.tg_last_error()
    assert lib.tg_search_reset(C.byref(d), None, 4, None) == -1 and b"null states" in lib.tg_last_error()
    assert lib.tg_search_select(C.byref(d), one, 3, None, None) == -1 and b"out_dtype" in lib.tg_last_error()
    assert lib.tg_search_commit(C.byref(d), None, one, None, None, None) == -1
    assert lib.tg_search_policy(C.byref(d), one, 0, 2, None) == -1 and b"n_logits" in lib.tg_last_error()
    assert lib.tg_search_policy(C.byref(d), one, 3, 0, None) == -1 and b"n_bar" in lib.tg_last_error()
    assert lib.tg_search_advance(C.byref(d), -2, None) == -1
    empty = _desc(B=0)
    assert lib.tg_search_select(C.byref(empty), None, 0, None, None) == 0  # an empty forest is a no-op


def test_forest_refuses_the_cpu():
    with pytest.raises(search.TensorGameError):
        search.SearchForest(2, 4, device="cpu", n_sim=4)


def fixture_policy(g, case):
    """policy_fn of search_ref.play that answers from the fixture's call table; a miss raises."""
    table = {}
    for head, att, scal, tok, q in zip(g[f"{case}_call_head"], g[f"{case}_call_attempt"], g[f"{case}_call_scalar"],
                                       g[f"{case}_call_tokens"], g[f"{case}_call_q"]):
        table[(head.tobytes(), int(att))] = (tok, np.float32(q), float(scal))

    def fn(head, frames, scalar, attempt, key):
        tok, q, scal = table[(np.asarray(head, np.int8).tobytes(), attempt)]
        assert scal == scalar
        return tok, q

    return fn


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_games(golden, case):
    g = golden("search_games")
    S, T, k, n_sim, max_actions, n_bar, n_logits, horizon, games, skipped = (int(x) for x in g[f"{case}_meta"])
    fn = fixture_policy(g, case)
    for gi in range(games):
        r = R.play(fn, g[f"{case}_start"][gi], max_actions, n_sim, n_bar, n_logits, horizon=horizon)
        L = r["length"]
        assert L == int(g[f"{case}_lengths"][gi])
        rows = np.flatnonzero(g[f"{case}_call_game"] == gi)                 # the calls the reference made in this game
        assert len(r["calls"]) == len(rows), (case, gi)
        for (frames, scalar, attempt, key), row in zip(r["calls"], rows):
            assert frames.shape == (T, S, S, S) and key == R.head_key(frames[0])
            assert np.array_equal(frames[0], g[f"{case}_call_head"][row]), (case, gi, row)
            assert float(scalar) == float(g[f"{case}_call_scalar"][row]) and attempt == int(g[f"{case}_call_attempt"][row])
        assert r["overflow"] is False
        assert np.array_equal(r["states"], g[f"{case}_states"][gi][:L])
        assert not g[f"{case}_states"][gi][L:].any()
        assert np.array_equal(r["policy"].view(np.int32), g[f"{case}_policy"][gi][:L].view(np.int32)), (case, gi)
        assert np.array_equal(r["rewards"], g[f"{case}_rewards"][gi][:L])
        assert np.array_equal(r["choice"], g[f"{case}_choice"][gi][:L])
        for m in range(L):
            nc = int(g[f"{case}_root_nc"][gi][m])
            assert len(r["root_N"][m]) == nc
            assert np.array_equal(r["root_N"][m].view(np.int32), g[f"{case}_root_n"][gi][m][:nc].view(np.int32))
            assert np.array_equal(r["root_Q"][m].view(np.int32), g[f"{case}_root_q"][gi][m][:nc].view(np.int32)), (case, gi, m)


def test_restatement_flags_a_child_that_leaves_int8():
    """A head of 127 with a product of -1 is 128 before the wrap: ``overflow`` is set (and the stored head wraps to
    -128); the same action on a head of 126 sets nothing."""
    S = 4
    minus = np.array([2, 1, 1, 1, 2, 1, 1, 1, 0, 1, 1, 1], np.int8)       # u = e0, v = e0, w = -e0: product -1 at [0,0,0]
    null = np.ones(12, np.int8)
    for top, want in ((127, True), (126, False)):
        start = np.zeros((1, S, S, S), np.int8)
        start[0, 0, 0, 0], start[0, 1, 1, 1] = top, 1
        r = R.play(lambda *a: (np.stack([null, minus]), np.float32(0.25)), start, 1, 1, 100, 3)
        assert r["overflow"] is want and r["length"] == 1 and len(r["calls"]) == 1
        assert int(r["final"][0, 0, 0, 0]) == (-128 if want else 127)


def test_fixture_covers_the_branches(golden):
    """The recorded cases cover T = 1 and 2, n_sim 4 and 16, max_actions 4 and 8 (the horizon bound), both branches of
    the improved policy's tau, an odd S, S = 16 and at least one retry."""
    g = golden("search_games")
    metas = {c: g[f"{c}_meta"] for c in CASES}
    assert {int(m[1]) for m in metas.values()} == {1, 2}
    assert {int(m[3]) for m in metas.values()} >= {4, 16} and {int(m[4]) for m in metas.values()} >= {4, 8}
    assert {int(m[5]) for m in metas.values()} == {2, 100}
    assert any(int(m[0]) % 2 for m in metas.values()) and any(int(m[0]) == 16 for m in metas.values())
    assert sum(int((g[f"{c}_call_attempt"] > 0).sum()) for c in CASES) > 0


def test_keyed_policy_restatement_is_deterministic():
    pool = np.random.default_rng(0).integers(0, 3, size=(6, 12)).astype(np.int8)
    fn = R.keyed_policy(pool, 8, seed=3)
    a = fn(None, None, 0, 0, 12345)
    b = fn(None, None, 0, 0, 12345)
    c = fn(None, None, 0, 1, 12345)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and not np.array_equal(a[0], c[0])
    assert -1.0 <= a[1] < 1.0 and a[0].shape == (8, 12) and a[0].min() >= 0 and a[0].max() <= 2


def test_golden_generator_is_byte_identical(tmp_path):
    """make_golden_search.py, rerun against the reference, writes the committed fixture byte for byte."""
    import importlib.util
    import os
    import sys

    gen = ROOT / "tests" / "golden" / "make_golden_search.py"
    spec = importlib.util.spec_from_file_location("make_golden_search", gen)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not Path(mod.REF).exists():
        pytest.skip("the reference checkout the generator drives is not present")
    out = tmp_path / "search_games.npz"
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    res = subprocess.run([sys.executable, str(gen), str(out)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    assert out.read_bytes() == (ROOT / "tests" / "golden" / "search_games.npz").read_bytes()
