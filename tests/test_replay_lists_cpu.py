"""CPU checks of move lists stored as games (include/tensor_game_replay_lists.h): the header is plain C, both libraries
export its symbol and the ctypes signature follows its prototype; the entry refuses bad arguments in its documented order
before any device work; the host restatement (tests/replay_lists_ref.py) reproduces what the reference leaves in its own
ring (tests/golden/replay_lists_cases.npz) and agrees with replay_ref's tg_replay_add on the padded form."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import replay_io_ref as IO
import replay_lists_ref as LR
import replay_ref as RR
import ring_cases as RC
from mat_mul_amd import _lib, build

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_replay_lists.h"
CASES = ["S4_T2", "S9_T4"]


# ---- the header ---------------------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_symbol_exported_and_signature_follows_the_prototype():
    text = HDR.read_text()
    syms = sorted(set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", text, flags=re.M)))
    assert syms == ["tg_replay_add_lists"] == sorted(_lib.REPLAY_LISTS_SIGNATURES)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "REPLAY_LISTS_SIGNATURES"]
    assert len(others) >= 10 and not any(set(syms) & set(t) for t in others)
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        assert hasattr(C.CDLL(str(path)), syms[0]), path
    args = re.search(r"^int\s+tg_replay_add_lists\s*\((.*?)\);", text, flags=re.M | re.S).group(1).split(",")
    kinds = [C.c_void_p if "*" in a or "tg_stream_t" in a else C.c_int64 if "int64_t" in a else C.c_int for a in args]
    assert len(args) == 13 and kinds == _lib.REPLAY_LISTS_SIGNATURES["tg_replay_add_lists"]
    assert _lib.lib.tg_replay_add_lists.argtypes == kinds
    for name in ("BAD_LENGTH", "BAD_GROUP", "BAD_RANGE", "NOT_ZERO"):
        bit = int(re.search(rf"#define TG_REPLAY_LISTS_{name} (\d+)u", text).group(1))
        assert bit == getattr(_lib, f"TG_REPLAY_LISTS_{name}") == getattr(LR, name)
    assert int(re.search(r"#define TG_REPLAY_LISTS_MAX_SHIFT (\d+)", text).group(1)) == _lib.TG_REPLAY_LISTS_MAX_SHIFT
    assert build.PKG.parent / "include" / "tensor_game_replay_lists.h" in build.HEADERS


# ---- the host checks, in their order --------------------------------------------------------------------------------------
ONE = 64  # a pointer that is never dereferenced: validation fails first


def _desc(**over):
    d = _lib.ReplayBufferDesc(C=8, L=4, T=2, S=4)
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        setattr(d, name, ONE)
    for key, val in over.items():
        setattr(d, key, val)
    return d


def _add(d, **over):
    kw = dict(starts=ONE, G=3, groups=ONE, tokens=ONE, lengths=ONE, M=2, K=4, shift=1, select=0, stored=ONE, status=ONE)
    kw.update(over)
    p = lambda k: C.c_void_p(kw[k])
    return _lib.lib.tg_replay_add_lists(None if d is None else C.byref(d), p("starts"), kw["G"], p("groups"),
                                        p("tokens"), p("lengths"), kw["M"], kw["K"], kw["shift"], kw["select"],
                                        p("stored"), p("status"), None)


def refused(words, d, **over):
    err = _lib.lib.tg_last_error
    assert _add(d, **over) == -1 and b"tg_replay_add_lists" in err() and words in err(), (over, err())


def test_validation_without_gpu_in_order():
    refused(b"null buffer", None)
    sizes = [(dict(C=0), b"C=0"), (dict(C=65537), b"C=65537"), (dict(L=0), b"L=0"), (dict(L=4097), b"L=4097"),
             (dict(T=0), b"T=0"), (dict(T=17), b"T=17"), (dict(S=0), b"S=0"), (dict(S=33), b"S=33")]
    for over, words in sizes:
        # a bad size wins over every later argument and over null and misaligned pointers
        refused(words, _desc(frames=None, offset=ONE + 4, **over), M=-1, K=0, tokens=None)
    refused(b"M=-1", _desc(frames=None), M=-1, G=-1, K=0)
    refused(b"M=2147483648", _desc(frames=None), M=2 ** 31, G=-1)
    refused(b"G=-1", _desc(frames=None), G=-1, K=0)
    refused(b"K=0", _desc(frames=None), K=0, shift=-1)
    refused(b"K=4097", _desc(frames=None), K=4097, shift=-1)
    refused(b"shift=-1", _desc(frames=None), shift=-1, select=2)
    refused(b"shift=65", _desc(frames=None), shift=65, select=2)
    refused(b"select=2", _desc(frames=None), select=2, tokens=None)
    # no lists: a no-op, whatever the pointers are
    assert _add(_desc(frames=None), M=0, starts=None, tokens=None, lengths=None, groups=None, stored=None) == 0
    refused(b"M=4 > G=3 with null groups", _desc(frames=None), M=4, groups=None, tokens=None)
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        refused(b"null buffer array", _desc(**{name: None, "offset" if name != "offset" else "ring": ONE + 4}),
                tokens=None)
    for name, at in (("rewards", ONE + 2), ("length", ONE + 2), ("offset", ONE + 4), ("ring", ONE + 4)):
        refused(b"buffer arrays not aligned", _desc(**{name: at}), tokens=None)
    for name in ("starts", "tokens", "lengths"):
        refused(b"null starts, tokens or lengths", _desc(), **{name: None, "status": ONE + 2})
    for name, at in (("lengths", ONE + 4), ("groups", ONE + 4), ("status", ONE + 2)):
        refused(b"not aligned to their elements", _desc(), **{name: at})


# ---- the restatement against the reference's ring ----------------------------------------------------------------------
def check_snapshot(g, name, a, ring):
    items = [ring.getitem(i) for i in range(len(ring))]
    assert np.array_equal(np.stack([it[0] for it in items]), g[f"{name}_snap{a}_frames"])
    assert np.array_equal(np.array([it[1] for it in items]), g[f"{name}_snap{a}_scalar"])
    assert np.array_equal(np.stack([it[2] for it in items]), g[f"{name}_snap{a}_action"])
    assert np.array_equal(np.array([it[3] for it in items]), g[f"{name}_snap{a}_reward"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_ring(golden, name):
    g = golden("replay_lists_cases")
    starts, tokens, lengths = g[f"{name}_starts"], g[f"{name}_tokens"], g[f"{name}_lengths"]
    A, K = tokens.shape[0], tokens.shape[1]
    assert not g[f"{name}_rank"].any()  # the reference's end reward -get_rank is 0 for every list
    one, many = RR.Ring(3, K), RR.Ring(3, K)
    for a in range(A):
        stored, status = LR.add_lists(one, starts, tokens[a:a + 1], lengths[a:a + 1], groups=[a])
        assert stored.tolist() == [1] and status == 0
        n = int(lengths[a])
        assert np.array_equal(one.slots[(one.pointer - 1) % 3][2], g[f"{name}_rewards"][a, :n])
        if f"{name}_snap{a}_frames" in g:
            check_snapshot(g, name, a, one)
    # all lists in one call: what the sequential adds left (only the last 3 remain, every list reported stored)
    stored, status = LR.add_lists(many, starts, tokens, lengths)
    assert stored.tolist() == [1] * A and status == 0 and IO.rings_equal(many, one)
    check_snapshot(g, name, A - 1, many)
    # the best ring: the first shortest list
    best = RR.Ring(3, K)
    stored, status = LR.add_lists(best, starts, tokens, lengths, select=True)
    first = int(np.argmin(lengths))
    assert stored.tolist() == [int(m == first) for m in range(A)] and best.added == 1
    assert np.array_equal(best.slots[0][1], tokens[first, :int(lengths[first])])


def random_lists(rng, S, T, K, M, G, shift):
    """Solvable by construction: the target of a group is the sum of its list's terms; history frames are random."""
    tokens = rng.integers(0, 3, size=(M, K, 3 * S)).astype(np.int8) + np.int8(shift - 1)
    lengths = rng.integers(1, K + 1, size=M).astype(np.int64)
    starts = rng.integers(-2, 3, size=(G, T, S, S, S)).astype(np.int8)
    for m in range(min(M, G)):
        starts[m, 0] = -LR.heads_of(np.zeros((S, S, S), np.int32), tokens[m], int(lengths[m]), shift)[-1]
    return starts, tokens, lengths


@pytest.mark.parametrize("select", [False, True])
def test_restatement_equals_replay_add_on_the_padded_form(select):
    """The equivalence clause: the valid lists, as padded states, one-hot policies and rewards, through replay_ref's
    restatement of tg_replay_add."""
    rng = np.random.default_rng(5)
    for S, T, K, shift in ((2, 1, 3, 1), (3, 2, 4, 2), (2, 4, 2, 1)):
        M = G = 7
        starts, tokens, lengths = random_lists(rng, S, T, K, M, G, shift)
        lengths[2] = 0                    # a bad length
        tokens[4, 0, 0] += 1              # no longer ends at zero
        groups = np.arange(M)
        groups[5] = G                     # a bad group
        ring, padded = RR.Ring(3, K + 1), RR.Ring(3, K + 1)
        stored, status = LR.add_lists(ring, starts, tokens, lengths, groups=groups, shift=shift, select=select)
        assert status & LR.BAD_LENGTH and status & LR.BAD_GROUP and status & LR.NOT_ZERO
        valid = np.array([m not in (2, 4, 5) for m in range(M)])
        if not select:
            assert stored.tolist() == valid.astype(int).tolist()
        st, po, rw, ln = LR.padded_form(starts, tokens[valid], lengths[valid], groups[valid], K + 1, shift, 3 + shift)
        padded.add(st, po, rw, ln, select=select)
        assert IO.rings_equal(padded, ring) and ring.added == (1 if select else int(valid.sum()))


@pytest.mark.parametrize("entry", RC.ENTRIES)
def test_ring_edge_cases_store_and_reject_in_every_combination(entry):
    """The cases tests/ring_cases.py gives the three GPU files, on the restatement alone: every combination stores at
    least one game and rejects at least one, so none of them passes vacuously on the device."""
    for N in RC.EDGE_N:
        args = RC.edge_case(entry, N)
        valid = N - len(range(3, N, 7))
        for C in RC.EDGE_C:
            for first in RC.edge_starts(C):
                for select in (False, True) if entry != "add_packed" else (False,):
                    ring, status, stored = RC.restate(entry, args, C, first, select)
                    assert status and ring.added == (1 if select else valid), (N, C, first, select)
                    assert len(ring.slots) == min(ring.added, C) and ring.pointer == (first + ring.added) % C
                    assert stored is None or stored.sum() == ring.added


def test_restated_edges():
    S, T, K = 2, 2, 3
    tok = lambda u: np.array([u, 0, 1, 0, 1, 0], np.int8) + 1  # the term u e0 (x) e0 (x) e0, shift 1
    starts = np.zeros((4, T, S, S, S), np.int8)
    starts[0, 0, 0, 0, 0] = 2       # two moves of e0 end at zero
    starts[1, 0, 0, 0, 0] = -128    # see below
    starts[2, 0, 0, 0, 0] = 1       # one move of e0
    starts[3, 0, 0, 0, 1] = 1       # one entry that no move of e0 reaches
    tokens = np.zeros((5, K, 3 * S), np.int8)
    tokens[0, :2] = tok(1)
    tokens[1] = tok(1), tok(-1), tok(-128)  # -129 (outside int8), -128, 0: leaves int8 and comes back
    tokens[2, 0] = tokens[3, 0] = tokens[4, 0] = tok(1)
    ring = RR.Ring(4, 2)
    stored, status = LR.add_lists(ring, starts, tokens, [2, 3, 1, 1, 3], groups=[0, 1, 2, 3, 0])
    # lists 1 and 4: length 3 > the ring's L (not replayed); list 3 ends one entry away from zero
    assert stored.tolist() == [1, 0, 1, 0, 0] and status == LR.BAD_LENGTH | LR.NOT_ZERO
    assert ring.slots[0][0][:, :, 0, 0, 0].tolist() == [[2, 0], [1, 2]] and ring.slots[0][2].tolist() == [-1, -2]
    flags, heads = LR.list_flags(starts, tokens[1], 3, 1, K, 3, 1)
    assert heads[1:, 0, 0, 0].tolist() == [-129, -128, 0] and flags == LR.BAD_RANGE
    starts[1, 0, 0, 0, 0] = 127
    tokens[1] = tok(-1), tok(-128), tok(0)  # 128 then 256: an int8 stepper wraps 256 to 0, the exact replay does not
    flags, heads = LR.list_flags(starts, tokens[1], 3, 1, K, 3, 1)
    assert heads[1:, 0, 0, 0].tolist() == [128, 256, 256] and flags == LR.BAD_RANGE | LR.NOT_ZERO
    assert LR.list_flags(starts, tokens[1], 0, 4, K, 3, 1)[0] == LR.BAD_LENGTH | LR.BAD_GROUP
