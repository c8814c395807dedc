"""CPU checks of the canonical form modulo a symmetry group (include/tensor_game_orbits.h): the header and the bindings,
the size checks, ``SymmetryGroup`` on the host (orders, closure, the matmul groups fix their tensors, the transversal),
and the algebra of the restatement (tests/orbits_ref.py): invariance under the group, orbit--stabiliser, equal ranks."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mat_mul_amd
from mat_mul_amd import SymmetryGroup, _lib, build, ops
from oracle.tensor_game import build_matmul_tensor

import orbits_ref as OR
import solutions_ref as SR
import symmetry_ref as SY

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_orbits.h"
ENTRIES = ["tg_orbit_canon", "tg_orbit_check", "tg_orbit_fixes", "tg_orbit_workspace_size"]


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_orbits_header_is_plain_c_and_its_symbols_are_bound_and_exported():
    text = HDR.read_text()
    syms = sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", text, flags=re.M)))
    assert syms == ENTRIES == sorted(_lib.ORBIT_SIGNATURES)
    assert not set(syms) & set(_lib.SOLUTION_SIGNATURES) and HDR in build.HEADERS
    for words in ("ORIGINAL", "before it addresses", "rescalings", "smallest index", "REPEAT", "every list is bad"):
        assert words in text, words
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    consts = dict(re.findall(r"#define (TG_ORBIT_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {
        "TG_ORBIT_MAX_G": _lib.TG_ORBIT_MAX_G, "TG_ORBIT_MAX_ROW": _lib.TG_ORBIT_MAX_ROW,
        "TG_ORBIT_BAD_LENGTH": OR.BAD_LENGTH, "TG_ORBIT_BAD_NEGATION": OR.BAD_NEGATION, "TG_ORBIT_BAD_GROUP": OR.BAD_GROUP}
    assert (_lib.TG_ORBIT_BAD_LENGTH, _lib.TG_ORBIT_BAD_NEGATION, _lib.TG_ORBIT_BAD_GROUP) == (1, 2, 4)
    for name in ("orbit_check", "orbit_fixes", "orbit_canon", "orbit_workspace_size"):
        assert name in ops.__all__
    assert "SymmetryGroup" in mat_mul_amd.__all__ and mat_mul_amd.orbits.SymmetryGroup is SymmetryGroup
    gcc = shutil.which("gcc")
    if gcc is not None:
        res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                              "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


@pytest.mark.parametrize("args, words", [
    ((8, 8, 0, 1, 4), "S=0"), ((8, 8, 33, 1, 4), "S=33"), ((8, 0, 4, 1, 4), "K=0"), ((8, 257, 4, 1, 4), "K=257"),
    ((8, 8, 4, -1, 4), "shift=-1"), ((8, 8, 4, 65, 4), "shift=65"), ((-1, 8, 4, 1, 4), "M=-1"),
    ((8, 8, 4, 1, 0), "G=0"), ((8, 8, 4, 1, 2049), "G=2049"),
])
def test_orbit_check_refuses_each_bound(args, words):
    with pytest.raises(_lib.TensorGameError, match=re.escape(words)):
        ops.orbit_check(*args)


def test_orbit_check_row_limit_is_the_whole_range_of_solution_check():
    """The LDS plan holds four images of a row: 96 KiB at K * 3S = 24 576, which K <= 256 and S <= 32 cannot exceed, so
    the limit admits every size tg_solution_check admits (K = 128 at S = 25 and K = 256 at S <= 16 among them)."""
    assert _lib.TG_ORBIT_MAX_ROW == _lib.TG_SOL_MAX_K * 3 * _lib.TG_MAX_S == 24576
    for K, S in ((256, 32), (128, 25), (256, 16), (1, 1)):
        ops.orbit_check(4096, K, S, 64, 2048)
    assert ops.orbit_workspace_size(1 << 20, 8, 4, 1536) == 0          # lists alone fill the device: no slicing
    assert ops.orbit_workspace_size(16, 8, 4, 4) == 0                  # a set too small to slice
    n = ops.orbit_workspace_size(16, 8, 4, 1536)
    assert n > 0 and n % 16 == 0 and n <= 16 * (1536 // 8) * (96 + 32)
    with pytest.raises(_lib.TensorGameError, match="G=0"):
        ops.orbit_workspace_size(16, 8, 4, 0)


def test_orbit_entries_refuse_before_any_launch():
    canon, fixes = _lib.lib.tg_orbit_canon, _lib.lib.tg_orbit_fixes
    p = lambda x: C.c_void_p(x)  # never dereferenced: validation fails first
    ok = dict(targets=p(1), tokens=p(4099), lengths=p(8192), M=4, K=8, S=4, shift=1, sym=p(3), G=48, canon=p(16387),
              rank=p(32768), key=p(65536), res=p(131072), which=p(262144), stab=p(524288), status=None, ws=None, wsb=0)
    order = tuple(ok)
    for over, words in ((dict(tokens=None), b"null tokens"), (dict(lengths=None), b"null lengths"),
                        (dict(sym=None), b"null sym"), (dict(canon=None), b"null canon"), (dict(rank=None), b"null rank"),
                        (dict(key=None), b"null key"), (dict(which=None), b"null which"), (dict(stab=None), b"null stab"),
                        (dict(targets=None), b"residual_nnz needs targets"), (dict(key=p(65540)), b"key not 8-byte"),
                        (dict(which=p(262145)), b"which not 4-byte"), (dict(canon=p(4099)), b"in-place"),
                        (dict(K=257), b"K=257"), (dict(S=33), b"S=33"), (dict(shift=65), b"shift=65"),
                        (dict(M=-1), b"M=-1"), (dict(G=0), b"G=0"), (dict(G=2049), b"G=2049"),
                        (dict(ws=p(24), wsb=1 << 30), b"workspace not 16-byte"),
                        (dict(ws=p(4096), wsb=16), b"workspace_bytes=16")):
        kw = {**ok, **over}
        assert canon(*[kw[k] for k in order], None) == -1 and words in _lib.lib.tg_last_error(), over
    assert canon(*([None] * 3), 0, 8, 4, 1, None, 48, *([None] * 8), 0, None) == 0      # M = 0 returns at once
    for args, words in (((None, 2, 4, p(3), 48, p(5), None), b"null targets"), ((p(1), 2, 4, None, 48, p(5), None), b"null sym"),
                        ((p(1), 2, 4, p(3), 48, None, None), b"null fixes"), ((p(1), 2, 33, p(3), 48, p(5), None), b"S=33"),
                        ((p(1), 2, 4, p(3), 2049, p(5), None), b"G=2049"), ((p(1), -1, 4, p(3), 48, p(5), None), b"M=-1")):
        assert fixes(*args, None) == -1 and words in _lib.lib.tg_last_error(), words
    assert fixes(None, 0, 4, None, 48, None, None, None) == 0
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.orbit_canon(None, torch.zeros((3, 4, 12), dtype=torch.int8), torch.zeros(3, dtype=torch.int64),
                        torch.zeros((1, 13), dtype=torch.uint8))
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        ops.orbit_fixes(torch.zeros((1, 4, 4, 4), dtype=torch.int8), torch.zeros((1, 13), dtype=torch.uint8))


# ---- SymmetryGroup on the host ---------------------------------------------------------------------------------------
GROUPS = {}


def group(n, signs):
    if (n, signs) not in GROUPS:
        GROUPS[n, signs] = SymmetryGroup.matmul(n, signs=signs)
    return GROUPS[n, signs]


@pytest.mark.parametrize("n, signs, order", [(2, False, 48), (2, True, 1536), (3, False, 1296)])
def test_matmul_group_orders_closure_and_every_element_fixes_the_tensor(n, signs, order):
    g = group(n, signs)
    S = n * n
    assert g.order == order and g.S == S and g.rows.shape == (order, 3 * S + 1) and g.rows.dtype == np.uint8
    assert np.array_equal(g.rows[0], SY.identity(1, S)[0])                        # the identity comes first
    assert len({r.tobytes() for r in g.rows}) == order
    T = build_matmul_tensor(1, n, n, n)[0].astype(np.int8)
    for i in range(0, order, 256):                                                # symmetry_ref's own formula
        rows = g.rows[i:i + 256]
        out, _, over, status = SY.apply(np.broadcast_to(T, (len(rows), S, S, S)), None, rows)
        assert status == 0 and not over.any() and (out == T[None]).all()
    assert OR.fixes(T[None], g.rows) == (np.ones(1, np.uint8), 0)
    assert g.closed()
    less = SymmetryGroup.from_elements(np.delete(g.rows, order // 2, axis=0))
    assert less.order == order - 1 and not less.closed()
    sd = g.state_dict()
    back = SymmetryGroup.from_state_dict(sd)
    assert np.array_equal(back.rows, g.rows) and sd["version"] == 1 and sd["sym"].dtype == torch.uint8


def test_the_six_mode_elements_are_in_the_group():
    n, S = 2, 4
    ident, tr = np.arange(S), np.array([0, 2, 1, 3])
    one = np.ones((3, S), np.int64)
    have = {r.tobytes() for r in group(2, False).rows}
    for rho, pis in (((0, 1, 2), (ident, ident, ident)), ((0, 2, 1), (tr, ident, ident)), ((1, 0, 2), (tr, tr, tr)),
                     ((1, 2, 0), (ident, tr, tr)), ((2, 0, 1), (tr, ident, tr)), ((2, 1, 0), (ident, tr, ident))):
        assert SY.encode(rho, np.stack(pis), one).tobytes() in have, rho


def test_matmul_3_with_signs_and_other_oversized_closures_are_refused():
    with pytest.raises(_lib.TensorGameError, match="max_order=2048"):
        SymmetryGroup.matmul(3, signs=True)
    with pytest.raises(_lib.TensorGameError, match="max_order=47"):
        SymmetryGroup.generate(group(2, False).rows[1:6], 4, max_order=47)
    assert SymmetryGroup.generate(np.empty((0, 13), np.uint8), 4).order == 1      # the identity alone


def test_from_elements_validates_on_the_host():
    rows = group(2, True).rows[:5].copy()
    for at, value, words in ((0, 6, "row 2: mode code"), (3, 4, "row 2: index >= S"), (3, 0x84, "row 2: index >= S")):
        bad = rows.copy()
        bad[2, at] = value
        with pytest.raises(_lib.TensorGameError, match=words):
            SymmetryGroup.from_elements(bad)
    twice = rows.copy()
    twice[1, 1:5] = [0, 0, 1, 2]
    with pytest.raises(_lib.TensorGameError, match="row 1: an index repeats"):
        SymmetryGroup.from_elements(twice)
    with pytest.raises(_lib.TensorGameError, match="G=2049"):
        SymmetryGroup.from_elements(np.tile(rows[:1], (2049, 1)))
    with pytest.raises(_lib.TensorGameError, match="without a device"):
        SymmetryGroup.from_elements(rows).sym


def test_modulo_term_signs_is_a_transversal_of_384_classes():
    g = group(2, True)
    t = g.modulo_term_signs()
    assert t.order == 384 and (t.overlap == 4).all() and not t.closed()
    assert np.array_equal(t.rows[0], g.rows[0])
    # every element of the group is a transversal element times one of the four constant-sign elements
    S = 4
    eps = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
    covered = set()
    for e in eps:
        rows = t.rows.copy()
        flip = np.repeat(np.array(e) < 0, S)
        rows[:, 1:] ^= np.where(flip, 0x80, 0).astype(np.uint8)[None]
        covered |= {r.tobytes() for r in rows}
    assert covered == {r.tobytes() for r in g.rows}
    plain = group(2, False).modulo_term_signs()                                   # no signs: every class is one element
    assert plain.order == 48 and (plain.overlap == 1).all()


# ---- the restatement's algebra ---------------------------------------------------------------------------------------
def strassen(golden, K=8):
    g = golden("strassen")
    tokens = np.zeros((K, 12), dtype=np.int8)
    tokens[:7] = g["tokens"]
    return g["tensor"].astype(np.int8), tokens, 7


def lists_s4(golden):
    """Strassen and two random proven lists at S = 4 (their targets are not fixed by the group: the algebra of the
    restatement does not need that)."""
    rng = np.random.default_rng(20261020)
    targets, tokens, lengths = OR.proven_lists(rng, 2, 8, 4, 1, 5)
    T, tok, L = strassen(golden)
    return [(T, tok, L)] + [(targets[m], tokens[m], int(lengths[m])) for m in range(2)]


def test_orbit_form_is_invariant_under_every_element_and_orbit_stabiliser_holds(golden):
    """Over the 48-element group, for EVERY h: orbit_canon(h.X) == orbit_canon(X); (distinct C_g) * stab == |G|; the
    rank is the same for every g.  (The 1 536-element group has 2.4 million pairs (g, h): it is checked below on a
    sample of h.)"""
    S, shift, grp = 4, 1, group(2, False)
    elems = [SY.decode(r, S) for r in grp.rows]
    for T, tok, L in lists_s4(golden):
        cn, rank, key, res, which, stab, bits, forms = OR.orbit_row(T, tok, L, S, shift, elems, want_forms=True)
        assert bits == 0 and res == 0 and len(forms) == 48
        assert len({k for k, _ in forms}) * stab == 48 and {r for _, r in forms} == {rank}
        for h in elems:
            moved = OR.act_tokens(tok, L, h, S, shift)
            c2, r2, k2, _, w2, s2, b2 = OR.orbit_row(None, moved, L, S, shift, elems)
            assert b2 == 0 and np.array_equal(c2, cn) and (r2, k2, s2) == (rank, key, stab)


def test_strassen_under_the_full_group_and_its_transversal(golden):
    S, shift = 4, 1
    grp = group(2, True)
    tr = grp.modulo_term_signs()
    T, tok, L = strassen(golden)
    elems, telems = [SY.decode(r, S) for r in grp.rows], [SY.decode(r, S) for r in tr.rows]
    cn, rank, key, res, which, stab, bits, forms = OR.orbit_row(T, tok, L, S, shift, elems, want_forms=True)
    assert (bits, res, rank) == (0, 0, 7) and len({k for k, _ in forms}) * stab == 1536
    assert np.array_equal(SR.term_sum(cn, rank, S, shift), T)                     # the group fixes T: still a proof
    c3, r3, k3, _, w3, s3, b3 = OR.orbit_row(T, tok, L, S, shift, telems)
    assert b3 == 0 and np.array_equal(c3, cn) and (r3, k3) == (rank, key) and 4 * s3 == stab
    assert np.array_equal(tr.rows[w3], grp.rows[which])                           # both name the first class that attains it
    plain = {SR.canon_row(T, OR.act_tokens(tok, L, h, S, shift), L, S, shift)[2] for h in elems[:64]}
    assert len(plain) > 1                                                         # the plain keys tell the images apart
    rng = np.random.default_rng(5)
    for h in rng.choice(1536, size=6, replace=False):
        moved = OR.act_tokens(tok, L, elems[h], S, shift)
        c2, r2, k2, n2, w2, s2, b2 = OR.orbit_row(T, moved, L, S, shift, elems)
        assert b2 == 0 and n2 == 0 and np.array_equal(c2, cn) and (r2, k2, s2) == (rank, key, stab)


def test_restatement_bad_rows_and_identity():
    S, K, shift = 2, 5, 0
    rng = np.random.default_rng(7)
    tokens, lengths = SR.random_lists(rng, 4, K, S, shift, [3, 0, 4, 2])
    lengths[1] = K + 1
    targets = SR.targets_for(rng, tokens, np.clip(lengths, 0, K), S, shift)
    ident = SY.identity(1, S)
    want = SR.canon(targets, tokens, lengths, shift)
    got = OR.orbit_canon(targets, tokens, lengths, shift, ident)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(a, b)
    assert got[6] == want[4] == OR.BAD_LENGTH and got[4].tolist() == [0, -1, 0, 0] and got[5].tolist() == [1, 0, 1, 1]
    # a sign flip of position 0 of mode 0 turns the token 127 (shift 0) into -127: fine; -128 into 128: bit 1
    flip = ident.copy()
    flip[0, 1] |= 0x80
    tokens[2, 0] = [-128, 1, 1, 0, 1, 0]                                          # plain: -u holds 128, bad already
    tokens[3, 0] = [127, -128, 1, 0, 1, 0]                                        # plain: fine; flipped: u = (-127, -128) -> 128
    plain = OR.orbit_canon(targets, tokens, lengths, shift, ident)
    assert plain[6] == OR.BAD_LENGTH | OR.BAD_NEGATION and plain[4].tolist() == [0, -1, -1, 0]
    both = OR.orbit_canon(targets, tokens, lengths, shift, np.concatenate([ident, flip]))
    assert both[6] == OR.BAD_LENGTH | OR.BAD_NEGATION and both[4].tolist()[1:] == [-1, -1, -1] and both[3][3] == -1
    # a bad row of the set: every list is bad, bit 2; the other bits are decided as before
    broken = np.concatenate([ident, ident])
    broken[1, 0] = 6
    out = OR.orbit_canon(targets, tokens, lengths, shift, broken)
    assert out[6] == OR.BAD_GROUP | OR.BAD_LENGTH | OR.BAD_NEGATION
    assert not out[0].any() and not out[1].any() and (out[4] == -1).all() and (out[5] == 0).all() and (out[3] == -1).all()
