"""GPU checks of the canonical form modulo a symmetry group: ``tg_orbit_canon`` and ``tg_orbit_fixes`` bit for bit
against the host restatement (tests/orbits_ref.py) on guarded, unaligned arrays, with and without the workspace that
spreads the group over workgroups; the matmul groups, odd sizes, the 256-thread path, the row limit, degenerate lists,
the three kinds of bad row; ``SymmetryGroup`` on the device; and ``SolutionArchive(group=)``."""
import functools
import io

import numpy as np
import pytest
import torch

from mat_mul_amd import SolutionArchive, SymmetryGroup, _lib, ops
from oracle.tensor_game import build_matmul_tensor

import orbits_ref as OR
import solutions_ref as SR
import symmetry_ref as SY
from guarded_buffers import CANARY, GUARD, check_flat, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("canon", "rank", "key", "residual_nnz", "which", "stab")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy()


def odd(x):
    """A copy of a one-byte-element tensor one byte behind an aligned allocation, canaries around it: (buffer, view)."""
    n = x.numel()
    buf = torch.full((GUARD + 1 + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = buf[GUARD + 1:GUARD + 1 + n].view(x.dtype).view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 1
    return buf, view


def run(targets, tokens, lengths, sym, shift=1, workspace=None):
    """``ops.orbit_canon`` on unaligned inputs into guarded outputs: (numpy outputs in NAMES' order, status)."""
    M, K, A3 = tokens.shape
    _, tok = odd(dev(tokens))
    _, rows = odd(dev(sym))
    tgt = None if targets is None else odd(dev(targets))[1]
    cbuf, canon = odd(torch.zeros((M, K, A3), dtype=torch.int8, device=DEV))
    bufs = {name: guarded((M,), dt) for name, dt in (("rank", torch.int32), ("key", torch.int64), ("which", torch.int32),
                                                     ("stab", torch.int32), ("residual_nnz", torch.int32))}
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.orbit_canon(tgt, tok, dev(np.asarray(lengths, np.int64)), rows, shift=shift, canon=canon, rank=bufs["rank"][1],
                          key=bufs["key"][1], residual_nnz=None if targets is None else bufs["residual_nnz"][1],
                          which=bufs["which"][1], stab=bufs["stab"][1], status=status, workspace=workspace)
    torch.cuda.synchronize()
    n = canon.numel()
    assert bool((cbuf[:GUARD + 1] == CANARY).all()) and bool((cbuf[GUARD + 1 + n:] == CANARY).all()), "canon"
    for name, (buf, _) in bufs.items():
        check_flat(buf, name)
    if targets is None:
        assert out[3] is None and bool((bufs["residual_nnz"][1].view(torch.uint8) == CANARY).all())
    got = [None if o is None else host(o) for o in out]
    got[2] = got[2].view(np.uint64)
    return got, int(status.cpu().view(torch.int32).item())


def check(targets, tokens, lengths, sym, shift=1, want=None):
    """Both decompositions equal the restatement; returns the restatement's outputs."""
    want = want or OR.orbit_canon(targets, tokens, lengths, shift, sym)
    for workspace in (None, False):
        got, status = run(targets, tokens, lengths, sym, shift, workspace)
        for name, a, b in zip(NAMES, got, want[:6]):
            if b is None:
                assert a is None, name
            else:
                assert np.array_equal(a, b), (name, workspace, a, b)
        assert status == want[6], (status, want[6], workspace)
    return want


@functools.lru_cache(maxsize=None)
def matmul_group(n, signs):
    return SymmetryGroup.matmul(n, DEV, signs=signs)


@functools.lru_cache(maxsize=None)
def generated_group(S, seed):
    """The closure of two random signed-permutation generators: one with a mode permutation, index permutations and
    signs, one with signs alone (seeds with a closure of 32 to 128 elements: two unrestricted elements generate far
    more than TG_ORBIT_MAX_G)."""
    gens = np.stack([SY.sample(1, S, seed, 0)[0], SY.sample(1, S, seed, 1, SY.SIGNS)[0]])
    return SymmetryGroup.generate(gens, S, DEV)


def strassen(golden, K=8):
    g = golden("strassen")
    tokens = np.zeros((K, 12), dtype=np.int8)
    tokens[:7] = g["tokens"]
    return g["tensor"].astype(np.int8), tokens


# ---- tg_orbit_canon --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signs, picks", [(False, (17, 29)), (True, (5, 17))])
def test_s4_strassen_its_images_and_an_unproven_list(golden, signs, picks):
    S, K, shift = 4, 8, 1
    grp = matmul_group(2, signs)
    assert grp.order == (1536 if signs else 48)
    T, tok = strassen(golden, K)
    rng = np.random.default_rng(3)
    tokens = np.stack([tok] + [OR.act_tokens(tok, 7, SY.decode(grp.rows[h], S), S, shift) for h in picks]
                      + [SR.random_lists(rng, 1, K, S, shift, [6])[0][0]])
    lengths = np.array([7, 7, 7, 6])
    targets = np.broadcast_to(T, (4, S, S, S)).copy()
    canon, rank, key, res, which, stab, status = check(targets, tokens, lengths, grp.rows)
    assert status == 0 and res[:3].tolist() == [0, 0, 0] and res[3] > 0 and rank[:3].tolist() == [7, 7, 7]
    assert key[0] == key[1] == key[2] != key[3] and np.array_equal(canon[0], canon[1]) and np.array_equal(canon[0], canon[2])
    assert len(set(which[:3].tolist())) == 3 and stab[0] == stab[1] == stab[2] and grp.order % int(stab[0]) == 0
    plain = ops.solution_canon(dev(targets), dev(tokens), dev(lengths))
    assert len(set(host(plain[2])[:3].tolist())) == 3 and host(plain[3])[:3].tolist() == [0, 0, 0]
    assert np.array_equal(SR.term_sum(canon[0], 7, S, shift), T)                  # the orbit form is a proof of T still
    if signs:                                                                     # the transversal: same form, stab / 4
        tr = grp.modulo_term_signs()
        c2, r2, k2, n2, w2, s2, st2 = check(targets, tokens, lengths, tr.rows)
        assert tr.order == 384 and np.array_equal(c2, canon) and np.array_equal(k2, key) and np.array_equal(r2, rank)
        assert np.array_equal(4 * s2, stab) and np.array_equal(tr.rows[w2], grp.rows[which])


def test_s9_with_the_1296_element_group():
    S, K, shift = 9, 6, 1
    grp = matmul_group(3, False)
    assert grp.order == 1296
    rng = np.random.default_rng(99)
    targets, tokens, lengths = OR.proven_lists(rng, 2, K, S, shift, 4)
    canon, rank, key, res, which, stab, status = check(targets, tokens, lengths, grp.rows)
    assert status == 0 and res.tolist() == [0, 0] and (rank > 0).all() and (stab >= 1).all()


def test_the_256_thread_path_at_k_65():
    S, K, shift = 2, 65, 1
    grp = generated_group(S, 4)
    assert grp.order == 32
    rng = np.random.default_rng(65)
    tokens, lengths = SR.random_lists(rng, 3, K, S, shift, [65, 0, 31])
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    canon, rank, key, res, which, stab, status = check(targets, tokens, lengths, grp.rows)
    assert status == 0 and rank[0] > 0 and rank[1] == 0 and which[1] == 0 and stab[1] == 32


@pytest.mark.parametrize("S, seed, order", [(3, 17, 64), (5, 7, 64), (7, 7, 128)])
def test_odd_sizes_with_generated_groups(S, seed, order):
    K, shift = 7, 1
    grp = generated_group(S, seed)
    assert grp.order == order and grp.closed()
    rng = np.random.default_rng(S)
    tokens, lengths = SR.random_lists(rng, 5, K, S, shift, [7, 0, 3, 5, 6])
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    want = check(targets, tokens, lengths, grp.rows)
    assert want[6] == 0 and len(set(want[4].tolist())) > 1
    got, status = run(None, tokens, lengths, grp.rows, shift)                     # without targets: no verification
    assert status == 0 and got[3] is None
    for name, a, b in zip(NAMES, got, want[:6]):
        assert name == "residual_nnz" or np.array_equal(a, b), name
    # invariance: every list moved by an element of the group has the same form
    h = SY.decode(grp.rows[order // 3], S)
    moved = np.stack([OR.act_tokens(tokens[m], int(lengths[m]), h, S, shift) for m in range(5)])
    got, status = run(None, moved, lengths, grp.rows, shift)
    assert status == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[5], want[5])


def test_the_row_limit_k_256_at_s_32():
    """K * 3S = TG_ORBIT_MAX_ROW: 96 KiB of dynamic LDS, above the 64 KiB a kernel has without the opt-in."""
    S, K, shift = 32, 256, 1
    assert K * 3 * S == _lib.TG_ORBIT_MAX_ROW
    rng = np.random.default_rng(256)
    tokens, lengths = SR.random_lists(rng, 2, K, S, shift, [256, 77])
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    sym = np.concatenate([SY.sample(1, S, 5), SY.identity(1, S)])
    want = check(targets, tokens, lengths, sym)
    assert want[6] == 0 and want[1][0] > 128 and want[1][1] > 0


@pytest.mark.parametrize("S, K", [(4, 7), (9, 65)])
def test_identity_alone_equals_solution_canon(S, K):
    shift, M = 1, 21 if S == 4 else 4
    rng = np.random.default_rng(1000 * S + K)
    tokens, lengths = SR.random_lists(rng, M, K, S, shift)
    targets = SR.targets_for(rng, tokens, lengths, S, shift)
    plain = ops.solution_canon(dev(targets), dev(tokens), dev(lengths), shift=shift)
    for workspace in (None, False):
        got, status = run(targets, tokens, lengths, SY.identity(1, S), shift, workspace)
        assert status == 0
        for name, a, b in zip(NAMES[:4], got, plain):
            assert np.array_equal(a.view(np.int64) if name == "key" else a, host(b)), name
        assert (got[4] == 0).all() and (got[5] == 1).all()
    got, _ = run(None, tokens, lengths, SY.identity(1, S), shift)
    assert np.array_equal(got[0], host(plain[0])) and np.array_equal(got[2].view(np.int64), host(plain[2]))


def test_empty_null_and_cancelling_lists(golden):
    S, K, shift = 4, 8, 1
    grp = matmul_group(2, False)
    T, tok = strassen(golden, K)
    tokens = np.stack([tok, tok, tok, tok])
    lengths = np.array([0, 3, 4, 7])
    tokens[1, :3, 4:8] = shift                                                    # v = 0: three null terms
    tokens[2, 2] = tokens[2, 0]                                                   # terms 0, 1 and their negatives
    tokens[2, 3] = tokens[2, 1]
    tokens[2, 2, :4] = 2 * shift - tokens[2, 2, :4]
    tokens[2, 3, 8:] = 2 * shift - tokens[2, 3, 8:]
    targets = np.broadcast_to(T, (4, S, S, S)).copy()
    canon, rank, key, res, which, stab, status = check(targets, tokens, lengths, grp.rows)
    assert status == 0 and rank.tolist() == [0, 0, 0, 7] and key[:3].tolist() == [0, 0, 0] and not canon[:3].any()
    assert which[:3].tolist() == [0, 0, 0] and stab[:3].tolist() == [48, 48, 48] and res[:3].tolist() == [8, 8, 8]
    assert res[3] == 0


def test_bad_lengths_negations_and_neighbours():
    S, K, shift = 2, 5, 0
    rng = np.random.default_rng(7)
    tokens, lengths = SR.random_lists(rng, 6, K, S, shift, [3, 0, 4, 0, 2, 5])
    lengths[[1, 3]] = -1, K + 1
    targets = SR.targets_for(rng, tokens, np.clip(lengths, 0, K), S, shift)
    grp = generated_group(S, 4)
    want = check(targets, tokens, lengths, grp.rows, shift)
    assert want[6] == OR.BAD_LENGTH and want[4].tolist()[1] == want[4].tolist()[3] == -1 and (want[4][[0, 2, 4, 5]] >= 0).all()
    # the asymmetric vocabulary of shift 0: 127 has a negative, -128 has none
    ident = SY.identity(1, S)
    flip = ident.copy()
    flip[0, 1] |= 0x80
    tokens[2, 0] = [-128, 1, 1, 0, 1, 0]                                          # -u holds 128 for the identity already
    tokens[4, 0] = [127, -128, 1, 0, 1, 0]                                        # fine as it is; flipped, u = (-127, -128)
    tokens[5, 1] = [-1, 0, 1, 0, 1, -128]                                         # sigma = -1 alone in its run: -w holds 128
    tokens[5, 2] = [-128, 1, 0, 0, 1, 0]                                          # a null term: dropped before any negation
    plain = check(targets, tokens, lengths, ident, shift)
    assert plain[6] == OR.BAD_LENGTH | OR.BAD_NEGATION and plain[4].tolist() == [0, -1, -1, -1, 0, -1]
    both = check(targets, tokens, lengths, np.concatenate([ident, flip]), shift)
    assert both[4].tolist()[1:] == [-1] * 5 and both[4][0] >= 0 and both[3][4] == -1 and both[5][4] == 0
    good = OR.orbit_canon(targets[:1], tokens[:1], lengths[:1], shift, np.concatenate([ident, flip]))
    for a, b in zip(both[:6], good[:6]):                                          # the good list, as if it were alone
        assert np.array_equal(a[:1], b)
    with pytest.raises(_lib.TensorGameError, match="sym"):
        ops.orbit_canon(None, dev(tokens), dev(lengths), dev(ident[:, :-1]))
    with pytest.raises(_lib.TensorGameError, match="G=2049"):
        ops.orbit_canon(None, dev(tokens), dev(lengths), dev(np.tile(ident, (2049, 1))))
    with pytest.raises(_lib.TensorGameError, match="workspace"):
        ops.orbit_canon(None, dev(tokens[:1]), dev(lengths[:1]), dev(np.tile(ident, (64, 1))),
                        workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("at", [0, 31, 17])
def test_a_bad_group_row_makes_every_list_bad(at):
    S, K, shift = 2, 5, 1
    rng = np.random.default_rng(at)
    tokens, lengths = SR.random_lists(rng, 4, K, S, shift, [3, 5, 0, 2])
    lengths[3] = K + 1
    targets = SR.targets_for(rng, tokens, np.clip(lengths, 0, K), S, shift)
    rows = generated_group(S, 4).rows.copy()
    if at == 17:
        rows[at, 3] = (rows[at, 3] & 0x80) | S                                    # an index >= S
    else:
        rows[at, 0] = 6                                                           # a mode code above 5
    want = check(targets, tokens, lengths, rows, shift)
    assert want[6] == OR.BAD_GROUP | OR.BAD_LENGTH and not want[0].any() and (want[4] == -1).all()
    assert (want[5] == 0).all() and (want[3] == -1).all() and (want[1] == 0).all() and (want[2] == 0).all()
    fixes, status = ops.orbit_fixes(dev(targets), dev(rows)), torch.zeros(1, dtype=torch.uint32, device=DEV)
    assert not bool(fixes.any())
    ops.orbit_fixes(dev(targets), dev(rows), status=status)
    assert int(status.cpu().view(torch.int32).item()) == 1


def test_a_list_alone_and_inside_a_batch_of_300(golden):
    """What a sliced decomposition can get wrong: the same list through different cuts of the group (alone: many
    slices; among 300: few; without workspace: none) has the same outputs."""
    S, K, shift = 4, 8, 1
    grp = matmul_group(2, True)
    T, tok = strassen(golden, K)
    rng = np.random.default_rng(300)
    tokens, lengths = SR.random_lists(rng, 300, K, S, shift)
    tokens[137], lengths[137] = OR.act_tokens(tok, 7, SY.decode(grp.rows[1000], S), S, shift), 7
    targets = np.broadcast_to(T, (300, S, S, S)).copy()
    sizes = [ops.orbit_workspace_size(M, K, S, grp.order) for M in (1, 300)]
    assert sizes[0] > 0 and sizes[1] > 0 and sizes[0] // 1 != sizes[1] // 300       # two different cuts
    alone = check(targets[137:138], tokens[137:138], lengths[137:138], grp.rows)
    assert alone[3][0] == 0 and alone[1][0] == 7 and alone[5][0] == 48
    for workspace in (None, False):
        got, status = run(targets, tokens, lengths, grp.rows, shift, workspace)
        assert status == 0
        for name, a, b in zip(NAMES, got, alone[:6]):
            assert np.array_equal(a[137:138], b), (name, workspace)
        if workspace is None:
            first = got
        else:
            for name, a, b in zip(NAMES, got, first):
                assert np.array_equal(a, b), name


# ---- tg_orbit_fixes and SymmetryGroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("n, signs", [(2, True), (3, False)])
def test_fixes_equals_symmetry_apply_per_element(n, signs):
    S = n * n
    grp = matmul_group(n, signs)
    T = build_matmul_tensor(1, n, n, n)[0].astype(np.int8)
    rng = np.random.default_rng(n)
    targets = np.stack([T, rng.integers(-2, 3, size=(S, S, S)).astype(np.int8), (3 * T).astype(np.int8), T])
    targets[3, 0, 0, 0] += 1                                                      # one entry off
    fbuf, fixes = guarded((4,), torch.uint8)
    status = torch.zeros(1, dtype=torch.uint32, device=DEV)
    out = ops.orbit_fixes(odd(dev(targets))[1], odd(grp.sym)[1], fixes=fixes, status=status)
    assert out is fixes and host(fixes).tolist() == [1, 0, 1, 0] == OR.fixes(targets, grp.rows)[0].tolist()
    check_flat(fbuf, "fixes")
    assert int(status.cpu().view(torch.int32).item()) == 0
    assert host(grp.fixes(dev(targets))).tolist() == [True, False, True, False]
    for m in range(4):                                                            # the definition, element by element
        frames = dev(np.broadcast_to(targets[m], (grp.order, 1, S, S, S)).copy())
        moved, _ = ops.symmetry_apply(frames, None, grp.sym, dtype=torch.int8)
        assert bool((moved == frames).flatten(1).all(1).all()) == bool(fixes[m])


def test_fixes_compares_in_32_bits():
    """s * T[b] == T[a] with T[b] = -128 and s = -1: 128 in int32, not the -128 an int8 negation wraps to."""
    sym = SY.identity(2, 1)
    sym[1, 1] |= 0x80                                                             # mode 0 negated: every entry changes sign
    targets = np.array([-128, 0, 5], dtype=np.int8).reshape(3, 1, 1, 1)
    assert host(ops.orbit_fixes(dev(targets), dev(sym))).tolist() == [0, 1, 0] == OR.fixes(targets, sym)[0].tolist()
    wrapped, _ = ops.symmetry_apply(dev(targets[:1, None]), None, dev(sym[1:]), dtype=torch.int8)
    assert int(wrapped.flatten()[0]) == -128                                      # what the int8 comparison would see
    big = np.full((2, 32, 32, 32), -128, dtype=np.int8)                           # the largest size, -128 everywhere
    big[1, 31, 31, 31] = 127
    perm = SY.sample(3, 32, 9, 0, SY.MODES | SY.PERMS)
    assert host(ops.orbit_fixes(dev(big), dev(perm))).tolist() == [1, 0] == OR.fixes(big, perm)[0].tolist()


def test_symmetry_group_on_the_device():
    grp = matmul_group(2, True)
    assert grp.sym.device == torch.device(DEV) and grp.sym.dtype == torch.uint8 and tuple(grp.sym.shape) == (1536, 13)
    same = SymmetryGroup.from_elements(grp.sym)
    assert np.array_equal(same.rows, grp.rows) and same.sym.device == grp.sym.device
    back = SymmetryGroup.from_state_dict(grp.modulo_term_signs().state_dict(), DEV)
    assert back.order == 384 and (back.overlap == 4).all() and torch.equal(back.sym, grp.modulo_term_signs().sym)
    with pytest.raises(_lib.TensorGameError, match="max_order"):
        SymmetryGroup.matmul(3, DEV, signs=True)


# ---- the archive -----------------------------------------------------------------------------------------------------
def strassen_images(golden, grp, count, seed):
    S, K, shift = 4, 8, 1
    T, tok = strassen(golden, K)
    rng = np.random.default_rng(seed)
    picks = rng.choice(grp.order, size=count, replace=False)
    tokens = np.stack([tok] + [SR.variant(rng, OR.act_tokens(tok, 7, SY.decode(grp.rows[h], S), S, shift), 7, K, S, shift,
                                          pairs=0, nulls=1)[0] for h in picks])
    lengths = np.array([7] + [8] * count)
    return np.broadcast_to(T, (count + 1, S, S, S)).copy(), tokens, lengths


def test_archive_counts_strassen_and_twenty_images_once(golden):
    S, K = 4, 8
    grp = matmul_group(2, True)
    targets, tokens, lengths = strassen_images(golden, grp, 20, 1)
    args = (dev(targets), dev(tokens), dev(lengths))
    plain = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV)
    rep0 = plain.add(*args)
    assert bool(rep0.proven.all()) and int(plain.count) > 1 and rep0.fixed is None and rep0.which is None and rep0.stab is None
    for group in (grp, grp.modulo_term_signs()):
        arch = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV, group=group)
        rep = arch.add(*args)
        assert bool(rep.proven.all()) and bool(rep.fixed.all()) and int(arch.count) == 1 and int(arch.lowest_rank) == 7
        assert host(rep.fresh).tolist() == [True] + [False] * 20 and len(set(host(rep.key).tolist())) == 1
        assert bool((rep.stab == (48 if group is grp else 12)).all()) and len(set(host(rep.which).tolist())) > 1
        etok, erank, ekey, etarget = arch.entries()
        canon, rank, key, res = ops.solution_canon(args[0][:1], etok, torch.full((1,), 7, dtype=torch.int64, device=DEV))
        assert int(res[0]) == 0 and int(rank[0]) == int(erank[0]) == 7            # the stored form re-verifies
        assert torch.equal(canon, etok) and int(ekey[0]) == int(rep.key[0]) and int(etarget[0]) == int(ops.state_hash(args[0][:1])[0])
        want = OR.orbit_canon(targets[:1], tokens[:1], lengths[:1], 1, group.rows)
        assert np.array_equal(host(etok)[0], want[0][0]) and host(ekey).view(np.uint64)[0] == want[2][0]


def test_archive_does_not_store_a_row_whose_target_the_group_does_not_fix(golden):
    S, K = 4, 8
    grp = matmul_group(2, False)
    targets, tokens, lengths = strassen_images(golden, grp, 2, 2)
    rng = np.random.default_rng(8)
    t2, tok2, len2 = OR.proven_lists(rng, 2, K, S, 1, 4)                          # proven, of targets nothing fixes
    targets, tokens, lengths = np.concatenate([targets, t2]), np.concatenate([tokens, tok2]), np.concatenate([lengths, len2])
    arch = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV, group=grp)
    rep = arch.add(dev(targets), dev(tokens), dev(lengths))
    assert host(rep.proven).tolist() == [True] * 5 and host(rep.fixed).tolist() == [True] * 3 + [False] * 2
    assert host(rep.fresh).tolist() == [True, False, False, False, False] and int(arch.count) == 1
    assert int(arch.canon_status.cpu().view(torch.int32).item()) == 0
    with pytest.raises(_lib.TensorGameError, match="S=9"):
        SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV, group=matmul_group(3, False))


def test_archive_state_dict_version_2_round_trip_and_version_1_unchanged(golden):
    S, K = 4, 8
    grp = matmul_group(2, True).modulo_term_signs()
    targets, tokens, lengths = strassen_images(golden, grp, 6, 3)
    rng = np.random.default_rng(4)
    tokens[3], lengths[3] = SR.random_lists(rng, 1, K, S, 1, [5])[0][0], 5        # an unproven row
    args = (dev(targets), dev(tokens), dev(lengths))
    arch = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV, group=grp)
    arch.add(*(x[:3] for x in args))
    blob = io.BytesIO()
    torch.save({"solutions": arch.state_dict()}, blob)
    blob.seek(0)
    sd = torch.load(blob, weights_only=True)["solutions"]
    assert sd["version"] == 2 and sd["group"]["version"] == 1 and tuple(sd["group"]["sym"].shape) == (384, 13)
    back = SolutionArchive.from_state_dict(sd, DEV)
    assert back.group.order == 384 and np.array_equal(back.group.rows, grp.rows) and int(back.count) == 1
    reps = [a.add(*args) for a in (arch, back)]
    for name in ("proven", "rank", "key", "fresh", "residual_nnz", "fixed", "which", "stab"):
        assert torch.equal(getattr(reps[0], name), getattr(reps[1], name)), name
    assert not bool(reps[0].fresh.any()) and int(arch.count) == int(back.count) == 1
    for x, y in zip(arch.entries(), back.entries()):
        assert torch.equal(x, y)
    plain = SolutionArchive(S=S, max_rank=K, capacity=64, device=DEV)
    plain.add(*args)
    sd1 = plain.state_dict()
    assert sd1["version"] == 1 and sorted(sd1) == sorted(["version", "S", "max_rank", "capacity", "shift", "count", "status",
                                                          "lowest_rank", "tokens", "rank", "key", "target_key"])
    again = SolutionArchive.from_state_dict(sd1, DEV)
    assert again.group is None and int(again.count) == int(plain.count) > 1
    with pytest.raises(_lib.TensorGameError, match="version"):
        SolutionArchive.from_state_dict({**sd1, "version": 3}, DEV)
