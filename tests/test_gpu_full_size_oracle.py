"""Kernel variants that the library selects by batch size or footprint alone, run at a batch that selects each of them
and compared in FULL with an independent CPU reference: the C oracle (oracle/c_oracle.py) for states, flags, children
and keys, numpy for nnz and ``seen``, the exact rank and change of basis on a sample that includes the last grid-stride
round and the last game.  The small-batch suite forces these variants through the A/B library; this module checks the
exact launches the product makes.

Inputs are adversarial, not demo replays: random states in {-2..2} and tokens in {0,1,2}, with terminal, overflowing,
full-range-token, null-action, int8-edge and (S=4) large-L1 games planted in game 0, the last game, on both sides of
every workgroup / unit / grid-stride boundary near the start and end of the batch, and sparsely elsewhere.  Every output
buffer has guard bytes around it (and between games).

SIZES is the table each case's batch was built from; test_kernel_thresholds_cpu.py pins the thresholds in the HIP
sources it rests on.  Every case asserts that its footprint lies in the band the source names, so a case cannot slide
silently onto another variant.

Wall time on one MI355X: 19.3 s for the 39 cases, most of it the oracle and the device-to-host copies; the largest
case (1.25 GiB of S=16 states, stepped twice) takes 2.5 s.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from guarded_buffers import check_flat, check_states, guarded, guarded_states
from mat_mul_amd import ops
from mat_mul_amd._lib import call
from oracle import tensor_game as O
from oracle.c_oracle import COracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MiB = 1 << 20
RAGGED = 37          # added to every smallest selecting batch: not a multiple of any workgroup, unit or grid cap
CHUNK = 64 * MiB     # bytes of games per device-to-host copy and oracle call

# name -> (S, band of the selecting footprint in bytes [lo, hi) or of the batch in games, what the footprint counts).
# The thresholds are constants of mat_mul_amd/csrc (pinned by tests/test_kernel_thresholds_cpu.py).
INF = 1 << 62
SIZES = {
    # tg_step_i8 (states bytes = B * stride)
    "step_s4_plain_one_way": (4, (0, 16 * MiB + 1), "states"),           # plain loads, sweep in one direction (<= 16 MiB)
    "step_s4_plain_reversed": (4, (16 * MiB + 1, 96 * MiB), "states"),   # plain loads, alternating sweep (> 16 MiB)
    "step_s4_nt_loads": (4, (96 * MiB, 384 * MiB), "states"),            # non-temporal loads (96 MiB .. kS4TokenWaitBytes)
    "step_s4_token_wait": (4, (384 * MiB, INF), "states"),               # token awaited first (kS4TokenWaitBytes ..)
    "step_s16_lines": (16, (96 * MiB, 320 * MiB), "states"),             # whole-line stores (96 MiB .. kNtLoadsFromBytes)
    "step_s16_nt_loads": (16, (320 * MiB, 1280 * MiB), "states"),        # [kNtLoadsFromBytes, kNtLoadsToBytes)
    "step_s16_lds_pad": (16, (1280 * MiB, INF), "states"),               # kS16LdsPad: occupancy held down
    "step_s25_lines": (25, (96 * MiB, 320 * MiB), "states"),
    "step_s25_nt_loads": (25, (320 * MiB, 1280 * MiB), "states"),
    "step_s25_lds_pad": (25, (1280 * MiB, INF), "states"),               # kS25LdsPad, plain stores again
    "step_s9_streaming": (9, (96 * MiB, INF), "states"),                 # s9_step_kernel beyond the L2s and the cache
    # tg_step_tracked_i8
    "tracked_s16_crossover": (16, (12000, INF), "games"),                # TensorGameEnv.TRACKED_FROM[16]
    "tracked_s16_beyond_caches": (16, (320 * MiB, INF), "states"),
    "tracked_s25_sparse": (25, (2048, INF), "games"),                    # kTrackedSparse25
    "tracked_s25_sparse_beyond_caches": (25, (320 * MiB, INF), "states"),
    # tg_expand_i8 / tg_expand_keyed_i8 (children bytes = B * k * stride)
    "expand_s4_nt": (4, (128 * MiB, INF), "children"),                   # s4_expand_kernel<true, ..> (kStreamOutBytes)
    "expand_s16_nt": (16, (128 * MiB, INF), "children"),                 # packed_kernel<16, 64, EXPAND, true, ..>
    "expand_s25_keyed": (25, (128 * MiB, INF), "children"),              # keys fused at S=25
    # tg_step_stream_i8 beyond the resident batch (games > tg_step_stream_capacity): rounds, no ready words
    "stream_s4_rounds": (4, ("capacity", INF), "games"),
    "stream_s16_rounds": (16, ("capacity", INF), "games"),
    "stream_s25_rounds": (25, ("capacity", INF), "games"),
    # tg_step_emit: two launches from kStreamOutBytes of model input on (B * T * 64 * 4 bytes, float32)
    "step_emit_s4_two_launches": (4, (128 * MiB, INF), "emit"),
    "step_emit_s16_two_launches": (16, (128 * MiB, INF), "emit"),        # (fused16 below it)
    # grid-capped launches: the batch goes past the cap (later grid-stride rounds run)
    "done_s4_grid_cap": (4, (8192 * 256 // 4 + 1, INF), "games"),        # 8192 blocks, 4 lanes per game
    "done_s16_grid_cap": (16, (8192 * 256 // 64 + 1, INF), "games"),     # 8192 blocks, 64 lanes per game
    "hash_s4_grid_cap": (4, (8192 * 256 // 4 + 1, INF), "games"),        # 8192 blocks
    "seen_grid_cap": (0, (8192 * 256 + 1, INF), "keys"),                 # 8192 blocks of 256 keys
    "rank_s4_grid_cap": (4, (4 * (1 << 20) + 1, INF), "games"),          # 2^20 blocks, 4 games per block
    "rank_s5_grid_cap": (5, ((1 << 20) + 1, INF), "games"),              # 2^20 blocks, a game per block
    "reset_broadcast_s4_grid_cap": (4, (8192 * 256 // 4 + 1, INF), "games"),   # 8192 blocks, 4 chunks per game
    "copy_bytes_grid_cap": (4, (65536 + 1, INF), "games"),               # byte path (unaligned stride): 65 536 blocks
    "copy_s16_nt1": (16, (256 * MiB + 1, 640 * MiB + 1), "both"),        # both buffers > 256 MiB
    "copy_s16_nt2": (16, (640 * MiB + 1, INF), "both"),                  # both buffers > 640 MiB
    "gen_s4_tokens_grid_cap": (4, (16384 * 256 * 16 + 1, INF), "vectors"),   # gen_tokens_kernel<4,16>: 16 384 workgroups
    "gen_s4_basis_grid_cap": (4, (16384 + 1, INF), "games"),             # basis_tokens_kernel<4>: 16 384 workgroups
    # basis_tokens_mfma_kernel<9>: 65 536 workgroups.  Reached only when the fused generator declines: the target's game
    # stride is 744 bytes, not a multiple of 16 (an aligned target with R <= 256 takes gen_fused_kernel instead)
    "gen_s9_basis_grid_cap": (9, (65536 + 1, INF), "games"),
    "change_basis_s16_rounds": (16, ("4 per CU", INF), "games"),          # matrix-core grid: 4 workgroups per CU
}

CO = COracle()


def stride_of(S):
    return -(-S ** 3 // 16) * 16


def first_batch(name, unit_bytes):
    """The smallest batch whose footprint (unit_bytes per game) is inside the entry's band, plus RAGGED."""
    lo = SIZES[name][1][0]
    return -(-lo // unit_bytes) + RAGGED


def assert_in_band(name, footprint):
    lo, hi = SIZES[name][1]
    assert lo <= footprint < hi, f"{name}: footprint {footprint} left its band [{lo}, {hi}) -- move SIZES['{name}']"


def host(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def abi(fn, *args):
    """An entry point of the C ABI called directly, for outputs that the ops wrappers allocate themselves (done / nnz,
    keys, ranks): here they are guarded buffers."""
    with torch.cuda.device(DEV):
        call(fn, *args, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def chunks(B, S):
    step = max(1, CHUNK // stride_of(S))
    for i in range(0, B, step):
        yield i, min(B, i + step)


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def boundaries(B, unit, rounds_at=()):
    """Unit boundaries near the start and the end of the batch, and the first game of every later grid-stride round."""
    out = {unit * i for i in range(1, 9)} | {B - B % unit - unit * i for i in range(0, 9)} | set(rounds_at)
    return sorted(b for b in out if 0 < b < B)


KINDS = ("terminal", "overflow", "wide", "null", "edge", "l1")


def planted_indices(B, bounds, rng, sparse=4096):
    """(indices, kinds): game 0, the last game and both sides of every boundary, their kinds cycling through KINDS in
    that order (deterministic: the pair around the i-th boundary gets kinds 2 + 2i and 3 + 2i), then sparse random games
    of random kinds.  ``kinds`` index KINDS; callers reduce them modulo the kinds they use."""
    fixed = [0, B - 1]
    for b in bounds:
        fixed += [b - 1, b]
    seen, idx = set(), []
    for i in fixed:
        if 0 <= i < B and i not in seen:
            seen.add(i)
            idx.append(i)
    kinds = list(range(len(idx)))
    for i in rng.integers(0, B, size=min(4000, B // sparse)).tolist():
        if i not in seen:
            seen.add(i)
            idx.append(i)
            kinds.append(int(rng.integers(0, len(KINDS))))
    return np.array(idx, np.int64), np.array(kinds, np.int64)


def plant(view, tok, S, bounds, rng, first=lambda t: t[:, 0]):
    """Write the adversarial games at game 0, the last game, both sides of every boundary and sparsely elsewhere
    (planted_indices: every kind in turn on the boundary pairs).
    view: (B,S,S,S) int8 on the device; tok: (B, n, 3S) tokens of each game (n actions: view of the device tensor),
    ``first(tok)`` the action the terminal case aims at.  Returns the planted indices."""
    idx, kinds = planted_indices(view.shape[0], bounds, rng)
    st = host(view[torch.from_numpy(idx).to(DEV)])
    tk = host(tok[torch.from_numpy(idx).to(DEV)])
    kinds = kinds % (len(KINDS) if S == 4 else len(KINDS) - 1)   # (the large-L1 case is S=4's)
    for j, kd in enumerate(kinds):
        kind = KINDS[kd]
        if kind == "terminal":
            st[j] = O.action_to_tensor(first(tk[j:j + 1])[0]).astype(np.int8)
        elif kind == "overflow":
            st[j] = 127
            tk[j, :, :S] = rng.integers(0, 3, size=tk[j, :, :S].shape)
            tk[j, :, 0] = 0                      # u_0 = -1 ...
            tk[j, :, S] = 2                      # ... v_0 = w_0 = 1: entry (0,0,0) becomes 128
            tk[j, :, 2 * S] = 2
        elif kind == "wide":
            tk[j] = rng.integers(-128, 128, size=tk[j].shape)
        elif kind == "null":
            tk[j, :, :S] = 1                     # u == 0: nothing changes
        elif kind == "edge":
            st[j] = rng.choice(np.array([-128, -127, 126, 127, 0], np.int8), size=st[j].shape)
        else:                                    # S=4: whole-game L1 norm above s4_digits_limit
            st[j] = rng.integers(-100, 101, size=st[j].shape)
    it = torch.from_numpy(idx).to(DEV)
    view[it] = torch.from_numpy(st).to(DEV)
    tok[it] = torch.from_numpy(tk).to(DEV)
    return idx


def random_states(B, S, gen, stride=None):
    """guarded (B,S,S,S) buffer of random states in {-2..2}, filled on the device in chunks."""
    stride = stride or stride_of(S)
    buf, view = guarded_states(B, S, stride)
    for i, j in chunks(B, S):
        view[i:j] = torch.randint(-2, 3, (j - i, S, S, S), dtype=torch.int8, device=DEV, generator=gen)
    return buf, view


def random_tokens(shape, gen):
    return torch.randint(0, 3, shape, dtype=torch.int8, device=DEV, generator=gen)


def setup(seed):
    return np.random.default_rng(seed), torch.Generator(device=DEV).manual_seed(seed)


def check_step(src, tok, out, done, ovf, S, what):
    B = src.shape[0]
    for i, j in chunks(B, S):
        w, wd, wo = CO.step_i8(host(src[i:j]), host(tok[i:j]))
        o, d, f = host(out[i:j]), host(done[i:j]), host(ovf[i:j])
        for got, want, field in ((o, w, "state"), (d, wd, "done"), (f, wo, "overflow")):
            if not np.array_equal(got, want):
                bad = i + int(np.nonzero((got != want).reshape(j - i, -1).any(axis=1))[0][0])
                raise AssertionError(f"{what}: {field} differs from the oracle first at game {bad} of {B}")


# ---------------------------------------------------------------------------------------------------------------------
# tg_step_i8


STEP_CASES = [n for n in SIZES if n.startswith("step_s")]


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_variant_by_footprint_matches_oracle(name):
    """One launch per sweep direction (the library alternates them), out of place and then in place, full output against
    the C oracle; guard bytes around the states, between games and around done / overflow."""
    S = SIZES[name][0]
    stride = stride_of(S)
    B = 16 * MiB // stride - 27 if name == "step_s4_plain_one_way" else first_batch(name, stride)
    assert_in_band(name, B * stride)
    rng, gen = setup(zlib.crc32(name.encode()))
    sbuf, src = random_states(B, S, gen)
    tok = random_tokens((B, 3 * S), gen)
    gpb = {4: 64, 9: 16, 16: 4, 25: 1}[S]                       # games per workgroup
    plant(src, tok.view(B, 1, 3 * S), S, boundaries(B, gpb * 8) + boundaries(B, gpb), rng)
    obuf, out = guarded_states(B, S, stride)
    dbuf, done = guarded((B,), torch.uint8)
    fbuf, ovf = guarded((B,), torch.uint8)
    ovf.zero_()
    ops.step(src, tok, out=out, done=done, overflow=ovf)
    free()
    check_states(obuf, B, S, stride, f"{name} out")
    check_flat(dbuf, f"{name} done")
    check_flat(fbuf, f"{name} overflow")
    check_step(src, tok, out, done, ovf, S, name)
    # the other sweep direction, in place: equal to the checked output
    done2 = torch.empty_like(done)
    ovf2 = torch.zeros_like(ovf)
    ops.step(src, tok, out=src, done=done2, overflow=ovf2)
    free()
    check_states(sbuf, B, S, stride, f"{name} in place")
    for i, j in chunks(B, S):
        assert torch.equal(src[i:j], out[i:j]), f"{name}: the second sweep direction differs in games {i}..{j - 1}"
    assert torch.equal(done2, done) and torch.equal(ovf2, ovf), name
    del sbuf, src, obuf, out, tok
    free()


# ---------------------------------------------------------------------------------------------------------------------
# tg_step_tracked_i8


@pytest.mark.parametrize("name", [n for n in SIZES if n.startswith("tracked_")])
def test_step_tracked_at_full_size_matches_oracle(name):
    """Two in-place tracked steps: state, done, overflow and the carried nnz against the oracle and count_nonzero."""
    S = SIZES[name][0]
    stride = stride_of(S)
    B = first_batch(name, 1 if SIZES[name][2] == "games" else stride)
    assert_in_band(name, B if SIZES[name][2] == "games" else B * stride)
    rng, gen = setup(zlib.crc32(name.encode()))
    sbuf, t = random_states(B, S, gen)
    tok = random_tokens((2, B, 3 * S), gen)
    gpb = 4 if S == 16 else 1
    plant(t, tok.transpose(0, 1), S, boundaries(B, gpb * 8) + boundaries(B, 64), rng)
    nbuf, nnz = guarded((B,), torch.int32)
    cur = []
    for i, j in chunks(B, S):
        c = host(t[i:j])
        cur.append(c)
        nnz[i:j] = torch.from_numpy(np.count_nonzero(c.reshape(j - i, -1), axis=1).astype(np.int32)).to(DEV)
    for k in range(2):
        dbuf, done = guarded((B,), torch.uint8)
        fbuf, ovf = guarded((B,), torch.uint8)
        ovf.zero_()
        ops.step_tracked(t, tok[k], nnz, done=done, overflow=ovf)
        free()
        check_states(sbuf, B, S, stride, f"{name} step {k}")
        check_flat(nbuf, f"{name} nnz")
        check_flat(dbuf, f"{name} done")
        check_flat(fbuf, f"{name} overflow")
        for c, (i, j) in enumerate(chunks(B, S)):
            w, wd, wo = CO.step_i8(cur[c], host(tok[k, i:j]))
            cur[c] = w
            assert np.array_equal(host(t[i:j]), w), f"{name} step {k}: state, games {i}..{j - 1}"
            assert np.array_equal(host(done[i:j]), wd) and np.array_equal(host(ovf[i:j]), wo), f"{name} step {k}: flags"
            assert np.array_equal(host(nnz[i:j]), np.count_nonzero(w.reshape(j - i, -1), axis=1)), f"{name} step {k}: nnz"
    del sbuf, t, tok, cur
    free()


# ---------------------------------------------------------------------------------------------------------------------
# tg_expand_i8 / tg_expand_keyed_i8


@pytest.mark.parametrize("name, keyed", [("expand_s4_nt", False), ("expand_s4_nt", True), ("expand_s16_nt", False),
                                         ("expand_s16_nt", True), ("expand_s25_keyed", True)])
def test_expand_streamed_children_match_oracle(name, keyed):
    """Children beyond kStreamOutBytes leave by non-temporal stores; children, done, changed, overflow and (keyed) the
    fused keys against the C oracle and its state_hash; guards around every buffer and between children."""
    S = SIZES[name][0]
    stride = stride_of(S)
    k = 4 if S == 25 else 8
    B = first_batch(name, k * stride)
    assert_in_band(name, B * k * stride)
    rng, gen = setup(zlib.crc32(f"{name}{keyed}".encode()))
    sbuf, src = random_states(B, S, gen)
    tok = random_tokens((B, k, 3 * S), gen)
    unit = {4: 64 // k, 16: 4, 25: 1}[S]
    plant(src, tok, S, boundaries(B, unit * 8) + boundaries(B, unit), rng)
    cbuf, kids = guarded_states(B * k, S, stride)
    fbuf, flags = guarded((3, B, k), torch.uint8)
    flags[2].zero_()
    if keyed:
        kbuf, keys = guarded((B, k), torch.int64)
        ops.expand(src, tok, out=kids.unflatten(0, (B, k)), done=flags[0], changed=flags[1], overflow=flags[2], keys=keys)
    else:
        ops.expand(src, tok, out=kids.unflatten(0, (B, k)), done=flags[0], changed=flags[1], overflow=flags[2])
    free()
    check_states(cbuf, B * k, S, stride, f"{name} children")
    check_flat(fbuf, f"{name} flags")
    if keyed:
        check_flat(kbuf, f"{name} keys")
    kv = kids.unflatten(0, (B, k))
    step = max(1, CHUNK // (k * stride))
    for i in range(0, B, step):
        j = min(B, i + step)
        wk, wd, wc, wo = CO.expand_i8(host(src[i:j]), host(tok[i:j]))
        assert np.array_equal(host(kv[i:j]), wk), f"{name}: children of parents {i}..{j - 1}"
        assert np.array_equal(host(flags[0, i:j]), wd) and np.array_equal(host(flags[1, i:j]), wc), f"{name}: done / changed"
        assert np.array_equal(host(flags[2, i:j]), wo), f"{name}: overflow"
        if keyed:
            want = CO.state_hash(wk.reshape((j - i) * k, S, S, S)).reshape(j - i, k)
            assert np.array_equal(host(keys[i:j]).view(np.uint64), want), f"{name}: keys of parents {i}..{j - 1}"
    del sbuf, src, cbuf, kids, tok
    free()


# ---------------------------------------------------------------------------------------------------------------------
# tg_step_stream_i8 beyond the resident batch


@pytest.mark.parametrize("name", ["stream_s4_rounds", "stream_s16_rounds", "stream_s25_rounds"])
def test_step_stream_in_rounds_matches_oracle(name):
    """Beyond tg_step_stream_capacity and without ready words the units run in rounds: K in-place steps, the state, the
    (K, B) done, overflow and progress against the oracle; guards around progress, status, done and overflow."""
    S = SIZES[name][0]
    K = 3
    cap = ops.step_stream_capacity(S, DEV)
    B = cap + RAGGED
    assert B > cap, name
    stride = stride_of(S)
    rng, gen = setup(zlib.crc32(name.encode()))
    sbuf, t = random_states(B, S, gen)
    tok = random_tokens((K, B, 3 * S), gen)
    unit = 64 if S == 4 else 4
    plant(t, tok.transpose(0, 1), S, boundaries(B, unit) + boundaries(B, cap) + [cap], rng)
    start = [host(t[i:j]) for i, j in chunks(B, S)]
    n_units = -(-B // 64) if S == 4 else B
    pbuf, prog = guarded((n_units,), torch.int32)
    prog.zero_()
    stbuf, status = guarded((1,), torch.int32)
    status.zero_()
    dbuf, done = guarded((K, B), torch.uint8)
    fbuf, ovf = guarded((B,), torch.uint8)
    ovf.zero_()
    ops.step_stream(t, tok, done=done, overflow=ovf, progress=prog, status=status)
    free()
    for buf, what in ((pbuf, "progress"), (stbuf, "status"), (dbuf, "done"), (fbuf, "overflow")):
        check_flat(buf, f"{name} {what}")
    check_states(sbuf, B, S, stride, f"{name} states")
    assert bool((prog == K).all()) and int(status[0]) == 0, name
    for c, (i, j) in enumerate(chunks(B, S)):
        cur, wo = start[c], np.zeros(j - i, np.uint8)
        for k in range(K):
            cur, wd, o = CO.step_i8(cur, host(tok[k, i:j]))
            wo |= o
            assert np.array_equal(host(done[k, i:j]), wd), f"{name}: done of step {k}, games {i}..{j - 1}"
        assert np.array_equal(host(t[i:j]), cur) and np.array_equal(host(ovf[i:j]), wo), f"{name}: games {i}..{j - 1}"
    del sbuf, t, tok, start
    free()


# ---------------------------------------------------------------------------------------------------------------------
# tg_step_emit


@pytest.mark.parametrize("name", ["step_emit_s4_two_launches", "step_emit_s16_two_launches"])
def test_step_emit_two_launches_match_oracle(name):
    """From kStreamOutBytes of model input on tg_step_emit is a step plus the frames kernel (at S=4 and S=16, each fused
    below it): the new head slot, done and the float32 frames (newest first) against the oracle."""
    S, T = SIZES[name][0], 2
    B = first_batch(name, T * S ** 3 * 4)
    assert_in_band(name, B * T * S ** 3 * 4)
    rng, gen = setup(7 + S)
    ring = ops.alloc_ring(B, S, T, DEV)
    ring.copy_(torch.randint(-2, 3, (B, T, S, S, S), dtype=torch.int8, device=DEV, generator=gen))
    tok = random_tokens((B, 3 * S), gen)
    plant(ring[:, 0], tok.view(B, 1, 3 * S), S, boundaries(B, 64 if S == 4 else 4), rng)
    before = host(ring)
    xbuf, x = guarded((B, T, S, S, S), torch.float32)
    scbuf, sc = guarded((B, 1), torch.float32)
    dbuf, done = guarded((B,), torch.uint8)
    _, _, _, nxt = ops.step_emit(ring, 0, tok, 3.0, dtype=torch.float32, out=x, scalars=sc, done=done)
    free()
    for buf, what in ((xbuf, "frames"), (scbuf, "scalars"), (dbuf, "done")):
        check_flat(buf, f"{name} {what}")
    assert nxt == 1
    for i, j in chunks(B, S):
        new, wd, _ = CO.step_i8(before[i:j, 0], host(tok[i:j]))
        r = host(ring[i:j])
        assert np.array_equal(r[:, 1], new) and np.array_equal(r[:, 0], before[i:j, 0]), f"{name}: ring, games {i}..{j - 1}"
        assert np.array_equal(host(done[i:j]), wd), f"{name}: done"
        assert np.array_equal(host(x[i:j]), r[:, [1, 0]].astype(np.float32)), f"{name}: frames"
        assert bool((sc[i:j] == 3.0).all()), f"{name}: scalars"
    del ring, x, before
    free()


# ---------------------------------------------------------------------------------------------------------------------
# grid-capped launches: the later grid-stride rounds


def zero_and_edge_games(view, S, bounds, rng):
    """All-zero games, games with one non-zero byte at the last position, full-range games at the boundaries."""
    idx, _ = planted_indices(view.shape[0], bounds, rng)
    st = np.zeros((len(idx), S, S, S), np.int8)
    for j in range(len(idx)):
        kind = j % 3
        if kind == 1:
            st[j].reshape(-1)[-1] = -128
        elif kind == 2:
            st[j] = rng.integers(-128, 128, size=(S, S, S))
    view[torch.from_numpy(idx).to(DEV)] = torch.from_numpy(st).to(DEV)


@pytest.mark.parametrize("name", ["done_s4_grid_cap", "done_s16_grid_cap"])
def test_done_and_nnz_past_the_grid_cap(name):
    S = SIZES[name][0]
    B = first_batch(name, 1)
    assert_in_band(name, B)
    rng, gen = setup(11 + S)
    _, st = random_states(B, S, gen)
    st.mul_((torch.rand((B, 1, 1, 1), device=DEV, generator=gen) < 0.5).to(torch.int8))   # half of the games all zero
    first_of_round2 = SIZES[name][1][0] - 1
    zero_and_edge_games(st, S, boundaries(B, 64) + [first_of_round2], rng)
    dbuf, d = guarded((B,), torch.uint8)
    nbuf, nnz = guarded((B,), torch.int32)
    abi("tg_done_i8", ptr(st), ptr(d), ptr(nnz), B, S, st.stride(0))
    free()
    check_flat(dbuf, f"{name} done")
    check_flat(nbuf, f"{name} nnz")
    for i, j in chunks(B, S):
        c = np.count_nonzero(host(st[i:j]).reshape(j - i, -1), axis=1)
        assert np.array_equal(host(nnz[i:j]), c), f"{name}: nnz, games {i}..{j - 1}"
        assert np.array_equal(host(d[i:j]), (c == 0).astype(np.uint8)), f"{name}: done, games {i}..{j - 1}"
    del st
    free()


def test_hash_past_the_grid_cap():
    name = "hash_s4_grid_cap"
    S = 4
    B = first_batch(name, 1)
    assert_in_band(name, B)
    rng, gen = setup(12)
    _, st = random_states(B, S, gen)
    zero_and_edge_games(st, S, boundaries(B, 64) + [SIZES[name][1][0] - 1], rng)
    kbuf, keys = guarded((B,), torch.int64)
    abi("tg_hash_u64", ptr(st), ptr(keys), B, S, st.stride(0))
    free()
    check_flat(kbuf, f"{name} keys")
    for i, j in chunks(B, S):
        assert np.array_equal(host(keys[i:j]).view(np.uint64), CO.state_hash(host(st[i:j]))), f"{name}: games {i}..{j - 1}"
    del st
    free()


def test_seen_past_the_grid_cap():
    """fresh = masked and not in the table before the call (equal keys in one call alike), against numpy; then every
    masked key is in the table."""
    name = "seen_grid_cap"
    n = first_batch(name, 1)
    assert_in_band(name, n)
    rng = np.random.default_rng(13)
    keys = rng.integers(1, 2 ** 63, size=n, dtype=np.int64)
    keys[rng.integers(0, n, size=n // 8)] = keys[rng.integers(0, n, size=n // 8)]   # duplicates within the call
    keys[-RAGGED:] = keys[0]                                                      # ... in the last round too
    keys[rng.integers(0, n, size=16)] = 0                                         # the zero key
    prior = np.concatenate([keys[rng.integers(0, n, size=n // 4)], rng.integers(1, 2 ** 63, size=1000, dtype=np.int64)])
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[-1] = 1
    table = ops.alloc_seen_table(1 << 23, DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.seen(torch.from_numpy(prior).to(DEV), table, insert=True, status=status)
    fbuf, fresh = guarded((n,), torch.uint8)
    kd = torch.from_numpy(keys).to(DEV)
    ops.seen(kd, table, mask=torch.from_numpy(mask).to(DEV), insert=True, status=status, fresh=fresh)
    free()
    check_flat(fbuf, name)
    want = O.seen_u64_np(keys.view(np.uint64), prior.view(np.uint64), mask)
    got = host(fresh)
    assert np.array_equal(got, want), f"{name}: fresh differs first at key {int(np.nonzero(got != want)[0][0])} of {n}"
    again = ops.seen(kd, table, mask=torch.from_numpy(mask).to(DEV))
    assert not bool(again.any()) and int(status[0]) == 0, name
    del table, kd
    free()


def sample_with_last_round(B, per_round, rng, n=200):
    """~n games: random ones, the last game, and the first / last games of the last grid-stride round."""
    last_round = (B - 1) // per_round * per_round
    s = set(rng.integers(0, B, size=n - 8).tolist()) | {0, B - 1, B - 2, last_round, last_round + 1, last_round - 1}
    return np.array(sorted(i for i in s if 0 <= i < B), np.int64)


@pytest.mark.parametrize("name", ["rank_s4_grid_cap", "rank_s5_grid_cap"])
def test_slice_rank_past_the_grid_cap(name):
    S = SIZES[name][0]
    B = first_batch(name, 1)
    assert_in_band(name, B)
    rng, gen = setup(14 + S)
    _, st = random_states(B, S, gen)
    per_round = (1 << 20) * (4 if S == 4 else 1)
    idx = sample_with_last_round(B, per_round, rng)
    edge = torch.from_numpy(rng.integers(-128, 128, size=(8, S, S, S)).astype(np.int8)).to(DEV)
    st[torch.from_numpy(idx[-8:]).to(DEV)] = edge                                # full-range games at the end
    st[int(idx[1])] = 0
    rbuf, rank = guarded((B,), torch.int32)
    abi("tg_rank_i32", ptr(st), ptr(rank), B, S, st.stride(0))
    free()
    check_flat(rbuf, f"{name} rank")
    it = torch.from_numpy(idx).to(DEV)
    assert np.array_equal(host(rank[it]), O.slice_rank_exact(host(st[it]))), name
    del st
    free()


@pytest.mark.parametrize("name", ["reset_broadcast_s4_grid_cap"])
def test_reset_broadcast_past_the_grid_cap(name):
    S = 4
    B = first_batch(name, 1)
    assert_in_band(name, B)
    rng = np.random.default_rng(15)
    obuf, out = guarded_states(B, S, stride_of(S))
    start = torch.from_numpy(rng.integers(-128, 128, size=(S, S, S)).astype(np.int8)).to(DEV)
    ops.reset_broadcast(out, start)
    free()
    check_states(obuf, B, S, stride_of(S), name)
    for i, j in chunks(B, S):
        assert bool((out[i:j] == start).all()), f"{name}: games {i}..{j - 1}"
    del out, obuf
    free()


@pytest.mark.parametrize("name", ["copy_bytes_grid_cap", "copy_s16_nt1", "copy_s16_nt2"])
def test_copy_by_footprint_and_past_the_grid_cap(name):
    S = SIZES[name][0]
    stride = 68 if name == "copy_bytes_grid_cap" else stride_of(S)             # 68: not 16-byte aligned -> byte path
    B = first_batch(name, 1 if SIZES[name][2] == "games" else 2 * stride)
    assert_in_band(name, B if SIZES[name][2] == "games" else 2 * B * stride)
    rng, gen = setup(16)
    sbuf, src = random_states(B, S, gen, stride)
    zero_and_edge_games(src, S, boundaries(B, 64) + [65536], rng)
    obuf, out = guarded_states(B, S, stride)
    ops.copy_states(src, out)
    free()
    check_states(obuf, B, S, stride, name)
    for i, j in chunks(B, S):
        assert torch.equal(out[i:j], src[i:j]), f"{name}: games {i}..{j - 1}"
    del sbuf, src, obuf, out
    free()


# ---------------------------------------------------------------------------------------------------------------------
# tg_gen_demos_i8, tg_sample_basis_i8, tg_change_basis_i8


def test_gen_demos_tokens_past_the_grid_cap():
    """gen_tokens_kernel<4, 16> beyond its 16 384 workgroups: tokens, target and overflow against the C oracle."""
    name = "gen_s4_tokens_grid_cap"
    S, R = 4, 8
    B = first_batch(name, 3 * R)
    assert_in_band(name, B * R * 3)
    tbuf, tok = guarded((B, R, 3 * S), torch.int8)
    gbuf, tgt = guarded_states(B, S, stride_of(S))
    fbuf, ovf = guarded((B,), torch.uint8)
    ovf.zero_()                                          # (overflow is sticky: the generator only sets it)
    ops.gen_demos(B, S, R, DEV, seed=21, target=tgt, actions=tok, overflow=ovf)
    free()
    check_flat(tbuf, f"{name} tokens")
    check_flat(fbuf, f"{name} overflow")
    check_states(gbuf, B, S, stride_of(S), f"{name} target")
    thr = O.categorical_thresholds((0.15, 0.7, 0.15))
    step = 1 << 20
    for i in range(0, B, step):
        j = min(B, i + step)
        wt, wg, wo = CO.gen_demos_i8(j - i, S, R, thr, (-1, 0, 1), 1, 21, game_id_offset=i)
        assert np.array_equal(host(tok[i:j]), wt) and np.array_equal(host(tgt[i:j]), wg), f"{name}: games {i}..{j - 1}"
        assert np.array_equal(host(ovf[i:j]), wo), f"{name}: overflow"
    del tok, tgt
    free()


@pytest.mark.parametrize("name", ["gen_s4_basis_grid_cap", "gen_s9_basis_grid_cap"])
def test_gen_demos_in_a_basis_past_the_grid_cap(name):
    """The basis-token kernels beyond their workgroup caps: every game against the numpy oracle (chunked by game id)."""
    S, R = SIZES[name][0], 8
    B = first_batch(name, 1)
    assert_in_band(name, B)
    stride = 744 if S == 9 else stride_of(S)             # S=9: not a multiple of 16, so the fused generator declines
    assert S != 9 or stride % 16 != 0
    P = ops.sample_basis(B, S, DEV, seed=22)
    tbuf, tok = guarded((B, R, 3 * S), torch.int8)
    gbuf, tgt = guarded_states(B, S, stride)
    fbuf, ovf = guarded((B,), torch.uint8)
    ovf.zero_()
    ops.gen_demos(B, S, R, DEV, seed=23, basis=P, target=tgt, actions=tok, overflow=ovf)
    free()
    check_flat(tbuf, f"{name} tokens")
    check_flat(fbuf, f"{name} overflow")
    check_states(gbuf, B, S, stride, f"{name} target")
    thr = O.categorical_thresholds((0.15, 0.7, 0.15))
    Ph = host(P)
    step = 8192
    for i in range(0, B, step):
        j = min(B, i + step)
        wt, wg, wo = O.gen_demos_i8(j - i, S, R, thr, (-1, 0, 1), 1, 23, game_id_offset=i, basis=Ph[i:j])
        assert np.array_equal(host(tok[i:j]), wt) and np.array_equal(host(tgt[i:j]), wg), f"{name}: games {i}..{j - 1}"
        assert np.array_equal(host(ovf[i:j]), wo), f"{name}: overflow"
    del P, tok, tgt
    free()


def test_sample_and_change_basis_past_the_matrix_core_grid():
    """sample_basis in full against the oracle; change_basis (matrix-core grid of 4 workgroups per CU, looping) on a sample
    that includes the last round and the last game, out and overflow against O.change_basis_i8."""
    name = "change_basis_s16_rounds"
    S = 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * cus * 2 + RAGGED
    assert B > 4 * cus, f"{name}: {B} games do not loop over a grid of {4 * cus} workgroups"
    rng, gen = setup(24)
    P = ops.sample_basis(B, S, DEV, seed=25)
    Po = O.sample_basis(B, S, O.categorical_thresholds((0.025, 0.95, 0.025)), (-1, 0, 1), seed=25)[0]
    assert np.array_equal(host(P), Po), name
    sbuf, st = random_states(B, S, gen)
    idx = sample_with_last_round(B, 4 * cus, rng)
    st[torch.from_numpy(idx[-4:]).to(DEV)] = torch.from_numpy(
        rng.integers(-128, 128, size=(4, S, S, S)).astype(np.int8)).to(DEV)   # overflowing games at the end
    obuf, out = guarded_states(B, S, stride_of(S))
    fbuf, ovf = guarded((B,), torch.uint8)
    ovf.zero_()
    ops.change_basis(st, P.to(torch.int32), out=out, overflow=ovf)
    free()
    check_states(obuf, B, S, stride_of(S), name)
    check_flat(fbuf, name)
    it = torch.from_numpy(idx).to(DEV)
    want, wo = O.change_basis_i8(host(st[it]), Po[idx])
    assert np.array_equal(host(out[it]), want) and np.array_equal(host(ovf[it]), wo), name
    del sbuf, st, obuf, out, P
    free()

