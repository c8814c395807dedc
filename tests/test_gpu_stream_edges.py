"""The four resident steppers of tg_step_stream_i8 (s4_stream_kernel<1>, s16_stream_kernel, s25_stream_kernel here; the lane
kernel and s4_stream_kernel<2> in test_gpu_ab_library.py) on batches that walk along the edges of the digit form for K
steps: tests/stream_walk.py builds them, tests/test_stream_walk_cpu.py holds them to their census.  State, every row of
the (K, B) done, the sticky overflow, progress and status against the oracle trajectory, bit for bit."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import mat_mul_amd
import stream_walk as W
from mat_mul_amd import ops
from guarded_buffers import check_flat, check_states, guarded, guarded_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = {S: (B, K) for S, B, K in W.GPU_CASES}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)    # (a copy: the shared walks are read-only)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "libtensorgame.so" in open("/proc/self/maps").read(), "the HIP library is not the one loaded"


@lru_cache(maxsize=None)
def walk(S, shift):
    """(state, actions, final state, done (K,B), overflow) of the batch for (S, shift): built and stepped by the oracle
    once, shared read-only by every test."""
    B, K = SIZES[S]
    st, ac = W.make_walk(S, B, K, shift, W.walk_seed(S, shift))
    out = (st, ac) + W.trajectory(st, ac, shift)
    for a in out:
        a.flags.writeable = False
    return out


def strided(st, stride):
    """The batch on the device at a game stride of ``stride`` bytes (zero padding)."""
    B, S = st.shape[0], st.shape[1]
    buf = torch.zeros((B, stride), dtype=torch.int8, device=DEV)
    t = buf[:, :S ** 3].unflatten(1, (S, S, S))
    t.copy_(dev(st))
    return t


def strides_of(S):
    n = -(-S ** 3 // 16) * 16
    return (n, n + 32)    # S = 4: 64 and 96 bytes; S = 16: packed and padded; S = 25: padded (15 632) and wider


def run(t, acd, shift, ready=None):
    B, S, K = t.shape[0], t.shape[1], acd.shape[0]
    n_units, gpu = ops.step_stream_layout(B, S, DEV)
    ovf = torch.zeros(B, dtype=torch.uint8, device=DEV)
    prog = torch.zeros(n_units, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    done = torch.full((K, B), 7, dtype=torch.uint8, device=DEV)
    ops.step_stream(t, acd, done=done, overflow=ovf, ready=ready, progress=prog, status=status, shift=shift)
    return done, ovf, prog, status


def check(S, shift, t, done, ovf, prog, status, what):
    st, ac, want, want_done, want_ovf = walk(S, shift)
    B, K = SIZES[S]
    kinds = W.kinds_of(B)
    assert int(status[0]) == 0 and bool((prog == K).all()), (what, int(status[0]), host(prog))
    bad = np.flatnonzero((host(t) != want).reshape(B, -1).any(axis=1))
    assert bad.size == 0, f"{what}: state of games {[(int(b), kinds[b]) for b in bad[:8]]} ({bad.size} in all)"
    bad = np.argwhere(host(done) != want_done)
    assert bad.size == 0, f"{what}: done[k, b] at {[(int(k), int(b), kinds[b]) for k, b in bad[:8]]} ({len(bad)} in all)"
    bad = np.flatnonzero(host(ovf) != want_ovf)
    assert bad.size == 0, f"{what}: overflow of games {[(int(b), kinds[b], int(want_ovf[b])) for b in bad[:8]]}"


@pytest.mark.parametrize("shift", W.SHIFTS)
@pytest.mark.parametrize("S", [4, 16, 25])
def test_walk_along_the_digit_form_edges(S, shift):
    """K = 19 steps (blocks of 8, 8, 3) of games that rise above the digit form's limit and return, sit on it, overflow
    and go on, are done by either form, done / undone / done, land on -129 / -128 / 127 / 128, with wide steps in the
    middle of a block -- at both game strides, for the four shifts that admit the digit form and two that do not."""
    st, ac, *_ = walk(S, shift)
    B, K = SIZES[S]
    n_units, gpu = ops.step_stream_layout(B, S, DEV)
    assert gpu == (16 if S == 4 else 1) and n_units == -(-B // gpu)
    assert S != 4 or (n_units > 8 and B % 16)          # several wavefronts and workgroups, a ragged last team
    acd = dev(ac)
    for stride in strides_of(S):
        t = strided(st, stride)
        assert t.stride(0) == stride
        out = run(t, acd, shift)
        torch.cuda.synchronize()
        check(S, shift, t, *out, what=f"S={S} shift={shift} stride={stride}")


@pytest.mark.parametrize("shift", W.SHIFTS)
def test_s25_walk_with_the_tokens_at_every_byte_offset(shift):
    """A step's 75 token bytes start at any byte address; the kernel fetches aligned dwords and reads from byte A & 3 on.
    With the actions four bytes into their buffer the offsets A & 3 still take all four values across games and steps."""
    S = 25
    st, ac, *_ = walk(S, shift)
    B, K = SIZES[S]
    buf = torch.zeros(K * B * 75 + 4, dtype=torch.int8, device=DEV)
    acd = buf[4:].view(K, B, 75)
    acd.copy_(dev(ac))
    assert acd.is_contiguous() and acd.data_ptr() % 4 == 0 and acd.data_ptr() == buf.data_ptr() + 4
    assert {(acd.data_ptr() + (k * B + g) * 75) & 3 for k in range(K) for g in range(B)} == {0, 1, 2, 3}
    t = strided(st, strides_of(S)[0])
    out = run(t, acd, shift)
    torch.cuda.synchronize()
    check(S, shift, t, *out, what=f"S=25 shift={shift} actions at +4")


@pytest.mark.parametrize("shift", [1, 0])
@pytest.mark.parametrize("S", [4, 16, 25])
def test_walk_released_step_by_step(S, shift):
    """The ready words released one by one from a second stream, each release waited for before the next: the stepper
    then mostly sees one new word at a time and runs blocks of one step, where the S = 4 test for a token above 3 is per
    step.  That is likely, not guaranteed -- a stepper that polls late finds several words set and takes them as one
    block, and nothing here can tell which happened; what the test holds is that the result does not depend on it.
    Every word is released, the spin is bounded by the kernel's own clock; the result is that of the run without ready
    words."""
    st, ac, *_ = walk(S, shift)
    B, K = SIZES[S]
    acd = dev(ac)
    plain = strided(st, strides_of(S)[0])
    plain_out = run(plain, acd, shift)
    t = strided(st, strides_of(S)[0])
    ready = torch.zeros(K, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    # (the producer on a HIGH-priority stream: its fills never queue up behind the resident stepper)
    side, prod = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):
        out = run(t, acd, shift, ready=ready)
    with torch.cuda.stream(prod):
        for k in range(K):
            ready[k:k + 1].fill_(1)
            prod.synchronize()
    side.synchronize()
    torch.cuda.synchronize()
    if int(out[3][0]) == 1:
        pytest.fail("the stepper gave up waiting (status 1) although every step was released within milliseconds")
    check(S, shift, t, *out, what=f"S={S} shift={shift} step by step")
    assert torch.equal(t, plain) and all(torch.equal(a, b) for a, b in zip(out, plain_out))


@pytest.mark.parametrize("S", [4, 16, 25])
def test_walk_leaves_every_guard_byte(S):
    """step_stream between guard bytes: in front of and behind the states and in the padding between the games (the 7
    bytes behind each S = 25 game, whose last chunk leaves as 8 + 1 bytes), around the (K, B) done rows, overflow and
    progress; the last S = 4 team has dead lanes that shadow the last game."""
    B, K = SIZES[S]
    assert S != 4 or B % 16
    for shift in (1, 4):
        st, ac, *_ = walk(S, shift)
        acd = dev(ac)
        for stride in strides_of(S):
            n_units, _ = ops.step_stream_layout(B, S, DEV)
            sbuf, t = guarded_states(B, S, stride)
            t.copy_(dev(st))
            dbuf, done = guarded((K, B), torch.uint8)
            obuf, ovf = guarded((B,), torch.uint8)
            pbuf, prog = guarded((n_units,), torch.int32)
            ovf.zero_()
            prog.zero_()
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.step_stream(t, acd, done=done, overflow=ovf, progress=prog, status=status, shift=shift)
            torch.cuda.synchronize()
            what = f"step_stream S={S} shift={shift} stride={stride}"
            check_states(sbuf, B, S, stride, what)
            for buf in (dbuf, obuf, pbuf):
                check_flat(buf, what)
            check(S, shift, t, done, ovf, prog, status, what)
    if S == 25:  # the packed layout (a game stride of 15 625 bytes, no multiple of 16) is refused, not stepped
        st, ac, *_ = walk(S, 1)
        sbuf, t = guarded_states(B, S, S ** 3)
        t.copy_(dev(st))
        assert t.stride(0) == S ** 3 and t.stride(0) % 16
        with pytest.raises(mat_mul_amd.TensorGameError, match="needs 16-byte aligned states") as err:
            ops.step_stream(t, dev(ac), shift=1)
        assert err.value.code < 0
        torch.cuda.synchronize()
        check_states(sbuf, B, S, S ** 3, "step_stream refusing the packed S = 25 layout")
        assert np.array_equal(host(t), st)


@pytest.mark.parametrize("fill", [1, -128])
def test_s25_padding_does_not_count(fill):
    """The chunk that holds an S = 25 game's last 9 bytes is loaded whole: what lies in the 7 bytes behind them must
    enter neither the chunk's norm nor done[k] -- games whose live bytes reach zero are done whatever the padding holds."""
    S, shift = 25, 1
    st, ac, want, want_done, want_ovf = walk(S, shift)
    B, K = SIZES[S]
    reach_zero = [b for b, kind in enumerate(W.kinds_of(B)) if kind in ("demo", "done_undone_done")]
    assert len(reach_zero) >= 4 and want_done[:, reach_zero].any(axis=0).all() and not want_done.all(axis=0).any()
    for stride in strides_of(S):
        buf = torch.full((B, stride), fill, dtype=torch.int8, device=DEV)
        t = buf[:, :S ** 3].unflatten(1, (S, S, S))
        t.copy_(dev(st))
        out = run(t, dev(ac), shift)
        torch.cuda.synchronize()
        check(S, shift, t, *out, what=f"S=25 padding {fill} stride={stride}")
        assert bool((buf[:, S ** 3:] == fill).all())
