"""Device buffers with guard bytes before and after them (and in the padding between games), and the checks that the
guards survived a launch.  Shared by test_gpu_parity.py::test_no_out_of_bounds_writes and test_gpu_full_size_oracle.py."""
import numpy as np
import torch

GUARD, CANARY = 256, 0x5A
DEV = "cuda:0"


def guarded_states(B, S, stride, device=DEV):
    """(buffer, (B,S,S,S) int8 view with a game stride of ``stride`` bytes) -- every byte outside the games is CANARY."""
    n = S ** 3
    buf = torch.full((GUARD + B * stride + GUARD,), CANARY, dtype=torch.uint8, device=device).view(torch.int8)
    view = buf[GUARD:GUARD + B * stride].view(B, stride)[:, :n].unflatten(1, (S, S, S))
    return buf, view


def check_states(buf, B, S, stride, what, chunk_bytes=64 << 20):
    """The guards around and between the games of a ``guarded_states`` buffer are intact (read back in chunks)."""
    raw = buf.view(torch.uint8)
    n = S ** 3
    assert bool((raw[:GUARD] == CANARY).all()) and bool((raw[GUARD + B * stride:] == CANARY).all()), what
    if stride == n:
        return
    body = raw[GUARD:GUARD + B * stride].view(B, stride)
    step = max(1, chunk_bytes // stride)
    for i in range(0, B, step):
        pad = body[i:i + step, n:]
        assert bool((pad == CANARY).all()), f"{what} (padding between games {i}..{min(B, i + step) - 1})"


def guarded(shape, dtype, device=DEV):
    """(buffer, tensor of ``shape`` / ``dtype``) with GUARD canary bytes on both sides."""
    numel = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + numel + GUARD,), CANARY, dtype=torch.uint8, device=device)
    return buf, buf[GUARD:GUARD + numel].view(dtype).view(shape)


def check_flat(buf, what):
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all()), what
