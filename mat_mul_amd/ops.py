"""Tensor-level wrappers over the C ABI (include/tensor_game.h).

Every function takes PyTorch-ROCm tensors, checks device / dtype / layout on the host,
and enqueues ONE kernel on the caller's current HIP stream (so calls can be captured in a
``torch.cuda.graph``).  PyTorch is plumbing here: device memory and streams.  There is
no CPU path: a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TG_MAX_ACTIONS, TG_MAX_S, TG_MAX_VALUES, TensorGameError, call

__all__ = [
    "step", "step_tracked", "copy_states", "prepare_step", "step_many", "step_stream", "step_stream_layout", "step_stream_capacity", "expand", "done", "reset_matmul", "reset_broadcast", "gen_from_factors",
    "gen_demos", "sample_basis", "change_basis", "as_tokens", "categorical_thresholds",
    "alloc_states", "alloc_ring", "emit_frames", "step_emit", "demo_items", "state_hash", "slice_rank", "alloc_seen_table", "seen",
    "search_reset", "search_select", "search_commit", "search_advance", "search_policy", "replay_add", "replay_items",
    "replay_pack", "replay_add_packed", "replay_add_lists",
    "net_check", "net_weights_size", "net_torso", "net_sample", "net_logits",
    "net_s25_check", "net_s25_weights_size", "net_s25_torso", "net_s25_sample", "net_s25_logits",
    "net_train_check", "net_train_workspace_size", "net_loss_grad",
    "net_train_sliced_check", "net_train_sliced_workspace_size", "net_loss_grad_sliced",
    "net_train_s25_check", "net_train_s25_workspace_size", "net_loss_grad_s25",
    "rollout_check", "rollout_records", "rollout_advance",
    "RolloutSlots", "rollout_slots", "rollout_advance_slots", "rollout_refill",
    "symmetry_sample", "symmetry_apply",
    "solution_check", "solution_canon",
    "orbit_check", "orbit_fixes", "orbit_workspace_size", "orbit_canon",
    "basis_inverse_check", "solution_rebase_check", "basis_inverse", "solution_rebase",
    "flip_check", "flip_begin", "flip_advance", "flip_plus_check", "flip_advance_plus",
    "flip2_check", "flip2_begin", "flip2_advance", "flip2_residual",
    "lift2_check", "lift2_workspace_bytes", "lift2_signs",
    "bilinear_check", "bilinear_encode", "bilinear_decode",
    "reset_matmul_rect", "bilinear_rect_check", "bilinear_rect_encode", "bilinear_rect_decode",
    "bilinear_products_check", "bilinear_products",
]


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _launch(dev, name: str, *args) -> None:
    """Enqueue ``name`` on device ``dev``: the device guard, and the caller's current stream as the last argument."""
    with torch.cuda.device(dev):
        call(name, *args, _stream(dev))


def _u64(x) -> int:
    """A seed or call index as the 64 bits the ABI takes (negative values wrap)."""
    return int(x) & (2 ** 64 - 1)


def _need_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise TensorGameError(name, -1, f"{name} must live on a ROCm device (got {t.device}); there is no CPU path")


def _state_layout(state: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(B, S, game_stride_bytes) of an int8 (B,S,S,S) tensor whose games are dense."""
    _need_gpu(state, name)
    if state.dtype != torch.int8 or state.dim() != 4 or not (state.shape[1] == state.shape[2] == state.shape[3]):
        raise TensorGameError(name, -1, f"{name} must be int8 of shape (B,S,S,S), got {state.dtype} {tuple(state.shape)}")
    B, S = state.shape[0], state.shape[1]
    if B > 0 and state.stride()[1:] != (S * S, S, 1):
        raise TensorGameError(name, -1, f"{name}: each game must be C-contiguous (S,S,S)")
    stride = state.stride(0) if B > 1 else max(state.stride(0), S ** 3)
    if stride < S ** 3:
        raise TensorGameError(name, -1, f"{name}: game stride {stride} < S^3")
    return B, S, stride


def _tokens(actions: torch.Tensor, lead: Tuple[int, ...], S: int, dev: torch.device, name: str) -> torch.Tensor:
    _need_gpu(actions, name)
    if actions.dtype != torch.int8:
        raise TensorGameError(name, -1, f"{name} must be int8 tokens (use ops.as_tokens), got {actions.dtype}")
    if tuple(actions.shape) != (*lead, 3 * S):
        raise TensorGameError(name, -1, f"{name} must have shape {(*lead, 3 * S)}, got {tuple(actions.shape)}")
    if actions.device != dev:
        raise TensorGameError(name, -1, f"{name} is on {actions.device}, state on {dev}")
    return actions if actions.is_contiguous() else actions.contiguous()


def _flag(t: Optional[torch.Tensor], shape: Tuple[int, ...], dtype, dev, name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
        raise TensorGameError(name, -1, f"{name} must be contiguous {dtype} {shape} on {dev}")
    return t


def _out(t: Optional[torch.Tensor], shape: Tuple[int, ...], dtype, dev, name: str, new=torch.empty) -> torch.Tensor:
    """An optional output: allocated with ``new`` when it is not given, held to the rule of ``_flag`` when it is."""
    if t is None:
        return new(shape, dtype=dtype, device=dev)
    return _flag(t, shape, dtype, dev, name)


def _out_states(out, state, B: int, S: int, stride: int, fn: str) -> torch.Tensor:
    """The state batch an entry writes for the input batch ``state``: allocated with the input's strides when it is not
    given, else of the same shape, game stride and device (``out=state`` is the in-place form)."""
    dev = state.device
    if out is None:
        out = torch.empty_strided(state.shape, state.stride(), dtype=torch.int8, device=dev)
    Bo, So, ostride = _state_layout(out, "out")
    if (Bo, So) != (B, S) or (B > 1 and ostride != stride) or out.device != dev:
        raise TensorGameError(fn, -1, "out must match state's shape, stride and device")
    return out


def as_tokens(actions, device=None, check: bool = True) -> torch.Tensor:
    """int64 (reference dtype, datasets.py:140) or any integer tensor -> int8 tokens.
    ``check`` verifies the values fit int8 (one host sync); the reference never range-checks
    tokens (utils.py:64-66), the build refuses values it cannot represent."""
    t = torch.as_tensor(actions)
    if t.dtype != torch.int8:
        if t.is_floating_point():
            raise TensorGameError("as_tokens", -1, "tokens must be integers")
        if check and t.numel() and (int(t.min()) < -128 or int(t.max()) > 127):
            raise TensorGameError("as_tokens", -1, "token outside int8 range")
        t = t.to(torch.int8)
    if device is not None:
        t = t.to(device)
    return t.contiguous()


def alloc_states(B: int, S: int, device, pad_to: int = 16, zero: bool = True) -> torch.Tensor:
    """int8 (B,S,S,S) states whose game stride is S^3 rounded up to ``pad_to`` bytes (16 keeps every
    game on the dwordx4 fast path; S=25 -> 15632).  Zero-filled unless ``zero=False`` (outputs that a
    kernel overwrites completely; the padding bytes are never read)."""
    n = S ** 3
    stride = -(-n // pad_to) * pad_to
    buf = (torch.zeros if zero else torch.empty)((B, stride), dtype=torch.int8, device=device)
    return buf[:, :n].unflatten(1, (S, S, S))


def step(state, actions, out=None, done=None, overflow=None, shift: int = 1):
    """state_out = state - u(x)v(x)w(actions); done[b] = state_out[b] all zero.
    == reference get_child_states (act.py:266-275, k=1,T=1) + tensor_factorized per game
    (utils.py:181-188).  ``out=state`` steps in place.  Returns (state_out, done)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    actions = _tokens(actions, (B,), S, dev, "actions")
    out = _out_states(out, state, B, S, stride, "step")
    done = _out(done, (B,), torch.uint8, dev, "done")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    _launch(dev, "tg_step_i8", _ptr(state), _ptr(out), _ptr(actions), _ptr(done), _ptr(overflow), B, S, stride, int(shift))
    return out, done


def copy_states(state, out=None):
    """out[b] = state[b] (a snapshot of a batch of games; the reference's step is functional and its callers
    keep the parent, act.py:183-195).  ``out`` may have a different game stride.  Returns out."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    if out is None:
        out = alloc_states(B, S, dev, zero=False)
    Bo, So, ostride = _state_layout(out, "out")
    if (Bo, So) != (B, S) or out.device != dev:
        raise TensorGameError("copy_states", -1, "out must match state's shape and device")
    _launch(dev, "tg_copy_i8", _ptr(state), _ptr(out), B, S, stride, ostride)
    return out


def prepare_step(state, actions_seq, done, overflow=None, shift: int = 1):
    """Validate once, launch many: returns ``launch(k)`` that enqueues one in-place
    ``tg_step_i8`` with ``actions_seq[k]`` on the current stream with no per-call checks
    (for rollouts and hipGraph capture, where Python overhead would dominate a 2 us kernel)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    acts = [_tokens(a, (B,), S, dev, "actions") for a in actions_seq]
    done = _flag(done, (B,), torch.uint8, dev, "done")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    fn = _lib.lib.tg_step_i8
    sp, dp, op = _ptr(state), _ptr(done), _ptr(overflow)
    aps = [_ptr(a) for a in acts]
    Bc, Sc, stc, shc = C.c_int64(B), C.c_int(S), C.c_int64(stride), C.c_int(int(shift))
    index = dev.index if dev.index is not None else torch.cuda.current_device()

    def launch(k: int) -> None:
        rc = fn(sp, sp, aps[k], dp, op, Bc, Sc, stc, shc, C.c_void_p(torch.cuda.current_stream(index).cuda_stream))
        if rc != 0:
            raise TensorGameError("tg_step_i8", rc, _lib.lib.tg_last_error().decode())

    launch.keepalive = (state, acts, done, overflow)  # the raw pointers above must stay valid
    return launch


def step_many(state, actions, out=None, done_step=None, overflow=None, shift: int = 1):
    """K sequential steps, state resident on chip.  actions int8 (B,K,3S).
    == reference SyntheticDemoDataset._take_actions (datasets.py:144-153).
    Returns (state_out, done_step int32: first step whose post-state is zero, or -1)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    if actions.dim() != 3:
        raise TensorGameError("step_many", -1, "actions must be (B,K,3S)")
    K = actions.shape[1]
    actions = _tokens(actions, (B, K), S, dev, "actions")
    out = _out_states(out, state, B, S, stride, "step_many")
    done_step = _out(done_step, (B,), torch.int32, dev, "done_step")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    _launch(dev, "tg_step_many_i8", _ptr(state), _ptr(out), _ptr(actions), _ptr(done_step), _ptr(overflow),
            B, S, K, stride, int(shift))
    return out, done_step


def step_tracked(state, actions, nnz, done=None, overflow=None, shift: int = 1):
    """The in-place step that reads only what the action touches: ``nnz`` int32 (B,) carries the exact number of non-zero
    entries per game (``done(state)[1]`` computes it) and is updated; ``done[b] = (nnz[b] == 0)``.  Same state, done and
    overflow as ``step(state, actions, out=state)``.  Returns (state, done)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    actions = _tokens(actions, (B,), S, dev, "actions")
    if nnz.dtype != torch.int32 or tuple(nnz.shape) != (B,) or not nnz.is_contiguous() or nnz.device != dev:
        raise TensorGameError("step_tracked", -1, f"nnz must be a contiguous int32 ({B},) tensor on {dev}")
    done = _out(done, (B,), torch.uint8, dev, "done")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    _launch(dev, "tg_step_tracked_i8", _ptr(state), _ptr(actions), _ptr(nnz), _ptr(done), _ptr(overflow), B, S, stride,
            int(shift))
    return state, done


def step_stream_layout(B: int, S: int, device=None) -> Tuple[int, int]:
    """(n_units, games_per_unit) of ``step_stream``: unit u (a wavefront) owns games [u*gpu, (u+1)*gpu)."""
    n, g = C.c_int64(0), C.c_int(0)
    with torch.cuda.device(torch.device(device) if device is not None else torch.cuda.current_device()):
        call("tg_step_stream_layout", B, S, C.byref(n), C.byref(g))
    return int(n.value), int(g.value)


def step_stream_capacity(S: int, device=None) -> int:
    """The largest batch ``step_stream`` takes together with ready words on this device (every unit resident at once)."""
    n = C.c_int64(0)
    with torch.cuda.device(torch.device(device) if device is not None else torch.cuda.current_device()):
        call("tg_step_stream_capacity", S, C.byref(n))
    return int(n.value)


def step_stream(state, actions, done=None, overflow=None, ready=None, progress=None, status=None, shift: int = 1):
    """K in-place steps in ONE launch for action blocks that become available step by step.
    actions int8 (K,B,3S) STEP-major; ready uint32/int32 (K) (step k waits for ready[k] != 0) or None;
    done uint8 (K,B); progress int32 (n_units); status int32 (1).  == K calls of ``step(state, actions[k], out=state)``
    without the launch boundary between them.  Returns (state, done)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    if actions.dim() != 3:
        raise TensorGameError("step_stream", -1, "actions must be (K,B,3S), step-major")
    K = actions.shape[0]
    actions = _tokens(actions, (K, B), S, dev, "actions")
    done = _out(done, (K, B), torch.uint8, dev, "done")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    for name, t, n in (("ready", ready, K), ("progress", progress, None), ("status", status, 1)):
        if t is not None and (t.dtype not in (torch.int32, torch.uint32) or t.dim() != 1 or not t.is_contiguous()
                              or (n is not None and t.numel() != n) or t.device != dev):
            # (device memory only: the stepper polls and publishes with agent-scope accesses; a host producer
            # releases a step by a fill / copy enqueued on another stream, not by writing mapped memory)
            raise TensorGameError("step_stream", -1, f"{name} must be a contiguous 32-bit vector on {dev}")
    if progress is not None:
        try:
            n_units = step_stream_layout(B, S, dev)[0]
        except TensorGameError:
            if ready is not None or S != 4:
                raise
            n_units = -(-B // 64)  # beyond the resident batch, without ready words: units of 64 games in rounds
        if progress.numel() < n_units:
            raise TensorGameError("step_stream", -1, "progress needs one word per unit (ops.step_stream_layout)")
    _launch(dev, "tg_step_stream_i8", _ptr(state), _ptr(actions), _ptr(done), _ptr(overflow), _ptr(ready), _ptr(progress),
            _ptr(status), B, S, K, stride, int(shift))
    return state, done


def expand(state, actions, out=None, done=None, changed=None, overflow=None, shift: int = 1, want_keys: bool = False,
           keys=None):
    """k children per parent.  actions int8 (B,k,3S) -> children int8 (B,k,S,S,S), done (B,k),
    changed (B,k).  == reference get_child_states (act.py:266-275) with k>1, T=1, plus the
    per-game form of remove_null_actions (utils.py:191-194).  ``want_keys`` (or a ``keys`` int64 (B,k) tensor) also
    returns the 64-bit key of every child (== ``state_hash`` of the child; the state_to_str keys of act.py:188-190):
    (children, done, changed, keys)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    if actions.dim() != 3:
        raise TensorGameError("expand", -1, "actions must be (B,k,3S)")
    k = actions.shape[1]
    actions = _tokens(actions, (B, k), S, dev, "actions")
    if out is None:
        out = alloc_states(B * k, S, dev, zero=False).unflatten(0, (B, k))
    if out.dtype != torch.int8 or tuple(out.shape) != (B, k, S, S, S) or out.device != dev:
        raise TensorGameError("expand", -1, f"out must be int8 {(B, k, S, S, S)} on {dev}")
    # child (b, i) lives at base + (b*k + i) * ostride: the (B, k) dims must collapse to ONE stride.  No
    # flatten() here -- on a view that cannot be flattened it would silently copy and the kernel would write
    # through the original pointer with the copy's strides
    if out.stride()[2:] != (S * S, S, 1):
        raise TensorGameError("expand", -1, "out: each child must be C-contiguous (S,S,S)")
    ostride = out.stride(1) if k > 1 else (out.stride(0) if B > 1 else max(out.stride(1), S ** 3))
    if ostride < S ** 3 or (B > 1 and k > 1 and out.stride(0) != k * ostride):
        raise TensorGameError("expand", -1, f"out: children must be evenly spaced (strides {out.stride()[:2]}); "
                                            "a slice like big[:, :k] of a wider buffer is not")
    done = _out(done, (B, k), torch.uint8, dev, "done")
    changed = _out(changed, (B, k), torch.uint8, dev, "changed")
    overflow = _flag(overflow, (B, k), torch.uint8, dev, "overflow")
    ptrs = (_ptr(state), _ptr(out), _ptr(actions), _ptr(done), _ptr(changed), _ptr(overflow))
    sizes = (B, S, k, stride, ostride, int(shift))
    if not want_keys and keys is None:
        _launch(dev, "tg_expand_i8", *ptrs, *sizes)
        return out, done, changed
    keys = _out(keys, (B, k), torch.int64, dev, "keys")
    _launch(dev, "tg_expand_keyed_i8", *ptrs, _ptr(keys), *sizes)
    return out, done, changed, keys


def done(state, want_nnz: bool = False):
    """done[b] = head of game b is all zero (== tensor_factorized, utils.py:181-188, per game);
    nnz[b] = number of non-zero entries (the rank bound of training.py:266)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    d = torch.empty((B,), dtype=torch.uint8, device=dev)
    nnz = torch.empty((B,), dtype=torch.int32, device=dev) if want_nnz else None
    _launch(dev, "tg_done_i8", _ptr(state), _ptr(d), _ptr(nnz), B, S, stride)
    return (d, nnz) if want_nnz else d


def reset_matmul(out, n: int):
    """every game <- <n,n,n> (== build_matmul_tensor(1,n,n,n)[0], utils.py:143-161)."""
    B, S, stride = _state_layout(out, "out")
    if S != n * n:
        raise TensorGameError("reset_matmul", -1, f"S={S} != n*n={n * n}")
    _launch(out.device, "tg_reset_matmul_i8", _ptr(out), B, int(n), stride)
    return out


def reset_broadcast(out, start):
    """every game <- start (int8 (S,S,S) on the same device)."""
    B, S, stride = _state_layout(out, "out")
    _need_gpu(start, "start")
    if start.dtype != torch.int8 or tuple(start.shape) != (S, S, S) or start.device != out.device:
        raise TensorGameError("reset_broadcast", -1, f"start must be int8 {(S, S, S)} on {out.device}")
    start = start.contiguous()
    _launch(out.device, "tg_reset_broadcast_i8", _ptr(start), _ptr(out), B, S, stride)
    return out


def gen_from_factors(actions, S: int, out=None, overflow=None, shift: int = 1):
    """target[b] = sum_r tensor(actions[b][r]); actions int8 (B,R,3S).  The deterministic half
    of create_synthetic_demo (utils.py:218-232) / uvw_to_demo (utils.py:40-53)."""
    _need_gpu(actions, "actions")
    if actions.dim() != 3:
        raise TensorGameError("gen_from_factors", -1, "actions must be (B,R,3S)")
    B, R = actions.shape[:2]
    dev = actions.device
    actions = _tokens(actions, (B, R), S, dev, "actions")
    if out is None:
        out = alloc_states(B, S, dev, zero=False)
    Bo, So, stride = _state_layout(out, "out")
    if (Bo, So) != (B, S) or out.device != dev:
        raise TensorGameError("gen_from_factors", -1, "out shape/device mismatch")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    _launch(dev, "tg_gen_from_factors_i8", _ptr(actions), _ptr(out), _ptr(overflow), B, S, R, stride, int(shift))
    return out


def categorical_thresholds(probs: Sequence[float]) -> np.ndarray:
    """uint32 cdf thresholds of a categorical distribution (normalised like
    torch.distributions.Categorical, reference utils.py:198): a 32-bit draw d selects
    values[#{t : d >= t}]."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 1 or len(p) < 1 or len(p) > TG_MAX_VALUES or (p < 0).any() or p.sum() <= 0:
        raise TensorGameError("categorical_thresholds", -1, f"probs must be 1..{TG_MAX_VALUES} non-negative weights")
    cdf = np.cumsum(p) / p.sum()
    return np.minimum(np.floor(cdf[:-1] * 4294967296.0 + 0.5), 4294967295.0).astype(np.uint32)


def _dist(values, probs, name):
    vals = np.asarray(values, dtype=np.int64)
    if vals.ndim != 1 or len(vals) != len(probs) or (np.abs(vals) > 127).any():
        raise TensorGameError(name, -1, "values must be int8 and match probs")
    thr = categorical_thresholds(probs)
    p = np.asarray(probs, dtype=np.float64)
    if not ((vals != 0) & (p > 0)).any():
        raise TensorGameError(name, -1, "the distribution can never draw a non-zero factor value")
    vals8 = vals.astype(np.int8)
    return (thr, vals8, thr.ctypes.data_as(C.c_void_p), vals8.ctypes.data_as(C.c_void_p), len(vals8))


def gen_demos(B: int, S: int, R: int, device, values=(-1, 0, 1), probs=(0.15, 0.7, 0.15), shift: int = 1,
              seed: int = 0, game_id_offset: int = 0, basis=None, target=None, actions=None, overflow=None):
    """The synthetic-demonstration generator (== create_synthetic_demo, utils.py:203-233 /
    SyntheticDemoDataset._create_synthetic_demos, datasets.py:124-142).  Returns
    (actions int8 (B,R,3S), target int8 (B,S,S,S)).  Deterministic in (seed, global game id)."""
    dev = torch.device(device)
    thr, vals, thr_p, val_p, nv = _dist(values, probs, "gen_demos")
    if target is None:
        target = alloc_states(B, S, dev, zero=False)
    Bo, So, stride = _state_layout(target, "target")
    if actions is None:
        actions = torch.empty((B, R, 3 * S), dtype=torch.int8, device=dev)
    if (Bo, So) != (B, S) or tuple(actions.shape) != (B, R, 3 * S) or actions.dtype != torch.int8 \
            or not actions.is_contiguous() or actions.device != target.device:
        raise TensorGameError("gen_demos", -1, "target/actions shape, dtype or device mismatch")
    dev = target.device
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    if basis is not None:
        if basis.dtype != torch.int8 or tuple(basis.shape) != (B, 3, S, S) or basis.device != dev:
            raise TensorGameError("gen_demos", -1, f"basis must be int8 {(B, 3, S, S)} on {dev}")
        basis = basis.contiguous()
    _launch(dev, "tg_gen_demos_i8", _ptr(target), _ptr(actions), _ptr(overflow), B, S, R, thr_p, val_p, nv,
            int(shift), C.c_uint64(_u64(seed)), C.c_uint64(game_id_offset), _ptr(basis), stride)
    return actions, target


def sample_basis(B: int, S: int, device, values=(-1, 0, 1), probs=None, seed: int = 0,
                 game_id_offset: int = 0, want_factors: bool = False):
    """Three random unimodular matrices per game, P = L @ U (not in the reference).
    ``probs`` are the off-diagonal value weights of L and U; the default keeps about 0.4 non-zero
    off-diagonal entries per row (p = min(0.15, 0.4/S) each for -1 and +1), dense enough to mix
    the basis and sparse enough that transformed int8 targets rarely overflow."""
    dev = torch.device(device)
    if probs is None:
        p = min(0.15, 0.4 / S)
        probs = (p, 1.0 - 2.0 * p, p)
    thr, vals, thr_p, val_p, nv = _dist(values, probs, "sample_basis")
    if (S * vals.astype(np.int64) ** 2 > 127).any():  # the library enforces the same rule
        raise TensorGameError("sample_basis", -1, f"every value needs S*v^2 <= 127 at S={S}: P = L @ U is emitted as int8")
    P = torch.empty((B, 3, S, S), dtype=torch.int8, device=dev)
    L = torch.empty_like(P) if want_factors else None
    U = torch.empty_like(P) if want_factors else None
    _launch(P.device, "tg_sample_basis_i8", _ptr(P), _ptr(L), _ptr(U), B, S, thr_p, val_p, nv,
            C.c_uint64(_u64(seed)), C.c_uint64(game_id_offset))
    return (P, L, U) if want_factors else P


def change_basis(state, basis, out=None, overflow=None):
    """T'[a,b,c] = sum A[a,i] B[b,j] C[c,k] T[i,j,k]; basis int32 (B,3,S,S)."""
    B, S, stride = _state_layout(state, "state")
    dev = state.device
    if basis.dtype != torch.int32 or tuple(basis.shape) != (B, 3, S, S) or basis.device != dev:
        raise TensorGameError("change_basis", -1, f"basis must be int32 {(B, 3, S, S)} on {dev}")
    basis = basis.contiguous()
    out = _out_states(out, state, B, S, stride, "change_basis")
    if out.data_ptr() == state.data_ptr():
        raise TensorGameError("change_basis", -1, "in-place change of basis is not supported")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    _launch(dev, "tg_change_basis_i8", _ptr(state), _ptr(basis), _ptr(out), _ptr(overflow), B, S, stride)
    return out


def alloc_ring(B: int, S: int, T: int, device, pad_to: int = 16) -> torch.Tensor:
    """Zeroed history ring int8 (B,T,S,S,S): T frame slots per game, each padded to ``pad_to`` bytes.
    ``ring[:, s]`` is a valid (B,S,S,S) state for every entry point (game stride = T * frame stride)."""
    n = S ** 3
    fs = -(-n // pad_to) * pad_to
    buf = torch.zeros((B, T, fs), dtype=torch.int8, device=device)
    return buf[:, :, :n].unflatten(2, (S, S, S))


# dtype codes of the model input (include/tensor_game.h); items may also be int8
_FLOAT_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_ITEM_DTYPES = {**_FLOAT_DTYPES, torch.int8: 3}


def _ring_layout(ring, fn: str) -> Tuple[int, int, int, int, int]:
    """(B, T, S, frame_stride, game_stride) in bytes of an int8 (B,T,S,S,S) history ring whose frames are dense (the
    layout of ``alloc_ring``; a single frame or a single game has no stride of its own to read)."""
    _need_gpu(ring, "ring")
    if ring.dtype != torch.int8 or ring.dim() != 5 or not (ring.shape[2] == ring.shape[3] == ring.shape[4]):
        raise TensorGameError(fn, -1, f"ring must be int8 (B,T,S,S,S), got {ring.dtype} {tuple(ring.shape)}")
    B, T, S = ring.shape[0], ring.shape[1], ring.shape[2]
    if ring.stride()[2:] != (S * S, S, 1):
        raise TensorGameError(fn, -1, "each frame must be C-contiguous (S,S,S)")
    fs = ring.stride(1) if T > 1 else S ** 3
    gs = ring.stride(0) if B > 1 else max(ring.stride(0), (T - 1) * fs + S ** 3)
    return B, T, S, fs, gs


def _model_input(out, scalars, shape: Tuple[int, ...], dtype, dev, fn: str):
    """The model input ``out`` (B,T,S,S,S) of ``dtype`` and its ``scalars`` float32 (B,1), each allocated when it is
    not given."""
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise TensorGameError(fn, -1, "out must be contiguous (B,T,S,S,S) of the requested dtype")
    return out, _out(scalars, (shape[0], 1), torch.float32, dev, "scalars")


def emit_frames(ring, head_slot: int, t_step: float = 0.0, dtype=torch.float32, out=None, scalars=None):
    """(B,T,S,S,S) model input from the history ring, newest frame first, plus the (B,1) scalars.
    == the history shift of get_child_states (act.py:271-274) + get_scalars (utils.py:22-37)."""
    B, T, S, fs, gs = _ring_layout(ring, "emit_frames")
    if dtype not in _FLOAT_DTYPES:
        raise TensorGameError("emit_frames", -1, "dtype must be float32, float16 or bfloat16")
    dev = ring.device
    out, scalars = _model_input(out, scalars, (B, T, S, S, S), dtype, dev, "emit_frames")
    _launch(dev, "tg_emit_frames", _ptr(ring), _ptr(out), _ptr(scalars), _FLOAT_DTYPES[dtype], B, S, T,
            int(head_slot) % T, C.c_float(float(t_step)), fs, gs)
    return out, scalars


def step_emit(ring, head_slot: int, actions, t_step: float = 0.0, dtype=torch.float32, out=None, scalars=None, done=None,
              overflow=None, shift: int = 1):
    """One env step on the history ring and the model input of the new state, in one call (the fused form of
    ``step`` + ``emit_frames``; one kernel at S=4).  The new head is written into slot ``(head_slot + 1) % T``.
    Returns (out (B,T,S,S,S), scalars (B,1), done (B,), new_head_slot)."""
    B, T, S, fs, gs = _ring_layout(ring, "step_emit")
    if dtype not in _FLOAT_DTYPES:
        raise TensorGameError("step_emit", -1, "dtype must be float32, float16 or bfloat16")
    dev = ring.device
    actions = _tokens(actions, (B,), S, dev, "actions")
    out, scalars = _model_input(out, scalars, (B, T, S, S, S), dtype, dev, "step_emit")
    done = _out(done, (B,), torch.uint8, dev, "done")
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    head = int(head_slot) % T
    _launch(dev, "tg_step_emit", _ptr(ring), _ptr(actions), _ptr(out), _ptr(scalars), _ptr(done), _ptr(overflow),
            _FLOAT_DTYPES[dtype], B, S, T, head, C.c_float(float(t_step)), fs, gs, int(shift))
    return out, scalars, done, (head + 1) % T


def _item_idx(idx, dev, fn: str) -> torch.Tensor:
    """The flat item indices int64 (N,) on ``dev``, made contiguous."""
    _need_gpu(idx, "idx")
    if idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != dev:
        raise TensorGameError(fn, -1, f"idx must be int64 (N,) on {dev}, got {idx.dtype} {tuple(idx.shape)} on {idx.device}")
    return idx if idx.is_contiguous() else idx.contiguous()


def _item_outputs(N: int, T: int, S: int, dtype, dev, fn: str, out, scalars, actions, rewards, overflow, status):
    """The outputs of N items in the layout of ``demo_items``: (dtype code, frames (N,T,S,S,S) of ``dtype``, scalars
    float32 (N,1), actions int8 (N,3S), rewards float32 (N,1)), each allocated when it is not given, and the optional
    overflow uint8 (N,) and status uint32 (1,)."""
    if dtype not in _ITEM_DTYPES:
        raise TensorGameError(fn, -1, "dtype must be float32, float16, bfloat16 or int8")
    if out is None:
        out = torch.empty((N, T, S, S, S), dtype=dtype, device=dev)
    elif out.dtype != dtype or tuple(out.shape) != (N, T, S, S, S) or not out.is_contiguous() or out.device != dev:
        raise TensorGameError(fn, -1, "out must be contiguous (N,T,S,S,S) of the requested dtype")
    return (_ITEM_DTYPES[dtype], out,
            _out(scalars, (N, 1), torch.float32, dev, "scalars"),
            _out(actions, (N, 3 * S), torch.int8, dev, "actions"),
            _out(rewards, (N, 1), torch.float32, dev, "rewards"),
            _flag(overflow, (N,), torch.uint8, dev, "overflow"),
            _flag(status, (1,), torch.uint32, dev, "status"))


def demo_items(tokens, targets, idx, T: int, dtype=torch.float32, out=None, scalars=None, actions=None, rewards=None,
               overflow=None, status=None, shift: int = 1):
    """Items of a demo set at flat indices ``idx`` (int64 (N,), item n = demo idx // R at action index idx % R), the
    ``__getitem__`` of SyntheticDemoDataset (datasets.py:78-122) for a whole shuffled batch in one launch (no host sync).
    tokens int8 (n_demos,R,3S); targets int8 (n_demos,S,S,S), game stride >= S^3 (``alloc_states`` padding accepted).
    Returns (frames (N,T,S,S,S) of ``dtype`` (float32, float16, bfloat16 or int8), scalars float32 (N,1) = R - k,
    actions int8 (N,3S), rewards float32 (N,1) = -(k+1)).  ``overflow`` uint8 (N,) is set where an exact frame value
    left int8; ``status`` uint32 (1,) gets bit 0 for an index outside [0, n_demos*R) (that item is all zero)."""
    B, S, stride = _state_layout(targets, "targets")
    dev = targets.device
    _need_gpu(tokens, "tokens")
    if tokens.dim() != 3 or tokens.shape[0] != B:
        raise TensorGameError("demo_items", -1, f"tokens must be int8 (n_demos,R,3S) with n_demos={B}, got {tuple(tokens.shape)}")
    R = tokens.shape[1]
    tokens = _tokens(tokens, (B, R), S, dev, "tokens")
    idx = _item_idx(idx, dev, "demo_items")
    N = idx.shape[0]
    code, out, scalars, actions, rewards, overflow, status = _item_outputs(
        N, T, S, dtype, dev, "demo_items", out, scalars, actions, rewards, overflow, status)
    _launch(dev, "tg_demo_items", _ptr(tokens), _ptr(targets), B, R, S, stride, _ptr(idx), N, int(T), code,
            _ptr(out), _ptr(scalars), _ptr(actions), _ptr(rewards), _ptr(overflow), _ptr(status), int(shift))
    return out, scalars, actions, rewards


def symmetry_sample(N: int, S: int, device, seed: int = 0, item_offset: int = 0, modes: bool = True, perms: bool = True,
                    signs: bool = True, out=None) -> torch.Tensor:
    """One element of the symmetry group per item (include/tensor_game_symmetry.h): uint8 (N,3S+1) rows, byte 0 the
    mode permutation's code, byte 1 + m*S + a = pi_m[a] | 0x80 for a negative sign.  Keyed by the global item id
    ``item_offset + n``, so any split of an id range gives the same rows.  A part switched off (``modes``, ``perms``,
    ``signs``) is the identity; the other parts do not change with it."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise TensorGameError("symmetry_sample", -1, f"device must be a ROCm device (got {dev}); there is no CPU path")
    N, S = int(N), int(S)
    if N < 0 or not 1 <= S <= TG_MAX_S:
        raise TensorGameError("symmetry_sample", -1, f"N={N} must be >= 0 and S={S} in [1,{TG_MAX_S}]")
    if out is None:
        out = torch.empty((N, 3 * S + 1), dtype=torch.uint8, device=dev)
    else:
        _need_gpu(out, "out")
        _flag(out, (N, 3 * S + 1), torch.uint8, out.device, "out")
    flags = (_lib.TG_SYM_MODES if modes else 0) | (_lib.TG_SYM_PERMS if perms else 0) | (_lib.TG_SYM_SIGNS if signs else 0)
    _launch(out.device, "tg_symmetry_sample", _ptr(out), N, S, C.c_uint64(_u64(seed)), C.c_uint64(_u64(item_offset)), flags)
    return out


def symmetry_apply(state_i8, action_i8, sym, dtype=torch.float32, shift: int = 1, overflow=None, status=None, out=None,
                   actions=None):
    """``sym[n]`` applied to item n (include/tensor_game_symmetry.h): state_i8 int8 (N,T,S,S,S) and action_i8 int8
    (N,3S) (or None) -> (state (N,T,S,S,S) of ``dtype`` (float32, float16, bfloat16 or int8), action int8 (N,3S) or
    None; ``out`` / ``actions`` receive them when given).  Out of place, one launch, no host sync.  ``overflow`` uint8
    (N,) is set where a negation left int8; ``status`` uint32 (1,) gets bit 0 for a bad row of ``sym`` (that item is
    all zero)."""
    fn = "symmetry_apply"
    _need_gpu(state_i8, "state_i8")
    if state_i8.dtype != torch.int8 or state_i8.dim() != 5 or not (state_i8.shape[2] == state_i8.shape[3] == state_i8.shape[4]):
        raise TensorGameError(fn, -1, f"state_i8 must be int8 (N,T,S,S,S), got {state_i8.dtype} {tuple(state_i8.shape)}")
    if not state_i8.is_contiguous():
        raise TensorGameError(fn, -1, "state_i8 must be C-contiguous")
    N, T, S = state_i8.shape[0], state_i8.shape[1], state_i8.shape[2]
    dev = state_i8.device
    if dtype not in _ITEM_DTYPES:
        raise TensorGameError(fn, -1, "dtype must be float32, float16, bfloat16 or int8")
    _need_gpu(sym, "sym")
    sym = _flag(sym, (N, 3 * S + 1), torch.uint8, dev, "sym")
    actions_out = None
    if action_i8 is not None:
        action_i8 = _tokens(action_i8, (N,), S, dev, "action_i8")
        actions_out = _out(actions, (N, 3 * S), torch.int8, dev, "actions")
    if out is None:
        out = torch.empty((N, T, S, S, S), dtype=dtype, device=dev)
    elif out.dtype != dtype or tuple(out.shape) != (N, T, S, S, S) or not out.is_contiguous() or out.device != dev:
        raise TensorGameError(fn, -1, "out must be contiguous (N,T,S,S,S) of the requested dtype")
    overflow = _flag(overflow, (N,), torch.uint8, dev, "overflow")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_symmetry_apply", _ptr(state_i8), _ptr(action_i8), _ptr(sym), N, T, S, int(shift), _ITEM_DTYPES[dtype],
            _ptr(out), _ptr(actions_out), _ptr(overflow), _ptr(status))
    return out, actions_out


def _list_shape(tokens, fn: str, name: str = "tokens", lead: str = "M") -> Tuple[int, int, int]:
    """(M, K, S) of the tokens int8 (M,K,3S) of M action lists."""
    if tokens.dtype != torch.int8 or tokens.dim() != 3 or tokens.shape[2] % 3:
        raise TensorGameError(fn, -1, f"{name} must be int8 ({lead},K,3S), got {tokens.dtype} {tuple(tokens.shape)}")
    return tokens.shape[0], tokens.shape[1], tokens.shape[2] // 3


def _list_tokens(tokens, fn: str):
    """(tokens made contiguous, M, K, S, device) of M action lists on a ROCm device."""
    _need_gpu(tokens, "tokens")
    return (tokens if tokens.is_contiguous() else tokens.contiguous(), *_list_shape(tokens, fn), tokens.device)


def _list_lengths(lengths, M: int, dev) -> torch.Tensor:
    _need_gpu(lengths, "lengths")
    return _flag(lengths, (M,), torch.int64, dev, "lengths")


def _list_targets(targets, residual_nnz, M: int, S: int, dev, fn: str):
    """The targets of the canon entries, made contiguous; None (no verification) refuses a ``residual_nnz`` output."""
    if targets is None:
        if residual_nnz is not None:
            raise TensorGameError(fn, -1, "residual_nnz needs targets")
        return None
    _need_gpu(targets, "targets")
    if targets.dtype != torch.int8 or tuple(targets.shape) != (M, S, S, S) or targets.device != dev:
        raise TensorGameError(fn, -1, f"targets must be int8 {(M, S, S, S)} on {dev}, got {targets.dtype} "
                                      f"{tuple(targets.shape)} on {targets.device}")
    return targets if targets.is_contiguous() else targets.contiguous()


def _canon_outputs(canon, rank, key, residual_nnz, verify: bool, M: int, K: int, S: int, dev):
    """(canon, rank, key, residual_nnz) of the canon entries; residual_nnz only with targets (``verify``)."""
    canon = _out(canon, (M, K, 3 * S), torch.int8, dev, "canon")
    rank = _out(rank, (M,), torch.int32, dev, "rank")
    key = _out(key, (M,), torch.int64, dev, "key")
    if verify:
        residual_nnz = _out(residual_nnz, (M,), torch.int32, dev, "residual_nnz")
    return canon, rank, key, residual_nnz


def solution_check(M: int, K: int, S: int, shift: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_solution_canon takes these sizes.  Host only."""
    call("tg_solution_check", int(M), int(K), int(S), int(shift))


def solution_canon(targets, tokens, lengths, shift: int = 1, canon=None, rank=None, key=None, residual_nnz=None,
                   status=None):
    """Verify and canonicalise M action lists in one launch (include/tensor_game_solutions.h).  tokens int8 (M,K,3S)
    and lengths int64 (M,) as ``RolloutResult.solutions()`` returns them; targets int8 (M,S,S,S) (the start heads) or
    None.  Returns (canon int8 (M,K,3S): the kept terms in canonical order, zero rows behind them; rank int32 (M,);
    key int64 (M,) holding the 64 bits; residual_nnz int32 (M,): the non-zero entries of target - sum of the ORIGINAL
    terms in exact arithmetic, 0 = proven; None when ``targets`` is None).  A row with a length outside [0,K] or a
    negation that leaves int8 is all zero, with rank 0, key 0 and residual_nnz -1, and sets bit 0 / bit 1 of ``status``
    uint32 (1,).  No host sync."""
    fn = "solution_canon"
    tokens, M, K, S, dev = _list_tokens(tokens, fn)
    solution_check(M, K, S, shift)
    targets = _list_targets(targets, residual_nnz, M, S, dev, fn)
    lengths = _list_lengths(lengths, M, dev)
    canon, rank, key, residual_nnz = _canon_outputs(canon, rank, key, residual_nnz, targets is not None, M, K, S, dev)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_solution_canon", _ptr(targets), _ptr(tokens), _ptr(lengths), M, K, S, int(shift), _ptr(canon),
            _ptr(rank), _ptr(key), _ptr(residual_nnz), _ptr(status))
    return canon, rank, key, residual_nnz


def orbit_check(M: int, K: int, S: int, shift: int = 1, G: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_orbit_canon takes these sizes.  Host only."""
    call("tg_orbit_check", int(M), int(K), int(S), int(shift), int(G))


def _group_rows(sym, S: int, dev, fn: str) -> torch.Tensor:
    """The set of group elements of the orbit entries: contiguous uint8 (G,3S+1) on ``dev``."""
    _need_gpu(sym, "sym")
    if sym.dtype != torch.uint8 or sym.dim() != 2 or sym.shape[1] != 3 * S + 1 or sym.shape[0] < 1:
        raise TensorGameError(fn, -1, f"sym must be uint8 (G,{3 * S + 1}) with G >= 1, got {sym.dtype} {tuple(sym.shape)}")
    return _flag(sym, tuple(sym.shape), torch.uint8, dev, "sym")


def orbit_fixes(targets, sym, fixes=None, status=None) -> torch.Tensor:
    """Whether every element of a set fixes each target, in one launch (include/tensor_game_orbits.h).  targets int8
    (M,S,S,S); sym uint8 (G,3S+1) in the encoding of ``symmetry_sample``.  Returns fixes uint8 (M,): 1 where
    ``symmetry_apply(target, g) == target`` for every row g.  A bad row of ``sym`` (mode code above 5, an index >= S)
    sets bit 0 of ``status`` uint32 (1,) and makes every flag 0.  No host sync."""
    fn = "orbit_fixes"
    _need_gpu(targets, "targets")
    if targets.dtype != torch.int8 or targets.dim() != 4 or not (targets.shape[1] == targets.shape[2] == targets.shape[3]):
        raise TensorGameError(fn, -1, f"targets must be int8 (M,S,S,S), got {targets.dtype} {tuple(targets.shape)}")
    M, S, dev = targets.shape[0], targets.shape[1], targets.device
    targets = targets if targets.is_contiguous() else targets.contiguous()
    sym = _group_rows(sym, S, dev, fn)
    fixes = _out(fixes, (M,), torch.uint8, dev, "fixes")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_orbit_fixes", _ptr(targets), M, S, _ptr(sym), sym.shape[0], _ptr(fixes), _ptr(status))
    return fixes


def orbit_workspace_size(M: int, K: int, S: int, G: int) -> int:
    """Bytes of workspace with which ``orbit_canon`` spreads the set over several workgroups per list (0: it does not)."""
    n = C.c_int64(0)
    call("tg_orbit_workspace_size", int(M), int(K), int(S), int(G), C.byref(n))
    return int(n.value)


def orbit_canon(targets, tokens, lengths, sym, shift: int = 1, canon=None, rank=None, key=None, residual_nnz=None,
                which=None, stab=None, status=None, workspace=None):
    """``solution_canon`` modulo a set of symmetries (include/tensor_game_orbits.h): per list the smallest canonical
    form over g.X, g a row of ``sym`` uint8 (G,3S+1).  Arguments and the first four results as ``solution_canon``
    (the residual is that of the ORIGINAL list); then which int32 (M,): the smallest row index attaining the minimum,
    and stab int32 (M,): how many rows attain it.  ``status`` uint32 (1,) gets bit 0 for a bad length, bit 1 for a token
    that leaves int8 under some g, bit 2 for a bad row of ``sym`` (every list is bad then); a bad list is all zero with
    rank 0, key 0, residual_nnz -1, which -1, stab 0.  ``workspace``: None allocates what ``orbit_workspace_size`` asks
    for (uint8, a small batch is then spread over the device: two launches), False uses none (one launch), or a uint8
    tensor of that size.  The outputs do not depend on it.  No host sync."""
    fn = "orbit_canon"
    tokens, M, K, S, dev = _list_tokens(tokens, fn)
    sym = _group_rows(sym, S, dev, fn)
    G = sym.shape[0]
    orbit_check(M, K, S, shift, G)
    targets = _list_targets(targets, residual_nnz, M, S, dev, fn)
    lengths = _list_lengths(lengths, M, dev)
    canon, rank, key, residual_nnz = _canon_outputs(canon, rank, key, residual_nnz, targets is not None, M, K, S, dev)
    which =_out(which, (M,), torch.int32, dev, "which")
    stab = _out(stab, (M,), torch.int32, dev, "stab")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    if workspace is False:
        workspace = None
    else:
        with torch.cuda.device(dev):  # the plan follows the device the launch goes to
            need = orbit_workspace_size(M, K, S, G)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        else:
            _need_gpu(workspace, "workspace")
            if workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.numel() < need or workspace.device != dev \
                    or not workspace.is_contiguous():
                raise TensorGameError(fn, -1, f"workspace must be contiguous uint8 of at least {need} bytes on {dev}")
            workspace = workspace if need else None
    _launch(dev, "tg_orbit_canon", _ptr(targets), _ptr(tokens), _ptr(lengths), M, K, S, int(shift), _ptr(sym), G,
            _ptr(canon), _ptr(rank), _ptr(key), _ptr(residual_nnz), _ptr(which), _ptr(stab), _ptr(status), _ptr(workspace),
            0 if workspace is None else workspace.numel())
    return canon, rank, key, residual_nnz, which, stab


def basis_inverse_check(N: int, S: int) -> None:
    """Raise TensorGameError (naming the argument) unless tg_basis_inverse_i32 takes these sizes.  Host only."""
    call("tg_basis_inverse_check", int(N), int(S))


def solution_rebase_check(M: int, K: int, S: int, G: int, shift: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_solution_rebase takes these sizes.  Host only."""
    call("tg_solution_rebase_check", int(M), int(K), int(S), int(G), int(shift))


def _optional_bad(bad, shape, dev):
    """The ``bad`` output of the two entries below: allocated when None, not written at all (NULL) when False."""
    return None if bad is False else _out(bad, shape, torch.uint8, dev, "bad")


def basis_inverse(lower, upper, inv=None, bad=None, status=None):
    """The exact integer inverses of N sampled bases in one launch (include/tensor_game_bases.h).  lower, upper int8
    (N,3,S,S): the L and U of ``sample_basis(want_factors=True)``, P = L @ U.  Returns (inv int32 (N,3,S,S) =
    U^-1 @ L^-1, bad uint8 (N,)).  A triple with a diagonal entry other than +-1 (bit 0 of ``status`` uint32 (1,)) or
    whose inverse leaves the accepted range (bit 1) is all zero and has bad = 1.  ``bad=False`` passes no flag buffer
    (None is returned in its place).  No host sync."""
    fn = "basis_inverse"
    for t, name in ((lower, "lower"), (upper, "upper")):
        if t.dtype != torch.int8 or t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3]:
            raise TensorGameError(fn, -1, f"{name} must be int8 (N,3,S,S), got {t.dtype} {tuple(t.shape)}")
    if upper.shape != lower.shape:
        raise TensorGameError(fn, -1, f"upper must have the shape of lower {tuple(lower.shape)}, got {tuple(upper.shape)}")
    _need_gpu(lower, "lower")
    _need_gpu(upper, "upper")
    N, S, dev = lower.shape[0], lower.shape[2], lower.device
    if upper.device != dev:
        raise TensorGameError(fn, -1, f"upper is on {upper.device}, lower on {dev}")
    basis_inverse_check(N, S)
    lower = lower if lower.is_contiguous() else lower.contiguous()
    upper = upper if upper.is_contiguous() else upper.contiguous()
    inv = _out(inv, (N, 3, S, S), torch.int32, dev, "inv")
    bad = _optional_bad(bad, (N,), dev)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_basis_inverse_i32", _ptr(lower), _ptr(upper), N, S, _ptr(inv), _ptr(bad), _ptr(status))
    return inv, bad


def solution_rebase(tokens, lengths, mats, index=None, shift: int = 1, tokens_out=None, lengths_out=None, bad=None,
                    status=None):
    """Apply a matrix triple to the factors of every term of M action lists in one launch
    (include/tensor_game_bases.h): (u,v,w) -> (A u, B v, C w) with (A,B,C) = mats[index[m]].  tokens int8 (M,K,3S) and
    lengths int64 (M,) as ``solutions()`` returns them; mats int32 (G,3,S,S); index int64 (M,), or None: row m uses
    triple m (G == M).  Returns (tokens_out int8 (M,K,3S), zero rows behind each list; lengths_out int64 (M,); bad uint8
    (M,)).  A row with a length outside [0,K] (bit 0 of ``status`` uint32 (1,)), an index outside [0,G) (bit 1) or a
    mapped token outside int8 (bit 2) is all zero, with length 0 and bad = 1.  With ``BasisSet.inverse`` as ``mats``
    this carries lists found in a changed basis back; with ``BasisSet.forward`` it moves known lists into it.
    ``bad=False`` passes no flag buffer.  Out of place; no host sync."""
    fn = "solution_rebase"
    M, K, S = _list_shape(tokens, fn)  # (this entry checks every shape before any device, in words of its own)
    if mats.dtype != torch.int32 or mats.dim() != 4 or tuple(mats.shape[1:]) != (3, S, S):
        raise TensorGameError(fn, -1, f"mats must be int32 (G,3,{S},{S}), got {mats.dtype} {tuple(mats.shape)}")
    G = mats.shape[0]
    if lengths.dtype != torch.int64 or tuple(lengths.shape) != (M,):
        raise TensorGameError(fn, -1, f"lengths must be int64 {(M,)}, got {lengths.dtype} {tuple(lengths.shape)}")
    if index is None:
        if G != M:
            raise TensorGameError(fn, -1, f"index must be given unless mats has one triple per row: G={G}, M={M}")
    elif index.dtype != torch.int64 or tuple(index.shape) != (M,):
        raise TensorGameError(fn, -1, f"index must be int64 {(M,)}, got {index.dtype} {tuple(index.shape)}")
    _need_gpu(tokens, "tokens")
    dev = tokens.device
    for t, name in ((lengths, "lengths"), (mats, "mats"), (index, "index")):
        if t is not None and t.device != dev:
            raise TensorGameError(fn, -1, f"{name} is on {t.device}, tokens on {dev}")
    solution_rebase_check(M, K, S, G, shift)
    tokens = tokens if tokens.is_contiguous() else tokens.contiguous()
    mats = mats if mats.is_contiguous() else mats.contiguous()
    lengths = lengths if lengths.is_contiguous() else lengths.contiguous()
    if index is not None and not index.is_contiguous():
        index = index.contiguous()
    tokens_out = _out(tokens_out, (M, K, 3 * S), torch.int8, dev, "tokens_out")
    if M and tokens_out.data_ptr() == tokens.data_ptr():
        raise TensorGameError(fn, -1, "tokens_out must not be tokens: in-place operation is not supported")
    lengths_out = _out(lengths_out, (M,), torch.int64, dev, "lengths_out")
    bad = _optional_bad(bad, (M,), dev)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_solution_rebase", _ptr(tokens), _ptr(lengths), _ptr(mats), _ptr(index), M, K, S, G, int(shift),
            _ptr(tokens_out), _ptr(lengths_out), _ptr(bad), _ptr(status))
    return tokens_out, lengths_out, bad


def state_hash(state) -> torch.Tensor:
    """64-bit key per game (int64 tensor holding the uint64 bits): the transposition-table key that
    replaces state_to_str (utils.py:164-169).  Equal states <=> equal keys (up to 2^-64 collisions)."""
    B, S, stride = _state_layout(state, "state")
    out = torch.empty((B,), dtype=torch.int64, device=state.device)
    _launch(state.device, "tg_hash_u64", _ptr(state), _ptr(out), B, S, stride)
    return out


def alloc_seen_table(capacity: int, device) -> torch.Tensor:
    """An empty transposition table for ``seen``: int64 (capacity,) zeros, capacity a power of two (keep it at most
    half full)."""
    if capacity < 2 or capacity & (capacity - 1):
        raise TensorGameError("alloc_seen_table", -1, "capacity must be a power of two >= 2")
    return torch.zeros((capacity,), dtype=torch.int64, device=device)


def seen(keys, table, mask=None, insert: bool = False, status=None, fresh=None) -> torch.Tensor:
    """fresh[i] = mask[i] and keys[i] not in table (as it was BEFORE the call); with ``insert`` every masked key is in
    the table afterwards.  == the tree filter of extend_tree (act.py:188-195: ``c not in new_mc_tree``) and the
    recording of the expanded state's key (act.py:209-211), on the 64-bit keys of ``state_hash``.  ``keys`` may have any
    shape (int64 bits of the uint64 keys); ``mask`` uint8 of the same shape (e.g. ``changed`` of ``expand``);
    ``status`` int32 (1,): bit 0 set when the table was full.  Returns fresh (uint8, shape of keys)."""
    _need_gpu(keys, "keys")
    _need_gpu(table, "table")
    dev = keys.device
    if keys.dtype != torch.int64 or not keys.is_contiguous():
        raise TensorGameError("seen", -1, "keys must be contiguous int64 (the bits of the uint64 keys)")
    if table.dtype != torch.int64 or table.dim() != 1 or not table.is_contiguous() or table.device != dev:
        raise TensorGameError("seen", -1, f"table must be a contiguous int64 vector on {dev} (ops.alloc_seen_table)")
    n = keys.numel()
    mask = _flag(mask, tuple(keys.shape), torch.uint8, dev, "mask")
    fresh = _out(fresh, tuple(keys.shape), torch.uint8, dev, "fresh")
    if status is not None and (status.dtype not in (torch.int32, torch.uint32) or status.numel() != 1 or status.device != dev):
        raise TensorGameError("seen", -1, f"status must be one 32-bit word on {dev}")
    _launch(dev, "tg_seen_u64", _ptr(keys), _ptr(table), table.numel(), _ptr(fresh), _ptr(mask), _ptr(status), n,
            1 if insert else 0)
    return fresh


def slice_rank(state) -> torch.Tensor:
    """int32 (B,): sum over the S slices state[b][i] of the exact rank of the S x S matrix
    (== get_rank per game, utils.py:134-140, which sums torch.linalg.matrix_rank over slices)."""
    B, S, stride = _state_layout(state, "state")
    out = torch.empty((B,), dtype=torch.int32, device=state.device)
    _launch(state.device, "tg_rank_i32", _ptr(state), _ptr(out), B, S, stride)
    return out


def debug_fallbacks(device="cuda:0") -> int:
    """Workgroups that fell back from the packed 16-bit kernels to the exact byte-wise form so far
    (debug counter; synchronises the device)."""
    out = C.c_uint64(0)
    with torch.cuda.device(torch.device(device)):
        call("tg_debug_fallbacks", C.byref(out))
    return int(out.value)


def debug_handovers(device="cuda:0") -> int:
    """Games the matrix-core pass of step_many handed to the lattice kernels so far (debug counter; synchronises)."""
    out = C.c_uint64(0)
    with torch.cuda.device(torch.device(device)):
        call("tg_debug_handovers", C.byref(out))
    return int(out.value)


# ---- batched MCTS (include/tensor_game_search.h) ---------------------------------------------------------------


def _search_call(name: str, forest, *args) -> None:
    _launch(forest.device, name, C.byref(forest.desc), *args)


def search_reset(forest, states, n_sim: int) -> None:
    """Load the roots of a ``search.SearchForest`` (int8 (B,T,S,S,S), frame 0 = head) and empty its trees."""
    _need_gpu(states, "states")
    want = (forest.B, forest.T, forest.S, forest.S, forest.S)
    if states.dtype != torch.int8 or tuple(states.shape) != want or states.device != forest.device:
        raise TensorGameError("search_reset", -1, f"states must be int8 {want} on {forest.device}, got {states.dtype} "
                              f"{tuple(states.shape)} on {states.device}")
    states = states.contiguous()
    _search_call("tg_search_reset", forest, _ptr(states), int(n_sim))


def search_select(forest, model_in=None, scalars=None) -> None:
    """One descent per active game (tg_search_select); ``model_in`` (B,T,S,S,S) float32/float16/bfloat16 and ``scalars``
    float32 (B,1) receive the leaf's model input when given."""
    code = 0
    if model_in is not None:
        want = (forest.B, forest.T, forest.S, forest.S, forest.S)
        if model_in.dtype not in _FLOAT_DTYPES or tuple(model_in.shape) != want or not model_in.is_contiguous() \
                or model_in.device != forest.device:
            raise TensorGameError("search_select", -1, f"model_in must be contiguous float32/float16/bfloat16 {want}")
        code = _FLOAT_DTYPES[model_in.dtype]
    scalars = _flag(scalars, (forest.B, 1), torch.float32, forest.device, "scalars")
    _search_call("tg_search_select", forest, _ptr(model_in), code, _ptr(scalars))


def search_commit(forest, tokens, leaf_q, prior=None, mask=None) -> None:
    """Expand and back up every selected game (tg_search_commit): tokens int8 (B,k,3S), leaf_q float32 (B,), prior
    float32 (B,k) or None, mask uint8 (B,) or None."""
    dev = forest.device
    tokens = _tokens(tokens, (forest.B, forest.k), forest.S, dev, "tokens")
    leaf_q = _flag(leaf_q, (forest.B,), torch.float32, dev, "leaf_q")
    prior = _flag(prior, (forest.B, forest.k), torch.float32, dev, "prior")
    mask = _flag(mask, (forest.B,), torch.uint8, dev, "mask")
    _search_call("tg_search_commit", forest, _ptr(tokens), _ptr(leaf_q), _ptr(prior), _ptr(mask))


def search_advance(forest, n_sim: int) -> None:
    """End the move of every game that is not done (tg_search_advance)."""
    _search_call("tg_search_advance", forest, int(n_sim))


def search_policy(forest, n_logits: int, n_bar: int, out=None) -> torch.Tensor:
    """Improved policy float32 (B, max_actions, 3S, n_logits) of every move played (tg_search_policy)."""
    shape = (forest.B, forest.max_actions, 3 * forest.S, n_logits)
    out = _out(out, shape, torch.float32, forest.device, "out")
    _search_call("tg_search_policy", forest, _ptr(out), int(n_logits), int(n_bar))
    return out


# ---- replay buffers and mixed batches (include/tensor_game_replay.h) ------------------------------------------------


def replay_add(buf, states, policy, rewards, lengths, select: bool = False, status=None) -> None:
    """Store finished games in a ``replay.GameBuffer`` (tg_replay_add): states int8 (B,L,T,S,S,S), policy float32
    (B,L,3S,n_logits), rewards float32 (B,L), lengths int64 (B,) -- what ``search.actor_prediction`` returns (its int64
    rewards converted).  ``select``: store only the first game with the greatest final reward (act_step's best game).
    ``status`` uint32 (1,) gets bit 0 for a game with length 0 or > L (not stored)."""
    dev = buf.device
    for t, name in ((states, "states"), (policy, "policy"), (rewards, "rewards"), (lengths, "lengths")):
        _need_gpu(t, name)
    B = states.shape[0] if states.dim() == 6 else -1
    want = (B, buf.L, buf.T, buf.S, buf.S, buf.S)
    if states.dtype != torch.int8 or tuple(states.shape) != want or states.device != dev:
        raise TensorGameError("replay_add", -1, f"states must be int8 (B,L,T,S,S,S) = {want[1:]} per game on {dev}, "
                              f"got {states.dtype} {tuple(states.shape)} on {states.device}")
    if policy.dtype != torch.float32 or policy.dim() != 4 or tuple(policy.shape[:3]) != (B, buf.L, 3 * buf.S) \
            or policy.device != dev:
        raise TensorGameError("replay_add", -1, f"policy must be float32 (B,L,3S,n_logits) with (B,L,3S) = "
                              f"{(B, buf.L, 3 * buf.S)} on {dev}, got {policy.dtype} {tuple(policy.shape)}")
    n_logits = policy.shape[3]
    if not 1 <= n_logits <= _lib.TG_REPLAY_MAX_LOGITS:
        raise TensorGameError("replay_add", -1, f"n_logits={n_logits} outside [1, {_lib.TG_REPLAY_MAX_LOGITS}]")
    rewards = _flag(rewards, (B, buf.L), torch.float32, dev, "rewards")
    lengths = _flag(lengths, (B,), torch.int64, dev, "lengths")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    states, policy = states.contiguous(), policy.contiguous()
    _launch(dev, "tg_replay_add", C.byref(buf.desc), _ptr(states), _ptr(policy), int(n_logits), _ptr(rewards),
            _ptr(lengths), B, 1 if select else 0, _ptr(status))


def replay_items(idx, T: int, S: int, device, tokens=None, targets=None, played=None, best=None, kind=None, src=None,
                 direct_kind: Optional[int] = None, dtype=torch.float32, out=None, scalars=None, actions=None,
                 rewards=None, overflow=None, status=None, shift: int = 1):
    """Items of a mixed dataset at dataset indices ``idx`` (int64 (N,)) in one launch (tg_replay_items), in the layout
    of ``demo_items``: (frames (N,T,S,S,S) of ``dtype``, scalars float32 (N,1), actions int8 (N,3S), rewards float32
    (N,1)).  Sources: the synthetic set ``tokens`` int8 (n_demos,R,3S) / ``targets`` int8 (n_demos,S,S,S) (both None:
    no synthetic set), the ``played`` and ``best`` ``replay.GameBuffer`` (or None).  With the epoch table ``kind``
    uint8 / ``src`` int64 (len_data,) row n is of kind[idx[n]] at source index src[idx[n]]; without it every row is of
    ``direct_kind`` (0 synthetic, 1 played, 2 best) at source index idx[n].  Synthetic rows equal ``demo_items``;
    played / best rows are PlayedGamesDataset.__getitem__ (scalar = the move index).  A bad row is all zero and sets
    bit 0 of ``status`` uint32 (1,); ``overflow`` uint8 (N,) as ``demo_items``.  No host sync."""
    dev = torch.device(device)
    idx = _item_idx(idx, dev, "replay_items")
    N = idx.shape[0]
    if (tokens is None) != (targets is None):
        raise TensorGameError("replay_items", -1, "pass both tokens and targets, or neither")
    if tokens is not None:
        n_demos, S_t, stride = _state_layout(targets, "targets")
        if S_t != S or targets.device != dev:
            raise TensorGameError("replay_items", -1, f"targets must be (n_demos,{S},{S},{S}) on {dev}")
        _need_gpu(tokens, "tokens")
        if tokens.dim() != 3 or tokens.shape[0] != n_demos:
            raise TensorGameError("replay_items", -1, f"tokens must be int8 (n_demos,R,3S) with n_demos={n_demos}")
        R = tokens.shape[1]
        tokens = _tokens(tokens, (n_demos, R), S, dev, "tokens")
    else:
        n_demos, R, stride = 0, 1, S ** 3
    for b, name in ((played, "played"), (best, "best")):
        if b is not None and (b.S != S or b.T != T or b.device != dev):
            raise TensorGameError("replay_items", -1, f"the {name} buffer holds S={b.S} T={b.T} on {b.device}, the "
                                  f"items S={S} T={T} on {dev}")
    if kind is not None:
        if direct_kind is not None:
            raise TensorGameError("replay_items", -1, "pass the epoch table (kind, src) or direct_kind, not both")
        len_data = kind.shape[0] if kind.dim() == 1 else -1
        kind = _flag(kind, (len_data,), torch.uint8, dev, "kind")
        src = _flag(src, (len_data,), torch.int64, dev, "src")
        if src is None:
            raise TensorGameError("replay_items", -1, "an epoch table needs src")
        code = 0
    else:
        if direct_kind not in (0, 1, 2):
            raise TensorGameError("replay_items", -1, "without an epoch table direct_kind must be 0, 1 or 2")
        len_data, code = 0, int(direct_kind)
    dcode, out, scalars, actions, rewards, overflow, status = _item_outputs(
        N, T, S, dtype, dev, "replay_items", out, scalars, actions, rewards, overflow, status)
    pdesc = None if played is None else C.byref(played.desc)
    bdesc = None if best is None else C.byref(best.desc)
    _launch(dev, "tg_replay_items", _ptr(tokens), _ptr(targets), n_demos, R, S, stride, int(shift), pdesc, bdesc,
            _ptr(kind), _ptr(src), len_data, code, _ptr(idx), N, int(T), dcode, _ptr(out),
            _ptr(scalars), _ptr(actions), _ptr(rewards), _ptr(overflow), _ptr(status))
    return out, scalars, actions, rewards


# ---- a buffer's stored moves as dense arrays (include/tensor_game_replay_io.h) --------------------------------------


def _dense_rows(buf, M: int):
    """The shapes of M dense rows of ``buf``'s games: frames, tokens, rewards."""
    return (M, buf.T, buf.S, buf.S, buf.S), (M, 3 * buf.S), (M,)


def replay_pack(buf, max_moves: int, frames=None, tokens=None, rewards=None, lengths=None, move_offset=None,
                counts=None, status=None):
    """The stored games of a ``replay.GameBuffer`` as dense rows, oldest first (tg_replay_pack): returns (frames int8
    (max_moves,T,S,S,S), tokens int8 (max_moves,3S), rewards float32 (max_moves,), lengths int32 (C,), move_offset int64
    (C+1,), counts int64 (2,) = (G, M)), each allocated when it is not given.  Rows [0, M), lengths[:G] and
    move_offset[:G+1] are written; a game whose rows would pass ``max_moves`` is not written and sets bit 1 of
    ``status`` uint32 (1,).  No host sync."""
    dev = buf.device
    max_moves = int(max_moves)
    if max_moves < 0:
        raise TensorGameError("replay_pack", -1, f"max_moves={max_moves} < 0")
    f_shape, t_shape, r_shape = _dense_rows(buf, max_moves)
    frames = _out(frames, f_shape, torch.int8, dev, "frames")
    tokens = _out(tokens, t_shape, torch.int8, dev, "tokens")
    rewards = _out(rewards, r_shape, torch.float32, dev, "rewards")
    lengths = _out(lengths, (buf.C,), torch.int32, dev, "lengths")
    move_offset = _out(move_offset, (buf.C + 1,), torch.int64, dev, "move_offset")
    counts = _out(counts, (2,), torch.int64, dev, "counts")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_replay_pack", C.byref(buf.desc), max_moves, _ptr(lengths), _ptr(move_offset), _ptr(counts),
            _ptr(rewards), _ptr(tokens), _ptr(frames), _ptr(status))
    return frames, tokens, rewards, lengths, move_offset, counts


def replay_add_packed(buf, frames, tokens, rewards, lengths, first_slot: int = -1, games_added: int = -1,
                      status=None) -> None:
    """Store games given as dense rows in a ``replay.GameBuffer`` (tg_replay_add_packed): frames int8 (M,T,S,S,S),
    tokens int8 (M,3S), rewards float32 (M,), lengths int32 (G,); game g's rows start at the sum of the earlier
    (non-negative) lengths.  ``first_slot`` -1 continues at the ring's next slot, else the first stored game goes there;
    ``games_added`` >= 0 sets the games-ever-added counter instead of growing it.  ``status`` uint32 (1,) gets bit 0 for
    a length < 1 or > L and bit 1 for a game whose rows would pass M (neither is stored).  No host sync."""
    dev = buf.device
    for t, name in ((frames, "frames"), (tokens, "tokens"), (rewards, "rewards"), (lengths, "lengths")):
        _need_gpu(t, name)
    M = frames.shape[0] if frames.dim() == 5 else -1
    G = lengths.shape[0] if lengths.dim() == 1 else -1
    f_shape, t_shape, r_shape = _dense_rows(buf, M)
    frames = _flag(frames, f_shape, torch.int8, dev, "frames")
    tokens = _flag(tokens, t_shape, torch.int8, dev, "tokens")
    rewards = _flag(rewards, r_shape, torch.float32, dev, "rewards")
    lengths = _flag(lengths, (G,), torch.int32, dev, "lengths")
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_replay_add_packed", C.byref(buf.desc), _ptr(frames), _ptr(tokens), _ptr(rewards), _ptr(lengths),
            G, M, int(first_slot), int(games_added), _ptr(status))


# ---- move lists stored as games (include/tensor_game_replay_lists.h) ------------------------------------------------


def replay_add_lists(buf, starts, tokens, lengths, groups=None, shift: int = 1, select: bool = False, stored=None,
                     status=None) -> torch.Tensor:
    """Replay move lists from their start states and store the games in a ``replay.GameBuffer`` (tg_replay_add_lists):
    starts int8 (G,T,S,S,S), tokens int8 (M,K,3S) = cat(u,v,w) + shift and lengths int64 (M,) as ``solutions()`` returns
    them, groups int64 (M,) (None: list m starts from starts[m], M <= G).  A list is stored when 1 <= length <=
    min(K, L), its group is in [0, G), no entry of its heads leaves int8 and its last head is zero; ``status`` uint32
    (1,) gets bit 0, 2, 3 or 4 otherwise.  Move t is stored with the frames ``get_child_states`` leaves after t moves,
    the list's tokens and the reward -(t+1).  ``select``: only the first shortest valid list.  Returns ``stored`` uint8
    (M,) (allocated when it is not given): 1 where the list was stored.  No host sync."""
    dev = buf.device
    for t, name in ((starts, "starts"), (tokens, "tokens"), (lengths, "lengths")):
        _need_gpu(t, name)
    G = starts.shape[0] if starts.dim() == 5 else -1
    want = (G, buf.T, buf.S, buf.S, buf.S)
    if starts.dtype != torch.int8 or tuple(starts.shape) != want or starts.device != dev:
        raise TensorGameError("replay_add_lists", -1, f"starts must be int8 (G,T,S,S,S) = {want[1:]} per state on {dev}, "
                              f"got {starts.dtype} {tuple(starts.shape)} on {starts.device}")
    if tokens.dim() != 3:
        raise TensorGameError("replay_add_lists", -1, f"tokens must be int8 (M,K,3S), got {tuple(tokens.shape)}")
    M, K = tokens.shape[0], tokens.shape[1]
    tokens = _tokens(tokens, (M, K), buf.S, dev, "tokens")  # (S is the buffer's here, and the words are _tokens's)
    lengths = _list_lengths(lengths, M, dev)
    if groups is None:
        if M > G:
            raise TensorGameError("replay_add_lists", -1, f"groups: without it list m starts from starts[m], but M={M} "
                                                          f"> G={G}")
    else:
        _need_gpu(groups, "groups")
        groups = _flag(groups, (M,), torch.int64, dev, "groups")
    stored = _out(stored, (M,), torch.uint8, dev, "stored", new=torch.zeros)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    starts = starts.contiguous()
    _launch(dev, "tg_replay_add_lists", C.byref(buf.desc), _ptr(starts), G, _ptr(groups), _ptr(tokens),
            _ptr(lengths), M, int(K), int(shift), 1 if select else 0, _ptr(stored), _ptr(status))
    return stored


# ---- fused network inference (include/tensor_game_net.h) ------------------------------------------------------------


def net_check(cfg) -> None:
    """Raise TensorGameError (naming the bound) unless ``cfg`` (``_lib.NetConfig``) is in the supported family."""
    call("tg_net_check", C.byref(cfg))


def net_weights_size(cfg) -> int:
    """Floats in the packed weight blob of ``cfg`` (tg_net_weights_size)."""
    return _weights_size("tg_net_weights_size", cfg)


def _weights_size(symbol: str, cfg) -> int:
    out = C.c_int64(0)
    call(symbol, C.byref(cfg), C.byref(out))
    return int(out.value)


def _net_blob(cfg, w: torch.Tensor, size_symbol: str = "tg_net_weights_size") -> torch.device:
    _need_gpu(w, "weights")
    n = _weights_size(size_symbol, cfg)
    if w.dtype != torch.float32 or tuple(w.shape) != (n,) or not w.is_contiguous():
        raise TensorGameError("weights", -1, f"weights must be a contiguous float32 blob of {n} floats, got {w.dtype} "
                              f"{tuple(w.shape)}")
    return w.device


def _net_mask(flags, need: int, B: int, dev, name: str) -> Optional[torch.Tensor]:
    """The row mask of net_torso / net_sample: flags uint8 (B,) with ``need`` in 1 .. 255, or None."""
    if flags is None:
        return None
    if not 1 <= int(need) <= 255:
        raise TensorGameError(name, -1, f"need={need} with flags given: the bits a row's flags must hold, 1 .. 255")
    return _flag(flags, (B,), torch.uint8, dev, "flags")


def _net_frames(cfg, frames, dev, fn: str) -> int:
    """B of the network's input frames: float32 or int8 (B,T,S,S,S) with the T and S of ``cfg``, on ``dev``."""
    B = frames.shape[0] if frames.dim() == 5 else -1
    want = (B, cfg.T, cfg.S, cfg.S, cfg.S)
    if frames.dtype not in (torch.float32, torch.int8) or tuple(frames.shape) != want or frames.device != dev:
        raise TensorGameError(fn, -1, f"frames must be float32 or int8 (B,T,S,S,S) = {want[1:]} per game on "
                              f"{dev}, got {frames.dtype} {tuple(frames.shape)} on {frames.device}")
    return B


# The C symbols of one header's inference entries.  ``torso`` / ``sample`` None: the header has the masked forms only,
# which take flags = NULL for every row.
@dataclass(frozen=True)
class _NetEntries:
    size: str
    torso: Optional[str]
    torso_masked: str
    sample: Optional[str]
    sample_masked: str
    logits: str


_NET = _NetEntries("tg_net_weights_size", "tg_net_torso", "tg_net_torso_masked", "tg_net_sample", "tg_net_sample_masked",
                   "tg_net_logits")
_NET_S25 = _NetEntries("tg_net_s25_weights_size", None, "tg_net_s25_torso", None, "tg_net_s25_sample", "tg_net_s25_logits")


def _masked_launch(dev, plain: Optional[str], masked: str, args, flags, need: int) -> None:
    if flags is None and plain is not None:
        _launch(dev, plain, *args)
    else:
        _launch(dev, masked, *args, _ptr(flags), int(need) if flags is not None else 0)


def net_torso(cfg, w, frames, scalars, out=None, flags=None, need: int = 0) -> torch.Tensor:
    """Torso.forward (tg_net_torso): frames (B,T,S,S,S) float32 or int8, scalars float32 (B,dim_s) -> ee float32
    (B,3S^2,c).  With ``flags`` uint8 (B,) only the rows with ``(flags & need) == need`` are computed
    (tg_net_torso_masked): a given ``out`` keeps its other rows, an allocated one holds zeros there."""
    return _torso(_NET, "net_torso", cfg, w, frames, scalars, out, flags, need)


def _torso(sym: _NetEntries, fn: str, cfg, w, frames, scalars, out, flags, need) -> torch.Tensor:
    dev = _net_blob(cfg, w, sym.size)
    _need_gpu(frames, "frames")
    B = _net_frames(cfg, frames, dev, fn)
    frames = frames.contiguous()
    scalars = _flag(scalars.contiguous(), (B, cfg.dim_s), torch.float32, dev, "scalars")
    shape = (B, 3 * cfg.S * cfg.S, cfg.c)
    flags = _net_mask(flags, need, B, dev, fn)
    out = _out(out, shape, torch.float32, dev, "out", torch.empty if flags is None else torch.zeros)
    args = (C.byref(cfg), _ptr(w), _ptr(frames), 1 if frames.dtype == torch.int8 else 0, _ptr(scalars), _ptr(out), B)
    _masked_launch(dev, sym.torso, sym.torso_masked, args, flags, need)
    return out


def net_sample(cfg, w, ee, rows, k: int, seed: int, call_idx: int, uniforms=None, tokens=None, probs=None, q=None,
               flags=None, need: int = 0):
    """PolicyHead.fwd_infer + the risk-managed value (tg_net_sample) for ee float32 (B,3S^2,c): returns tokens int8
    (B,k,n_steps), probs float32 (B,k), q float32 (B,).  ``rows`` int64 (B,) key the random stream with ``seed`` and
    ``call_idx``; ``uniforms`` float32 (B,k,n_steps) replaces the stream when given.  With ``flags`` uint8 (B,)
    only the rows with ``(flags & need) == need`` are decoded (tg_net_sample_masked): given outputs keep their other
    rows, allocated ones hold zeros there."""
    return _sample(_NET, "net_sample", cfg, w, ee, rows, k, seed, call_idx, uniforms, tokens, probs, q, flags, need)


def _sample(sym: _NetEntries, fn: str, cfg, w, ee, rows, k, seed, call_idx, uniforms, tokens, probs, q, flags, need):
    dev = _net_blob(cfg, w, sym.size)
    B = ee.shape[0]
    flags = _net_mask(flags, need, B, dev, fn)
    new = torch.empty if flags is None else torch.zeros
    ee = _flag(ee, (B, 3 * cfg.S * cfg.S, cfg.c), torch.float32, dev, "ee")
    rows = _flag(rows, (B,), torch.int64, dev, "rows")
    uniforms = _flag(uniforms, (B, k, cfg.n_steps), torch.float32, dev, "uniforms")
    tokens = _out(tokens, (B, k, cfg.n_steps), torch.int8, dev, "tokens", new)
    probs = _out(probs, (B, k), torch.float32, dev, "probs", new)
    q = _out(q, (B,), torch.float32, dev, "q", new)
    args = (C.byref(cfg), _ptr(w), _ptr(ee), _ptr(rows), B, int(k), _u64(seed), _u64(call_idx), _ptr(uniforms),
            _ptr(tokens), _ptr(probs), _ptr(q))
    _masked_launch(dev, sym.sample, sym.sample_masked, args, flags, need)
    return tokens, probs, q


def net_logits(cfg, w, ee, g_action):
    """The forward of PolicyHead.fwd_train and the ValueHead on zz[:, 0] (tg_net_logits): ee float32 (B,3S^2,c),
    g_action (B,n_steps) integer tokens -> oo float32 (B,n_steps,n_logits), zz0 float32 (B,W), q float32
    (B,n_quantile)."""
    return _logits(_NET, "net_logits", cfg, w, ee, g_action)


def _logits(sym: _NetEntries, fn: str, cfg, w, ee, g_action):
    dev = _net_blob(cfg, w, sym.size)
    B = ee.shape[0]
    ee = _flag(ee, (B, 3 * cfg.S * cfg.S, cfg.c), torch.float32, dev, "ee")
    _need_gpu(g_action, "g_action")
    if tuple(g_action.shape) != (B, cfg.n_steps) or g_action.dtype.is_floating_point:
        raise TensorGameError(fn, -1, f"g_action must be integer (B,n_steps) = {(B, cfg.n_steps)}, got "
                              f"{g_action.dtype} {tuple(g_action.shape)}")
    g_action = g_action.to(dev, torch.int64).contiguous()
    oo = torch.empty((B, cfg.n_steps, cfg.n_logits), dtype=torch.float32, device=dev)
    zz0 = torch.empty((B, cfg.W), dtype=torch.float32, device=dev)
    q = torch.empty((B, cfg.n_quantile), dtype=torch.float32, device=dev)
    _launch(dev, sym.logits, C.byref(cfg), _ptr(w), _ptr(ee), _ptr(g_action), B, _ptr(oo), _ptr(zz0), _ptr(q))
    return oo, zz0, q


# ---- include/tensor_game_net_s25.h: the same entries at S = TG_NET_WIDE3_S --------------------------------------------
def net_s25_check(cfg) -> None:
    """Raise TensorGameError (naming the bound) unless ``cfg`` is in the S = 25 inference family (tg_net_s25_check)."""
    call("tg_net_s25_check", C.byref(cfg))


def net_s25_weights_size(cfg) -> int:
    """Floats in the packed weight blob of ``cfg`` (tg_net_s25_weights_size; the layout of every size)."""
    return _weights_size("tg_net_s25_weights_size", cfg)


def net_s25_torso(cfg, w, frames, scalars, out=None, flags=None, need: int = 0) -> torch.Tensor:
    """net_torso at S = 25 (tg_net_s25_torso): the same arguments and results."""
    return _torso(_NET_S25, "net_s25_torso", cfg, w, frames, scalars, out, flags, need)


def net_s25_sample(cfg, w, ee, rows, k: int, seed: int, call_idx: int, uniforms=None, tokens=None, probs=None, q=None,
                   flags=None, need: int = 0):
    """net_sample at S = 25 (tg_net_s25_sample): the same arguments and results."""
    return _sample(_NET_S25, "net_s25_sample", cfg, w, ee, rows, k, seed, call_idx, uniforms, tokens, probs, q, flags,
                   need)


def net_s25_logits(cfg, w, ee, g_action):
    """net_logits at S = 25 (tg_net_s25_logits): the same arguments and results."""
    return _logits(_NET_S25, "net_s25_logits", cfg, w, ee, g_action)


# ---- include/tensor_game_train.h ---------------------------------------------------------------------------------------
def net_train_check(cfg) -> None:
    """Raise TensorGameError (naming the bound) unless ``cfg`` is in the training family (tg_net_train_check)."""
    call("tg_net_train_check", C.byref(cfg))


def _workspace_size(symbol: str, cfg, B: int) -> int:
    out = C.c_int64(0)
    call(symbol, C.byref(cfg), int(B), C.byref(out))
    return int(out.value)


def net_train_workspace_size(cfg, B: int) -> int:
    """Bytes of workspace tg_net_loss_grad needs for B games."""
    return _workspace_size("tg_net_train_workspace_size", cfg, B)


def net_loss_grad(cfg, theta, pos_fix, frames, scalars, g_action, g_value, workspace, grad=None, losses=None,
                  status=None, weight_pol: float = 1.0, weight_val: float = 1000.0, dropout_p: float = 0.0,
                  seed: int = 0, call_idx: int = 0, keep_in=None, keep_out=None):
    """AlphaTensor.fwd_train's losses and the gradient of weight_pol * l_pol + weight_val * l_val (tg_net_loss_grad).

    theta float32 (the blob layout, pos slot = pos_enc), pos_fix float32 (n_steps, W), frames (B,T,S,S,S) float32 or
    int8, scalars float32 (B,dim_s), g_action int8 (B,n_steps), g_value float32 (B,1), workspace uint8 of at least
    net_train_workspace_size bytes.  grad (like theta) None means a loss-only call.  keep_in / keep_out: uint8
    (B, blocks, 2, n_steps, W) or None.  Returns (losses float32 [2], status int32 [1]); no host sync."""
    return _loss_grad("net_loss_grad", "tg_net_loss_grad", "tg_net_train_workspace_size", cfg, theta, pos_fix, frames,
                      scalars, g_action, g_value, workspace, grad, losses, status, weight_pol, weight_val, dropout_p, seed,
                      call_idx, keep_in, keep_out)


def _loss_grad(fn, symbol, size_symbol, cfg, theta, pos_fix, frames, scalars, g_action, g_value, workspace, grad, losses,
               status, weight_pol, weight_val, dropout_p, seed, call_idx, keep_in, keep_out,
               weights_symbol="tg_net_weights_size"):
    """The argument rules and the launch of net_loss_grad, net_loss_grad_sliced and net_loss_grad_s25, which differ in
    the C symbols."""
    dev = _net_blob(cfg, theta, weights_symbol)
    B = _net_frames(cfg, frames, dev, fn)
    if B < 1:
        raise TensorGameError(fn, -1, "B must be at least 1")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise TensorGameError(fn, -1, f"dropout_p={dropout_p} outside [0, 1)")
    frames = frames.contiguous()
    pos_fix = _flag(pos_fix, (cfg.n_steps, cfg.W), torch.float32, dev, "pos_fix")
    scalars = _flag(scalars, (B, cfg.dim_s), torch.float32, dev, "scalars")
    g_action = _flag(g_action, (B, cfg.n_steps), torch.int8, dev, "g_action")
    g_value = _flag(g_value, (B, 1), torch.float32, dev, "g_value")
    mask = (B, cfg.blocks, 2, cfg.n_steps, cfg.W)
    keep_in = _flag(keep_in, mask, torch.uint8, dev, "keep_in")
    keep_out = _flag(keep_out, mask, torch.uint8, dev, "keep_out")
    grad = _flag(grad, tuple(theta.shape), torch.float32, dev, "grad")
    losses = _out(losses, (2,), torch.float32, dev, "losses")
    status = _out(status, (1,), torch.int32, dev, "status")
    need = _workspace_size(size_symbol, cfg, B)
    _need_gpu(workspace, "workspace")
    if workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or \
            workspace.numel() < need or workspace.device != dev:
        raise TensorGameError(fn, -1, f"workspace must be contiguous uint8 of at least {need} bytes on "
                              f"{dev}, got {workspace.dtype} {tuple(workspace.shape)} on {workspace.device}")
    _launch(dev, symbol, C.byref(cfg), _ptr(theta), _ptr(pos_fix), _ptr(frames),
            1 if frames.dtype == torch.int8 else 0, _ptr(scalars), _ptr(g_action), _ptr(g_value), B,
            float(weight_pol), float(weight_val), float(dropout_p), _u64(seed), _u64(call_idx), _ptr(keep_in),
            _ptr(keep_out), _ptr(workspace), workspace.numel(), _ptr(grad), _ptr(losses), _ptr(status))
    return losses, status


# ---- include/tensor_game_train_sliced.h: the same three entries at S = TG_NET_WIDE2_S ---------------------------------
def net_train_sliced_check(cfg) -> None:
    """Raise TensorGameError (naming the bound) unless ``cfg`` is in the sliced training family
    (tg_net_train_sliced_check): S = 16 and both LDS plans within 160 KiB."""
    call("tg_net_train_sliced_check", C.byref(cfg))


def net_train_sliced_workspace_size(cfg, B: int) -> int:
    """Bytes of workspace tg_net_loss_grad_sliced needs for B games."""
    return _workspace_size("tg_net_train_sliced_workspace_size", cfg, B)


def net_loss_grad_sliced(cfg, theta, pos_fix, frames, scalars, g_action, g_value, workspace, grad=None, losses=None,
                         status=None, weight_pol: float = 1.0, weight_val: float = 1000.0, dropout_p: float = 0.0,
                         seed: int = 0, call_idx: int = 0, keep_in=None, keep_out=None):
    """net_loss_grad at S = TG_NET_WIDE2_S (tg_net_loss_grad_sliced): the same arguments and results, workspace of at
    least net_train_sliced_workspace_size bytes."""
    return _loss_grad("net_loss_grad_sliced", "tg_net_loss_grad_sliced", "tg_net_train_sliced_workspace_size", cfg, theta,
                      pos_fix, frames, scalars, g_action, g_value, workspace, grad, losses, status, weight_pol, weight_val,
                      dropout_p, seed, call_idx, keep_in, keep_out)


# ---- include/tensor_game_train_s25.h: the same three entries at S = TG_NET_WIDE3_S ------------------------------------
def net_train_s25_check(cfg) -> None:
    """Raise TensorGameError (naming the bound) unless ``cfg`` is in the S = 25 training family
    (tg_net_train_s25_check): tg_net_s25_check's and the three LDS plans within 160 KiB."""
    call("tg_net_train_s25_check", C.byref(cfg))


def net_train_s25_workspace_size(cfg, B: int) -> int:
    """Bytes of workspace tg_net_loss_grad_s25 needs for B games."""
    return _workspace_size("tg_net_train_s25_workspace_size", cfg, B)


def net_loss_grad_s25(cfg, theta, pos_fix, frames, scalars, g_action, g_value, workspace, grad=None, losses=None,
                      status=None, weight_pol: float = 1.0, weight_val: float = 1000.0, dropout_p: float = 0.0,
                      seed: int = 0, call_idx: int = 0, keep_in=None, keep_out=None):
    """net_loss_grad at S = TG_NET_WIDE3_S (tg_net_loss_grad_s25): the same arguments and results, workspace of at
    least net_train_s25_workspace_size bytes."""
    return _loss_grad("net_loss_grad_s25", "tg_net_loss_grad_s25", "tg_net_train_s25_workspace_size", cfg, theta,
                      pos_fix, frames, scalars, g_action, g_value, workspace, grad, losses, status, weight_pol, weight_val,
                      dropout_p, seed, call_idx, keep_in, keep_out, weights_symbol="tg_net_s25_weights_size")


# ---- sampled policy rollouts (include/tensor_game_rollout.h) --------------------------------------------------------
def rollout_check(B: int, n: int, S: int, T: int, dim_s: int = 0, step: int = 0, max_actions: int = 0,
                  with_actions: bool = False) -> None:
    """Raise TensorGameError (naming the argument) unless tg_rollout_advance takes these sizes.  Host only."""
    call("tg_rollout_check", int(B), int(n), int(S), int(T), int(dim_s), int(step), int(max_actions),
         1 if with_actions else 0)


def rollout_records(G: int, S: int, device):
    """Fresh group records of a rollout: int32 (G,) each -- best_nnz = S^3 (the reference's lowest_rank starts there,
    training.py:329), hits = 0, solved_step = solved_sample = -1."""
    kw = dict(dtype=torch.int32, device=device)
    return (torch.full((G,), S ** 3, **kw), torch.zeros((G,), **kw), torch.full((G,), -1, **kw),
            torch.full((G,), -1, **kw))


def rollout_advance(frames, tokens, n: int, step: int, records, scalars=None, nnz=None, overflow=None, actions=None,
                    shift: int = 1, active=None, stop_solved: bool = False):
    """One step of a sampled rollout in one launch (tg_rollout_advance): == reference training.py:253-268 (the new
    head, the history shift, scalars + 1, rank_ubs and the best sample per group) + the running statistics of
    :343-346.  frames int8 (B,T,S,S,S), stepped IN PLACE (newest first: the next ``net_torso`` input); tokens int8
    (B,3S); rows are group-major, row g*n + s = sample s of group g; ``records`` = (best_nnz, hits, solved_step,
    solved_sample), int32 (B/n,) each (``rollout_records``), updated; scalars float32 (B,dim_s) += 1; overflow uint8
    (B,) is set where an entry left int8; actions int8 (B,max_actions,3S) receives the tokens at index ``step``.
    Returns nnz int32 (B,), the non-zero count of every new head.

    ``stop_solved`` (tg_rollout_advance_masked): only the groups whose solved_step is still negative are stepped; of the
    others nothing but solved_step is read and nothing is written.  ``active`` uint8 (B,), initialised to 1 by the
    caller, receives 1 for the rows of a group still unsolved after this step and 0 for the rows of a group it solved:
    the row mask of the next ``net_torso`` / ``net_sample`` call (``need=1``).  A given ``nnz`` keeps the counts of the
    rows that are not stepped; an allocated one holds zeros there."""
    _need_gpu(frames, "frames")
    if active is not None and not stop_solved:
        raise TensorGameError("rollout_advance", -1, "active is written by the masked step only: pass stop_solved=True")
    if frames.dtype != torch.int8 or frames.dim() != 5 or not (frames.shape[2] == frames.shape[3] == frames.shape[4]):
        raise TensorGameError("rollout_advance", -1, f"frames must be int8 (B,T,S,S,S), got {frames.dtype} "
                              f"{tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise TensorGameError("rollout_advance", -1, "frames must be contiguous (they are stepped in place)")
    B, T, S = frames.shape[0], frames.shape[1], frames.shape[2]
    dev = frames.device
    tokens = _tokens(tokens, (B,), S, dev, "tokens")
    dim_s = 0
    if scalars is not None:
        dim_s = scalars.shape[1] if scalars.dim() == 2 else -1
        scalars = _flag(scalars, (B, dim_s), torch.float32, dev, "scalars")
    max_actions = 0
    if actions is not None:
        max_actions = actions.shape[1] if actions.dim() == 3 else -1
        actions = _flag(actions, (B, max_actions, 3 * S), torch.int8, dev, "actions")
    rollout_check(B, n, S, T, dim_s, step, max_actions, actions is not None)
    nnz = _out(nnz, (B,), torch.int32, dev, "nnz", torch.zeros if stop_solved else torch.empty)
    overflow = _flag(overflow, (B,), torch.uint8, dev, "overflow")
    active = _flag(active, (B,), torch.uint8, dev, "active")
    if len(records) != 4:
        raise TensorGameError("rollout_advance", -1, "records must be (best_nnz, hits, solved_step, solved_sample)")
    rec = [_flag(r, (B // n,), torch.int32, dev, name)
           for r, name in zip(records, ("best_nnz", "hits", "solved_step", "solved_sample"))]
    if any(r is None for r in rec):
        raise TensorGameError("rollout_advance", -1, "records must be four int32 tensors (ops.rollout_records)")
    ptrs = (_ptr(frames), _ptr(tokens), _ptr(scalars), _ptr(nnz), _ptr(overflow), *map(_ptr, rec), _ptr(actions))
    sizes = (B, int(n), S, T, dim_s, int(step), max_actions, int(shift))
    if stop_solved:
        _launch(dev, "tg_rollout_advance_masked", *ptrs, _ptr(active), *sizes)
    else:
        _launch(dev, "tg_rollout_advance", *ptrs, *sizes)
    return nnz


# ---- the solution search over a queue of start states (include/tensor_game_rollout_slots.h) -------------------------
@dataclass
class RolloutSlots:
    """The slot-side buffers of ``rollout_advance_slots`` / ``rollout_refill``: R slots of n rows, B = R*n.  ``records``
    = (best_nnz, hits, solved_step, solved_sample) int32 (R,); ``slot_state`` int64 (R,) (< 0: empty), ``slot_step``
    int32 (R,); per row frames int8 (B,T,S,S,S), scalars float32 (B,dim_s), nnz int32, overflow / active uint8, actions
    int8 (B,max_actions,3S), tokens int8 (B,3S) (the policy's persistent output), rows int64 (the stream keys),
    uniforms float32 (B,1,3S); ``head`` int64 [1] and ``live`` int32 [1] are the queue's device words."""

    n: int
    max_actions: int
    frames: torch.Tensor
    scalars: torch.Tensor
    nnz: torch.Tensor
    overflow: torch.Tensor
    active: torch.Tensor
    actions: torch.Tensor
    tokens: torch.Tensor
    rows: torch.Tensor
    uniforms: torch.Tensor
    records: Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]
    slot_state: torch.Tensor
    slot_step: torch.Tensor
    head: torch.Tensor
    live: torch.Tensor


def rollout_slots(R: int, n: int, S: int, T: int, dim_s: int, max_actions: int, device) -> RolloutSlots:
    """R empty slots of n rows each (``slot_state`` = -1, ``head`` = 0): the first ``rollout_refill`` fills them."""
    R, n, K = int(R), int(n), int(max_actions)
    if R < 0 or R > _lib.TG_ROLLOUT_MAX_SLOTS:
        raise TensorGameError("rollout_slots", -1, f"R={R} slots outside [0,{_lib.TG_ROLLOUT_MAX_SLOTS}] "
                              "(TG_ROLLOUT_MAX_SLOTS)")
    B = R * max(n, 0)
    rollout_check(B, n, S, T, dim_s, 0, K, True)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    return RolloutSlots(n, K, z((B, T, S, S, S), torch.int8), z((B, dim_s), torch.float32), z((B,), torch.int32),
                        z((B,), torch.uint8), z((B,), torch.uint8), z((B, K, 3 * S), torch.int8),
                        z((B, 3 * S), torch.int8), torch.full((B,), -1, dtype=torch.int64, device=device),
                        z((B, 1, 3 * S), torch.float32), rollout_records(R, S, device),
                        torch.full((R,), -1, dtype=torch.int64, device=device), z((R,), torch.int32),
                        z((1,), torch.int64), z((1,), torch.int32))


def _slot_rows(slots: RolloutSlots, fn: str):
    """(B, R, S, T, dim_s, K, dev) of the slot buffers, every one held to its shape."""
    f = slots.frames
    _need_gpu(f, "frames")
    if f.dtype != torch.int8 or f.dim() != 5 or not (f.shape[2] == f.shape[3] == f.shape[4]) or not f.is_contiguous():
        raise TensorGameError(fn, -1, f"frames must be contiguous int8 (B,T,S,S,S), got {f.dtype} {tuple(f.shape)}")
    B, T, S = f.shape[0], f.shape[1], f.shape[2]
    dev, n, K = f.device, int(slots.n), int(slots.max_actions)
    dim_s = slots.scalars.shape[1] if slots.scalars.dim() == 2 else -1
    rollout_check(B, n, S, T, dim_s, 0, K, True)
    R = B // n
    for name, shape, dtype in (("scalars", (B, dim_s), torch.float32), ("nnz", (B,), torch.int32),
                               ("overflow", (B,), torch.uint8), ("active", (B,), torch.uint8),
                               ("actions", (B, K, 3 * S), torch.int8), ("tokens", (B, 3 * S), torch.int8),
                               ("rows", (B,), torch.int64), ("uniforms", (B, 1, 3 * S), torch.float32),
                               ("slot_state", (R,), torch.int64), ("slot_step", (R,), torch.int32),
                               ("head", (1,), torch.int64), ("live", (1,), torch.int32)):
        if getattr(slots, name) is None:
            raise TensorGameError(fn, -1, f"slots.{name} is missing (ops.rollout_slots allocates it)")
        _flag(getattr(slots, name), shape, dtype, dev, name)
    if len(slots.records) != 4:
        raise TensorGameError(fn, -1, "records must be (best_nnz, hits, solved_step, solved_sample)")
    for r, name in zip(slots.records, ("best_nnz", "hits", "solved_step", "solved_sample")):
        if r is None:
            raise TensorGameError(fn, -1, "records must be four int32 tensors (ops.rollout_records)")
        _flag(r, (R,), torch.int32, dev, name)
    return B, R, S, T, dim_s, K, dev


def rollout_advance_slots(slots: RolloutSlots, tokens=None, shift: int = 1) -> None:
    """One step of every LIVE slot, each at its own step index, in one launch (tg_rollout_advance_slots): a slot is
    live iff it holds a state (slot_state >= 0) that is unsolved (solved_step < 0) with slot_step < max_actions.  Live
    slots get what ``rollout_advance(stop_solved=True)`` gives an active group with ``step`` = their slot_step, then
    slot_step += 1; of the others nothing but the three words is read and nothing is written.  ``tokens`` int8 (B,3S)
    defaults to ``slots.tokens``."""
    B, R, S, T, dim_s, K, dev = _slot_rows(slots, "rollout_advance_slots")
    tokens = _tokens(slots.tokens if tokens is None else tokens, (B,), S, dev, "tokens")
    _launch(dev, "tg_rollout_advance_slots", _ptr(slots.frames), _ptr(tokens), _ptr(slots.scalars), _ptr(slots.nnz),
            _ptr(slots.overflow), *map(_ptr, slots.records), _ptr(slots.actions), _ptr(slots.active),
            _ptr(slots.slot_state), _ptr(slots.slot_step), B, int(slots.n), S, T, dim_s, K, int(shift))


def rollout_refill(slots: RolloutSlots, states, scalars, out, seed: int = 0, first_state: int = 0,
                   uniforms: bool = True) -> None:
    """Flush the finished slots to the dense per-state outputs, hand the next queue states to the finished and the empty
    slots in slot order, and prepare the next policy call (tg_rollout_refill: two launches, no host sync).  ``states``
    int8 (N,T,S,S,S) and ``scalars`` float32 (N,dim_s) are the queue, ``slots.head`` its read position; ``out`` =
    (best_nnz, hits, solved_step, solved_sample int32 (N,), overflow uint8 (N,), tokens int8 (N,max_actions,3S)).
    Afterwards ``slots.active`` marks the rows of the slots that hold an unfinished state, ``slots.live`` counts those
    slots, ``slots.rows`` = (first_state + state) * n + sample keys their streams, and with ``uniforms`` the rows'
    ``slots.uniforms`` are what ``net_sample`` would draw with ``seed`` and ``call_idx`` = the slot's own step."""
    B, R, S, T, dim_s, K, dev = _slot_rows(slots, "rollout_refill")
    _need_gpu(states, "states")
    N = states.shape[0] if states.dim() == 5 else -1
    if states.dtype != torch.int8 or tuple(states.shape) != (N, T, S, S, S) or states.device != dev or \
            not states.is_contiguous():
        raise TensorGameError("rollout_refill", -1, f"states must be contiguous int8 (N,T,S,S,S) = {(T, S, S, S)} per "
                              f"state on {dev}, got {states.dtype} {tuple(states.shape)} on {states.device}")
    scalars = _flag(scalars, (N, dim_s), torch.float32, dev, "scalars")
    if int(first_state) < 0:
        raise TensorGameError("rollout_refill", -1, f"first_state={first_state} < 0")
    if len(out) != 6:
        raise TensorGameError("rollout_refill", -1, "out must be (best_nnz, hits, solved_step, solved_sample, overflow, "
                              "tokens)")
    shapes = [((N,), torch.int32)] * 4 + [((N,), torch.uint8), ((N, K, 3 * S), torch.int8)]
    names = ("out best_nnz", "out hits", "out solved_step", "out solved_sample", "out overflow", "out tokens")
    for t, (shape, dtype), name in zip(out, shapes, names):
        if t is None:
            raise TensorGameError("rollout_refill", -1, f"{name} is missing")
        _flag(t, shape, dtype, dev, name)
    _launch(dev, "tg_rollout_refill", _ptr(states), _ptr(scalars), N, _ptr(slots.head), int(first_state), _u64(seed),
            3 * S if uniforms else 0, _ptr(slots.frames), _ptr(slots.scalars), _ptr(slots.nnz), _ptr(slots.overflow),
            *map(_ptr, slots.records), _ptr(slots.actions), _ptr(slots.active), _ptr(slots.slot_state),
            _ptr(slots.slot_step), *map(_ptr, out), _ptr(slots.rows), _ptr(slots.uniforms if uniforms else None),
            _ptr(slots.live), B, int(slots.n), S, T, dim_s, K)


def flip_check(M: int, W: int, K: int, S: int, shift: int = 1, bound: int = 1, step0: int = 0, n_steps: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_flip_begin / tg_flip_advance take these sizes.  Host only."""
    call("tg_flip_check", int(M), int(W), int(K), int(S), int(shift), int(bound), int(step0), int(n_steps))


_FLIP_STATE = (("cur", torch.int8), ("cur_rank", torch.int32), ("best", torch.int8), ("best_rank", torch.int32),
               ("best_step", torch.int64), ("flips", torch.int64), ("state", torch.int32))


# and the two tensor_game_flips_plus.h adds
_FLIP_PLUS_STATE = _FLIP_STATE + (("since", torch.int32), ("pluses", torch.int64))


# the nine of include/tensor_game_flips_mod2.h: the two lists are rows of three mask words
_FLIP2_STATE = (("cur", torch.int32), ("cur_rank", torch.int32), ("best", torch.int32), ("best_rank", torch.int32),
                ("best_step", torch.int64), ("flips", torch.int64), ("state", torch.int32), ("since", torch.int32),
                ("pluses", torch.int64))


def _flip_state(given: dict, W: int, K: int, S: int, dev, fn: str, names=_FLIP_STATE, row=None) -> dict:
    """The walk-state tensors ``names`` (the seven of include/tensor_game_flips.h) on ``dev``: ``given[name]`` held to
    the rule of ``_flag``, or allocated where it is None.  ``row``: the width of a row of the two lists (3S tokens)."""
    out = {}
    for name, dtype in names:
        shape = (W, K, 3 * S if row is None else row) if name in ("cur", "best") else (W,)
        t = given.get(name)
        if t is not None:
            _need_gpu(t, name)
        out[name] = _out(t, shape, dtype, dev, name)
    return out


def flip_begin(tokens, lengths, src=None, bound: int = 1, shift: int = 1, status=None, **state):
    """Start W flip-graph walks in one launch (include/tensor_game_flips.h).  tokens int8 (M,K,3S) and lengths int64 (M,)
    as ``solutions()`` or an archive's ``entries()`` give them; ``src`` int64 (W,): the list walk w starts from (None:
    walk w starts from list w).  Each list loses its null terms, is brought to stored form and reduced.  Returns the walk
    state, a dict of device tensors: cur, best int8 (W,K,3S); cur_rank, best_rank, state int32 (W,); best_step, flips
    int64 (W,) (any of them may be passed in by name).  A bad row (length outside [0,K]: bit 0 of ``status`` uint32 (1,);
    a factor value outside [-bound,bound]: bit 1; a ``src`` outside [0,M): bit 2) gets state -1.  No host sync."""
    fn = "flip_begin"
    tokens, M, K, S, dev = _list_tokens(tokens, fn)
    lengths = _list_lengths(lengths, M, dev)
    W = M
    if src is not None:
        _need_gpu(src, "src")
        if src.dim() != 1:
            raise TensorGameError(fn, -1, f"src must be int64 (W,), got {tuple(src.shape)}")
        W = src.shape[0]
        src = _flag(src, (W,), torch.int64, dev, "src")
    flip_check(M, W, K, S, shift, bound)
    st = _flip_state(state, W, K, S, dev, fn)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_flip_begin", _ptr(tokens), _ptr(lengths), M, _ptr(src), W, K, S, int(shift), int(bound),
            *[_ptr(st[name]) for name, _ in _FLIP_STATE], _ptr(status))
    return st


def flip_advance(st: dict, n_steps: int, bound: int = 1, shift: int = 1, seed: int = 0, walk0: int = 0, step0: int = 0):
    """``n_steps`` steps (at most TG_FLIP_MAX_STEPS) of the walks ``st`` (the dict ``flip_begin`` returned) in place, in
    one launch: steps step0 .. step0 + n_steps - 1 of the walks with global ids walk0 .. walk0 + W - 1, drawn from Philox
    keyed by (seed, id, step).  Walks of state 1 (stuck) or -1 (bad) are left alone.  Returns ``st``.  No host sync."""
    fn = "flip_advance"
    cur = st["cur"]
    _need_gpu(cur, "cur")
    W, K, S = _list_shape(cur, fn, "cur", "W")
    flip_check(0, W, K, S, shift, bound, step0, n_steps)
    st = _flip_state({name: st[name] for name, _ in _FLIP_STATE}, W, K, S, cur.device, fn)
    _launch(cur.device, "tg_flip_advance", *[_ptr(st[name]) for name, _ in _FLIP_STATE], W, K, S, int(shift), int(bound),
            C.c_uint64(_u64(seed)), C.c_uint64(_u64(walk0)), int(step0), int(n_steps))
    return st


def flip_plus_check(W: int, K: int, S: int, shift: int = 1, bound: int = 1, step0: int = 0, n_steps: int = 1,
                    plus_after: int = 1, plus_slack: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_flip_advance_plus takes these sizes.  Host only."""
    call("tg_flip_plus_check", int(W), int(K), int(S), int(shift), int(bound), int(step0), int(n_steps), int(plus_after),
         int(plus_slack))


def flip_advance_plus(st: dict, n_steps: int, plus_after: int, plus_slack: int = 1, bound: int = 1, shift: int = 1,
                      seed: int = 0, walk0: int = 0, step0: int = 0):
    """``flip_advance`` with plus transitions (include/tensor_game_flips_plus.h): a walk that has no flip left, or has
    not lowered its rank for ``plus_after`` steps, rewrites two terms into three while its list is shorter than
    min(K, best_rank + plus_slack), and goes on.  ``st`` holds the seven tensors of ``flip_begin`` and ``since`` int32
    (W,), ``pluses`` int64 (W,), zero for fresh walks (a missing one is a refusal: the counters carry from call to
    call).  In place, one launch, no host sync.  Returns ``st``."""
    fn = "flip_advance_plus"
    cur = st["cur"]
    _need_gpu(cur, "cur")
    W, K, S = _list_shape(cur, fn, "cur", "W")
    flip_plus_check(W, K, S, shift, bound, step0, n_steps, plus_after, plus_slack)
    for name in ("since", "pluses"):
        if st.get(name) is None:
            raise TensorGameError(fn, -1, f"{name} must be given (zeros for fresh walks)")
    st = _flip_state({name: st[name] for name, _ in _FLIP_PLUS_STATE}, W, K, S, cur.device, fn, _FLIP_PLUS_STATE)
    _launch(cur.device, "tg_flip_advance_plus", *[_ptr(st[name]) for name, _ in _FLIP_PLUS_STATE], W, K, S, int(shift),
            int(bound), C.c_uint64(_u64(seed)), C.c_uint64(_u64(walk0)), int(step0), int(n_steps), int(plus_after),
            int(plus_slack))
    return st


def flip2_check(M: int, W: int, K: int, S: int, shift: int = 1, step0: int = 0, n_steps: int = 1, plus_after: int = 0,
                plus_slack: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_flip2_begin / tg_flip2_advance take these sizes.  Host only."""
    call("tg_flip2_check", int(M), int(W), int(K), int(S), int(shift), int(step0), int(n_steps), int(plus_after),
         int(plus_slack))


def _flip2_lists(lists, fn: str, name: str, lead: str) -> Tuple[int, int]:
    """(W, K) of the mask rows int32 (W,K,3) of W lists over Z_2 on a ROCm device."""
    _need_gpu(lists, name)
    if lists.dtype != torch.int32 or lists.dim() != 3 or lists.shape[2] != 3:
        raise TensorGameError(fn, -1, f"{name} must be int32 ({lead},K,3), got {lists.dtype} {tuple(lists.shape)}")
    return lists.shape[0], lists.shape[1]


def flip2_begin(tokens, lengths, src=None, shift: int = 1, status=None, **state):
    """Start W flip-graph walks over Z_2 in one launch (include/tensor_game_flips_mod2.h).  tokens int8 (M,K,3S) and
    lengths int64 (M,) as ``solutions()`` or an archive's ``entries()`` give them; ``src`` int64 (W,): the list walk w
    starts from (None: walk w starts from list w).  Each list is taken mod 2 (a factor becomes one mask word), loses its
    null terms and is reduced.  Returns the walk state, a dict of device tensors: cur, best int32 (W,K,3); cur_rank,
    best_rank, state, since int32 (W,); best_step, flips, pluses int64 (W,) (any of them may be passed in by name).  A
    bad row (length outside [0,K]: bit 0 of ``status`` uint32 (1,); a ``src`` outside [0,M): bit 2) gets state -1; there
    is no range error.  No host sync."""
    fn = "flip2_begin"
    tokens, M, K, S, dev = _list_tokens(tokens, fn)
    lengths = _list_lengths(lengths, M, dev)
    W = M
    if src is not None:
        _need_gpu(src, "src")
        if src.dim() != 1:
            raise TensorGameError(fn, -1, f"src must be int64 (W,), got {tuple(src.shape)}")
        W = src.shape[0]
        src = _flag(src, (W,), torch.int64, dev, "src")
    flip2_check(M, W, K, S, shift)
    st = _flip_state(state, W, K, S, dev, fn, _FLIP2_STATE, row=3)
    status = _flag(status, (1,), torch.uint32, dev, "status")
    _launch(dev, "tg_flip2_begin", _ptr(tokens), _ptr(lengths), M, _ptr(src), W, K, S, int(shift),
            *[_ptr(st[name]) for name, _ in _FLIP2_STATE], _ptr(status))
    return st


def flip2_advance(st: dict, n_steps: int, S: int, plus_after: int = 0, plus_slack: int = 1, seed: int = 0, walk0: int = 0,
                  step0: int = 0):
    """``n_steps`` steps (at most TG_FLIP_MAX_STEPS) of the Z_2 walks ``st`` (the dict ``flip2_begin`` returned, of lists
    over S values) in place, in one launch: steps step0 .. step0 + n_steps - 1 of the walks with global ids walk0 ..
    walk0 + W - 1, drawn from Philox keyed by (seed, id, step).  No flip is ever refused.  With ``plus_after`` > 0 a walk
    that has no flip left, or has not lowered its rank for that many steps, takes a plus transition while its list is
    shorter than min(K, best_rank + plus_slack).  Walks of state 1 (stuck) or -1 (bad) are left alone.  Returns ``st``.
    No host sync."""
    fn = "flip2_advance"
    W, K = _flip2_lists(st["cur"], fn, "cur", "W")
    dev = st["cur"].device
    flip2_check(0, W, K, S, 0, step0, n_steps, plus_after, plus_slack)
    for name, _ in _FLIP2_STATE:
        if st.get(name) is None:
            raise TensorGameError(fn, -1, f"{name} must be given (flip2_begin makes it)")
    st = _flip_state({name: st[name] for name, _ in _FLIP2_STATE}, W, K, S, dev, fn, _FLIP2_STATE, row=3)
    _launch(dev, "tg_flip2_advance", *[_ptr(st[name]) for name, _ in _FLIP2_STATE], W, K, int(S), C.c_uint64(_u64(seed)),
            C.c_uint64(_u64(walk0)), int(step0), int(n_steps), int(plus_after), int(plus_slack))
    return st


def flip2_residual(targets, lists, ranks, residual=None):
    """The proof of lists over Z_2 (tg_flip2_residual), one launch, exact: int32 (M,), per list the number of cells of
    ``targets`` int8 (M,S,S,S) whose parity differs from that of the sum of the first ``ranks[m]`` (int32 (M,)) terms of
    ``lists`` int32 (M,K,3); -1 for a rank outside [0,K].  No host sync."""
    fn = "flip2_residual"
    M, K = _flip2_lists(lists, fn, "lists", "M")
    dev = lists.device
    _need_gpu(targets, "targets")
    if targets.dtype != torch.int8 or targets.dim() != 4 or targets.shape[0] != M or targets.device != dev \
            or not (targets.shape[1] == targets.shape[2] == targets.shape[3]):
        raise TensorGameError(fn, -1, f"targets must be int8 ({M},S,S,S) on {dev}, got {targets.dtype} "
                                      f"{tuple(targets.shape)} on {targets.device}")
    S = targets.shape[1]
    flip2_check(M, 0, K, S, 0)
    targets = targets if targets.is_contiguous() else targets.contiguous()
    lists = _flag(lists, (M, K, 3), torch.int32, dev, "lists")
    _need_gpu(ranks, "ranks")
    ranks = _flag(ranks, (M,), torch.int32, dev, "ranks")
    if residual is not None:
        _need_gpu(residual, "residual")
    residual = _out(residual, (M,), torch.int32, dev, "residual")
    _launch(dev, "tg_flip2_residual", _ptr(targets), _ptr(lists), _ptr(ranks), M, K, S, _ptr(residual))
    return residual


_LIFT2_OUT = ("status", "try_used", "unknowns", "sys_rank", "miss")


def lift2_workspace_bytes(K: int, S: int) -> int:
    """Bytes of scratch ``lift2_signs`` needs per concurrently resident list of up to K terms over S values
    (tg_lift2_workspace_bytes); 0 where the system fits in LDS.  Host only."""
    n = _lib.lib.tg_lift2_workspace_bytes(int(K), int(S))
    if n < 0:
        raise TensorGameError("tg_lift2_workspace_bytes", int(n), _lib.lib.tg_last_error().decode("utf-8", "replace"))
    return int(n)


def lift2_check(W: int, K: int, S: int, shift: int = 1, tries: int = 1, ws_lists: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_lift2_signs takes these sizes.  Host only."""
    call("tg_lift2_check", int(W), int(K), int(S), int(shift), int(tries), int(ws_lists))


def lift2_signs(targets, lists, ranks, tries: int = 32, seed: int = 0, list0: int = 0, shift: int = 1, workspace=None,
                ws_lists: Optional[int] = None, tokens=None, **out):
    """The sign lift of W lists over Z_2 to the integers, one launch (include/tensor_game_lift.h).  ``targets`` int8
    (W,S,S,S): the INTEGER targets; ``lists`` int32 (W,K,3) and ``ranks`` int32 (W,) as the Z_2 walks hold them.  Returns
    (tokens int8 (W,K,3S), dict of status, try_used, unknowns, sys_rank, miss int32 (W,)); any of them may be passed in
    by name.  ``workspace``: a uint8 tensor of at least ``ws_lists * lift2_workspace_bytes(K, S)`` bytes, needed where
    that size is not 0 (``ws_lists`` defaults to what the tensor holds).  No host sync, no allocation beyond the outputs
    that were not given."""
    fn = "lift2_signs"
    W, K = _flip2_lists(lists, fn, "lists", "W")
    dev = lists.device
    _need_gpu(targets, "targets")
    if targets.dtype != torch.int8 or targets.dim() != 4 or targets.shape[0] != W or targets.device != dev \
            or not (targets.shape[1] == targets.shape[2] == targets.shape[3]):
        raise TensorGameError(fn, -1, f"targets must be int8 ({W},S,S,S) on {dev}, got {targets.dtype} "
                                      f"{tuple(targets.shape)} on {targets.device}")
    S = targets.shape[1]
    per_list = 0 if not (1 <= K <= _lib.TG_FLIP_MAX_K and 1 <= S <= _lib.TG_MAX_S) else lift2_workspace_bytes(K, S)
    if workspace is not None:
        _need_gpu(workspace, "workspace")
        if workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.device != dev or not workspace.is_contiguous():
            raise TensorGameError(fn, -1, f"workspace must be contiguous uint8 (bytes,) on {dev}")
    if ws_lists is None:
        ws_lists = 0 if workspace is None or per_list == 0 else min(workspace.numel() // per_list, _lib.TG_LIFT2_MAX_WS_LISTS)
    lift2_check(W, K, S, shift, tries, ws_lists)
    if per_list and W and (workspace is None or workspace.numel() < int(ws_lists) * per_list):
        raise TensorGameError(fn, -1, f"workspace must hold ws_lists={int(ws_lists)} x {per_list} bytes, got "
                                      f"{0 if workspace is None else workspace.numel()}")
    targets = targets if targets.is_contiguous() else targets.contiguous()
    lists = _flag(lists, (W, K, 3), torch.int32, dev, "lists")
    _need_gpu(ranks, "ranks")
    ranks = _flag(ranks, (W,), torch.int32, dev, "ranks")
    if tokens is not None:
        _need_gpu(tokens, "tokens")
    tokens = _out(tokens, (W, K, 3 * S), torch.int8, dev, "tokens")
    res = {}
    for name in _LIFT2_OUT:
        t = out.pop(name, None)
        if t is not None:
            _need_gpu(t, name)
        res[name] = _out(t, (W,), torch.int32, dev, name)
    if out:
        raise TensorGameError(fn, -1, f"unknown outputs {sorted(out)}")
    _launch(dev, "tg_lift2_signs", _ptr(targets), _ptr(lists), _ptr(ranks), W, K, S, int(shift), C.c_uint64(_u64(seed)),
            C.c_uint64(_u64(list0)), int(tries), _ptr(tokens), *[_ptr(res[name]) for name in _LIFT2_OUT],
            _ptr(workspace if per_list else None), int(ws_lists))
    return tokens, res


_BILINEAR_DTYPES = {torch.float32: ("f32", 4), torch.float64: ("f64", 8)}


def bilinear_check(batch: int, rows: int, cols: int, ld: Optional[int] = None, batch_stride: Optional[int] = None,
                   R: int = 1, n: int = 2, mode: int = 0, shift: int = 1, elem_bytes: int = 4) -> None:
    """Raise TensorGameError (naming the argument) unless tg_bilinear_encode_* / tg_bilinear_decode_* take these sizes
    (``ld`` defaults to ``cols``, ``batch_stride`` to ``rows * ld``).  Host only."""
    ld = cols if ld is None else ld
    call("tg_bilinear_check", int(batch), int(rows), int(cols), int(ld),
         int(rows * ld if batch_stride is None else batch_stride), int(R), int(n), int(mode), int(shift), int(elem_bytes))


def _bilinear_matrices(t: torch.Tensor, name: str, fn: str):
    """(batch, rows, cols, ld, batch_stride, entry suffix, element bytes) of a strided (batch,rows,cols) view, which is
    taken as it is (no copy): only the column stride is held to 1."""
    _need_gpu(t, name)
    if t.dtype not in _BILINEAR_DTYPES or t.dim() != 3:
        raise TensorGameError(fn, -1, f"{name} must be float32 or float64 (batch,rows,cols), got {t.dtype} "
                                      f"{tuple(t.shape)}")
    if t.stride(2) != 1:
        raise TensorGameError(fn, -1, f"{name}: the column stride must be 1, got {t.stride(2)}")
    batch, rows, cols = t.shape
    ld = t.stride(1) if rows > 1 else max(t.stride(1), cols)
    return (batch, rows, cols, ld, t.stride(0) if batch > 1 else rows * ld, *_BILINEAR_DTYPES[t.dtype])


def _bilinear_list(tokens: torch.Tensor, R: int, n: int, dev, fn: str) -> torch.Tensor:
    """The list of a bilinear entry: int8 (K,3n^2) on ``dev`` with K >= R, made contiguous."""
    _need_gpu(tokens, "tokens")
    if tokens.dtype != torch.int8 or tokens.dim() != 2 or tokens.shape[1] != 3 * n * n or tokens.device != dev:
        raise TensorGameError(fn, -1, f"tokens must be int8 (K,{3 * n * n}) on {dev}, got {tokens.dtype} "
                                      f"{tuple(tokens.shape)} on {tokens.device}")
    if R > tokens.shape[0]:
        raise TensorGameError(fn, -1, f"R={R} above the K={tokens.shape[0]} rows of tokens")
    return tokens if tokens.is_contiguous() else tokens.contiguous()


def _bilinear_decode_out(M: torch.Tensor, R: int, gr: int, gc: int, out, fn: str) -> torch.Tensor:
    """The checks of a decode's M (contiguous (batch,R,h,w)) and of its ``out`` (batch,gr*h,gc*w), which is made where
    none is given."""
    _need_gpu(M, "M")
    if M.dtype not in _BILINEAR_DTYPES or M.dim() != 4 or M.shape[1] != R or not M.is_contiguous():
        raise TensorGameError(fn, -1, f"M must be contiguous float32 or float64 (batch,R={R},h,w), got {M.dtype} "
                                      f"{tuple(M.shape)}")
    shape = (M.shape[0], gr * M.shape[2], gc * M.shape[3])
    if out is None:
        return torch.empty(shape, dtype=M.dtype, device=M.device)
    if out.dtype != M.dtype or tuple(out.shape) != shape or out.device != M.device:
        raise TensorGameError(fn, -1, f"out must be {M.dtype} {shape} on {M.device}, got {out.dtype} {tuple(out.shape)} "
                                      f"on {out.device}")
    return out


def bilinear_encode(X, tokens, R: int, n: int, mode: int, shift: int = 1, out=None) -> torch.Tensor:
    """The R block combinations of ``batch`` matrices in one launch (include/tensor_game_bilinear.h): X float32 or
    float64 (batch,rows,cols), any row and batch stride (a view is not copied), cut into n x n blocks of (h,w);
    tokens int8 (K,3n^2), of which rows 0 .. R-1 and part ``mode`` (0: u, for the left operand; 1: v, for the right
    one) are used.  Returns ``out`` (batch,R,h,w), contiguous: out[b][r] = sum_a (tokens[r][mode*S+a] - shift) * block a
    of X[b], by the header's arithmetic rule.  No host sync."""
    fn = "bilinear_encode"
    batch, rows, cols, ld, stride, suffix, eb = _bilinear_matrices(X, "X", fn)
    bilinear_check(batch, rows, cols, ld, stride, R, n, mode, shift, eb)
    tokens = _bilinear_list(tokens, R, n, X.device, fn)
    if out is not None:
        _need_gpu(out, "out")
    out = _out(out, (batch, int(R), rows // n, cols // n), X.dtype, X.device, "out")
    _launch(X.device, f"tg_bilinear_encode_{suffix}", _ptr(X), batch, rows, cols, ld, stride, _ptr(tokens), int(R), int(n),
            int(mode), int(shift), _ptr(out))
    return out


def bilinear_decode(M, tokens, R: int, n: int, shift: int = 1, out=None) -> torch.Tensor:
    """The n x n blocks of ``batch`` result matrices from the R block products, in one launch: M float32 or float64
    (batch,R,h,w), contiguous; part 2 (w) of rows 0 .. R-1 of tokens is used.  Returns ``out`` (batch,n*h,n*w), which
    may be a strided view when given (column stride 1): block c of out[b] = sum_r (tokens[r][2S+c] - shift) * M[b][r].
    Every element is written.  No host sync."""
    fn = "bilinear_decode"
    out = _bilinear_decode_out(M, R, n, n, out, fn)
    batch, rows, cols, ld, stride, suffix, eb = _bilinear_matrices(out, "out", fn)
    bilinear_check(batch, rows, cols, ld, stride, R, n, 0, shift, eb)
    tokens = _bilinear_list(tokens, R, n, M.device, fn)
    _launch(M.device, f"tg_bilinear_decode_{suffix}", _ptr(M), batch, rows, cols, ld, stride, _ptr(tokens), int(R), int(n),
            int(shift), _ptr(out))
    return out


def reset_matmul_rect(out, n: int, m: int, p: int):
    """The target <n,m,p> of include/tensor_game_rect.h into every game of ``out`` int8 (B,S,S,S), in one launch: entry
    (i*m+j, j*p+k, i*p+k) is 1, every other entry 0.  S >= max(n*m, m*p, n*p); the bytes between games stay."""
    B, S, stride = _state_layout(out, "out")
    _launch(out.device, "tg_reset_matmul_rect_i8", _ptr(out), B, int(n), int(m), int(p), S, stride)
    return out


def bilinear_rect_check(batch: int, rows: int, cols: int, ld: Optional[int] = None, batch_stride: Optional[int] = None,
                        R: int = 1, S: int = 4, gr: int = 2, gc: int = 2, part: int = 0, shift: int = 1,
                        elem_bytes: int = 4) -> None:
    """Raise TensorGameError (naming the argument) unless tg_bilinear_rect_encode_* / tg_bilinear_rect_decode_* take
    these sizes (``ld`` defaults to ``cols``, ``batch_stride`` to ``rows * ld``).  Host only."""
    ld = cols if ld is None else ld
    call("tg_bilinear_rect_check", int(batch), int(rows), int(cols), int(ld),
         int(rows * ld if batch_stride is None else batch_stride), int(R), int(S), int(gr), int(gc), int(part), int(shift),
         int(elem_bytes))


def _bilinear_rect_list(tokens: torch.Tensor, R: int, dev, fn: str):
    """(tokens made contiguous, S) of a list of cube size S: int8 (K,3S) on ``dev`` with K >= R."""
    _need_gpu(tokens, "tokens")
    if tokens.dtype != torch.int8 or tokens.dim() != 2 or tokens.shape[1] % 3 or tokens.device != dev:
        raise TensorGameError(fn, -1, f"tokens must be int8 (K,3S) on {dev}, got {tokens.dtype} {tuple(tokens.shape)} on "
                                      f"{tokens.device}")
    if R > tokens.shape[0]:
        raise TensorGameError(fn, -1, f"R={R} above the K={tokens.shape[0]} rows of tokens")
    return (tokens if tokens.is_contiguous() else tokens.contiguous()), tokens.shape[1] // 3


def bilinear_rect_encode(X, tokens, R: int, gr: int, gc: int, part: int, shift: int = 1, out=None) -> torch.Tensor:
    """The R block combinations of ``batch`` matrices in one launch (include/tensor_game_rect.h): X float32 or float64
    (batch,rows,cols), any row and batch stride (a view is not copied), cut into gr x gc blocks of (h,w); tokens int8
    (K,3S) with S >= gr*gc, of which rows 0 .. R-1 and the first gr*gc entries of part ``part`` (0: u, 1: v) are used.
    Returns ``out`` (batch,R,h,w), contiguous: out[b][r] = sum_e (tokens[r][part*S+e] - shift) * block e of X[b], by the
    header's arithmetic rule.  No host sync."""
    fn = "bilinear_rect_encode"
    batch, rows, cols, ld, stride, suffix, eb = _bilinear_matrices(X, "X", fn)
    tokens, S = _bilinear_rect_list(tokens, R, X.device, fn)
    bilinear_rect_check(batch, rows, cols, ld, stride, R, S, gr, gc, part, shift, eb)
    if out is not None:
        _need_gpu(out, "out")
    out = _out(out, (batch, int(R), rows // gr, cols // gc), X.dtype, X.device, "out")
    _launch(X.device, f"tg_bilinear_rect_encode_{suffix}", _ptr(X), batch, rows, cols, ld, stride, _ptr(tokens), int(R), S,
            int(gr), int(gc), int(part), int(shift), _ptr(out))
    return out


def bilinear_rect_decode(M, tokens, R: int, gr: int, gc: int, shift: int = 1, out=None) -> torch.Tensor:
    """The gr x gc blocks of ``batch`` result matrices from the R block products, in one launch: M float32 or float64
    (batch,R,h,w), contiguous; the first gr*gc entries of part 2 (w) of rows 0 .. R-1 of tokens are used.  Returns ``out``
    (batch,gr*h,gc*w), which may be a strided view when given (column stride 1): block e of out[b] = sum_r
    (tokens[r][2S+e] - shift) * M[b][r].  Every element is written.  No host sync."""
    fn = "bilinear_rect_decode"
    out = _bilinear_decode_out(M, R, gr, gc, out, fn)
    batch, rows, cols, ld, stride, suffix, eb = _bilinear_matrices(out, "out", fn)
    tokens, S = _bilinear_rect_list(tokens, R, M.device, fn)
    bilinear_rect_check(batch, rows, cols, ld, stride, R, S, gr, gc, 2, shift, eb)
    _launch(M.device, f"tg_bilinear_rect_decode_{suffix}", _ptr(M), batch, rows, cols, ld, stride, _ptr(tokens), int(R), S,
            int(gr), int(gc), int(shift), _ptr(out))
    return out


_PRODUCTS_DTYPES = {torch.bfloat16: "bf16", torch.float16: "f16"}


def bilinear_products_check(batch: int, P: int, Q: int, T: int, lda: Optional[int] = None, stride_a: Optional[int] = None,
                            ldb: Optional[int] = None, stride_b: Optional[int] = None, R: int = 1, S: int = 4, n: int = 2,
                            m: int = 2, p: int = 2, shift: int = 1) -> None:
    """Raise TensorGameError (naming the argument) unless tg_bilinear_products_* take these sizes (``lda`` defaults to Q,
    ``ldb`` to T, the batch strides to rows * ld).  Host only."""
    lda, ldb = Q if lda is None else lda, T if ldb is None else ldb
    call("tg_bilinear_products_check", int(batch), int(P), int(Q), int(T), int(lda),
         int(P * lda if stride_a is None else stride_a), int(ldb), int(Q * ldb if stride_b is None else stride_b), int(R),
         int(S), int(n), int(m), int(p), int(shift))


def _products_matrices(t: torch.Tensor, name: str, fn: str):
    """(batch, rows, cols, ld, batch_stride) of a strided bfloat16 or float16 (batch,rows,cols) view, which is taken as it
    is (no copy): only the column stride is held to 1."""
    _need_gpu(t, name)
    if t.dtype not in _PRODUCTS_DTYPES or t.dim() != 3:
        raise TensorGameError(fn, -1, f"{name} must be bfloat16 or float16 (batch,rows,cols), got {t.dtype} "
                                      f"{tuple(t.shape)}")
    if t.stride(2) != 1:
        raise TensorGameError(fn, -1, f"{name}: the column stride must be 1, got {t.stride(2)}")
    batch, rows, cols = t.shape
    ld = t.stride(1) if rows > 1 else max(t.stride(1), cols)
    return batch, rows, cols, ld, t.stride(0) if batch > 1 else rows * ld


def bilinear_products(A, B, tokens, R: int, n: int, m: int, p: int, shift: int = 1, out=None) -> torch.Tensor:
    """The R block products of a bilinear algorithm for <n,m,p> in one launch (include/tensor_game_products.h): A (batch,P,Q)
    and B (batch,Q,T), both bfloat16 or both float16, any row and batch stride (a view is not copied), A cut into n x m
    blocks and B into m x p; tokens int8 (K,3S), of which rows 0 .. R-1 and the first n*m entries of part 0 and m*p of part 1
    are used.  Returns ``out`` float32 (batch,R,P/n,T/p), contiguous: out[b][r] = rn(sum_e u_r[e] * block e of A[b]) times
    rn(sum_e v_r[e] * block e of B[b]), the combinations rounded to the operands' type and never written to memory, the
    products accumulated in float32 on the matrix cores.  No host sync."""
    fn = "bilinear_products"
    batch, P, Q, lda, stride_a = _products_matrices(A, "A", fn)
    batch_b, Q2, T, ldb, stride_b = _products_matrices(B, "B", fn)
    if A.dtype != B.dtype:
        raise TensorGameError(fn, -1, f"mixed dtypes: A is {A.dtype}, B is {B.dtype}")
    if batch_b != batch or Q2 != Q or B.device != A.device:
        raise TensorGameError(fn, -1, f"A {tuple(A.shape)} on {A.device} and B {tuple(B.shape)} on {B.device} do not "
                                      "multiply: equal batch, Q and device are required")
    tokens, S = _bilinear_rect_list(tokens, R, A.device, fn)
    bilinear_products_check(batch, P, Q, T, lda, stride_a, ldb, stride_b, R, S, n, m, p, shift)
    if out is not None:
        _need_gpu(out, "out")
    out = _out(out, (batch, int(R), P // int(n), T // int(p)), torch.float32, A.device, "out")
    _launch(A.device, f"tg_bilinear_products_{_PRODUCTS_DTYPES[A.dtype]}", _ptr(A), _ptr(B), batch, P, Q, T, lda, stride_a,
            ldb, stride_b, _ptr(tokens), int(R), S, int(n), int(m), int(p), int(shift), _ptr(out))
    return out
