"""Every refusal of mat_mul_amd/ops.py, characterised without a device.

``CASES`` is a table of named calls, each with one bad argument (a few with two, to pin the order of the checks).  Every
tensor is a ``Cuda`` stand-in that says it lives on a ROCm device, every optional output is supplied, forests and buffers
are ``types.SimpleNamespace``: no call allocates or launches before the check under test raises.

``tests/golden/ops_errors.json`` holds what the PARENT of the commit that introduced the argument helpers raised for every
case: exception type, ``code``, the full message, and the line of that parent's ops.py that raised (the line is for the
coverage count only).  It is recorded by

    git show <parent>:mat_mul_amd/ops.py > parent_ops.py
    python tests/test_ops_errors_cpu.py --record --ops parent_ops.py

and never from the refactored code.  The test compares type, code and message of today's ops.py with it.

The one intended difference is listed apart (``INTENDED``): ``change_basis`` now refuses an ``out`` on another device,
and the message of its out check says so.
"""
import ast
import importlib.util
import json
import sys
import traceback
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = Path(__file__).resolve().parent / "golden" / "ops_errors.json"
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from mat_mul_amd import _lib, ops  # noqa: E402

from net_ref import CONFIGS, dims  # noqa: E402

DEV, OTHER = torch.device("cuda:0"), torch.device("cuda:1")
i8, u8, i32, u32, i64, f16, f32, f64 = (torch.int8, torch.uint8, torch.int32, torch.uint32, torch.int64, torch.float16,
                                        torch.float32, torch.float64)

# raise lines of the parent's ops.py that no case reaches, each with the reason
UNCOVERED = {
    157: "prepare_step's launch closure reports the return code of a launch",
    252: "step_stream's progress size check comes after step_stream_layout, a device query",
}
MAX_UNCOVERED = 5


class Cuda:
    """A CPU tensor that says it lives on a ROCm device; what returns a tensor of the same place returns a stand-in."""

    is_cuda = True

    def __init__(self, t, device=DEV):
        self._t, self.device = t, device

    def contiguous(self):
        return self if self._t.is_contiguous() else Cuda(self._t.contiguous(), self.device)

    def to(self, device, dtype):
        return Cuda(self._t.to(dtype), torch.device(device))

    def __getattr__(self, name):
        return getattr(self._t, name)


def t(shape, dtype=i8, device=DEV):
    return Cuda(torch.zeros(shape, dtype=dtype), device)


def view(fn, shape, dtype=i8, device=DEV):
    """A stand-in for ``fn(zeros(shape))``: a transposed, sliced or restrided view."""
    return Cuda(fn(torch.zeros(shape, dtype=dtype)), device)


def games(B, S=4, device=DEV):
    return t((B, S, S, S), device=device)


def padded(B, S, stride):
    return view(lambda z: z[:, :S ** 3].unflatten(1, (S, S, S)), (B, stride))


CASES = {}


def case(name, fn, base, **bad):
    assert name not in CASES, name
    CASES[name] = (fn, base, bad)


def cases(fn, base, **named):
    for name, bad in named.items():
        case(f"{fn}.{name}", fn, base, **bad)


# ---- the state entries ---------------------------------------------------------------------------------------------
STATE = games(3)
FLAG3 = t((3,), u8)
STEP = dict(state=STATE, actions=t((3, 12)), out=games(3), done=t((3,), u8), overflow=FLAG3)
cases("step", STEP,
      state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)),
      state_dtype=dict(state=t((3, 4, 4, 4), i32)),
      state_dim=dict(state=t((3, 4, 4))),
      state_not_cubic=dict(state=t((3, 4, 4, 5))),
      state_transposed=dict(state=view(lambda z: z.transpose(2, 3), (3, 4, 4, 4))),
      state_overlapping=dict(state=view(lambda z: z.as_strided((3, 4, 4, 4), (32, 16, 4, 1)), (128,))),
      actions_cpu=dict(actions=torch.zeros((3, 12), dtype=i8)),
      actions_dtype=dict(actions=t((3, 12), i64)),
      actions_shape=dict(actions=t((3, 11))),
      actions_device=dict(actions=t((3, 12), device=OTHER)),
      out_cpu=dict(out=torch.zeros((3, 4, 4, 4), dtype=i8)),
      out_dtype=dict(out=t((3, 4, 4, 4), f32)),
      out_batch=dict(out=games(2)),
      out_size=dict(out=games(3, 5)),
      out_stride=dict(out=padded(3, 4, 128)),
      out_device=dict(out=games(3, device=OTHER)),
      done_dtype=dict(done=t((3,), i32)),
      done_shape=dict(done=t((4,), u8)),
      done_device=dict(done=t((3,), u8, OTHER)),
      done_strided=dict(done=view(lambda z: z[::2], (6,), u8)),
      overflow_shape=dict(overflow=t((3, 1), u8)),
      state_then_actions=dict(state=t((3, 4, 4)), actions=t((3, 11))),
      actions_then_out=dict(actions=t((3, 11)), out=games(2)),
      out_then_done=dict(out=games(2), done=t((4,), u8)),
      done_then_overflow=dict(done=t((4,), u8), overflow=t((4,), u8)))
cases("copy_states", dict(state=STATE, out=padded(3, 4, 128)),
      state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)),
      out_dtype=dict(out=t((3, 4, 4, 4), u8)),
      out_batch=dict(out=games(4)),
      out_device=dict(out=games(3, device=OTHER)))
cases("prepare_step", dict(state=STATE, actions_seq=[t((3, 12)), t((3, 12))], done=FLAG3, overflow=FLAG3),
      state_dtype=dict(state=t((3, 4, 4, 4), u8)),
      actions_shape=dict(actions_seq=[t((3, 12)), t((2, 12))]),
      done_dtype=dict(done=t((3,), i8)),
      overflow_shape=dict(overflow=t((2,), u8)))
cases("step_many", dict(state=STATE, actions=t((3, 3, 12)), out=games(3), done_step=t((3,), i32), overflow=FLAG3),
      state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)),
      actions_dim=dict(actions=t((3, 12))),
      actions_shape=dict(actions=t((2, 3, 12))),
      out_batch=dict(out=games(2)),
      out_stride=dict(out=padded(3, 4, 80)),
      out_device=dict(out=games(3, device=OTHER)),
      done_step_dtype=dict(done_step=t((3,), u8)),
      overflow_dtype=dict(overflow=t((3,), i32)),
      dim_then_out=dict(actions=t((3, 12)), out=games(2)),
      out_then_done_step=dict(out=games(2), done_step=t((3,), u8)))
cases("step_tracked", dict(state=STATE, actions=t((3, 12)), nnz=t((3,), i32), done=FLAG3, overflow=FLAG3),
      actions_dtype=dict(actions=t((3, 12), u8)),
      nnz_dtype=dict(nnz=t((3,), i64)),
      nnz_shape=dict(nnz=t((2,), i32)),
      nnz_device=dict(nnz=t((3,), i32, OTHER)),
      done_shape=dict(done=t((2,), u8)),
      overflow_dtype=dict(overflow=t((3,), i8)),
      nnz_then_done=dict(nnz=t((2,), i32), done=t((2,), u8)))
cases("step_stream", dict(state=STATE, actions=t((3, 3, 12)), done=t((3, 3), u8), overflow=FLAG3, ready=t((3,), i32),
                          progress=None, status=t((1,), i32)),
      state_dim=dict(state=t((3, 4, 4))),
      actions_dim=dict(actions=t((3, 12))),
      actions_shape=dict(actions=t((3, 2, 12))),
      done_shape=dict(done=t((3,), u8)),
      overflow_shape=dict(overflow=t((3, 3), u8)),
      ready_size=dict(ready=t((2,), i32)),
      ready_dtype=dict(ready=t((3,), i64)),
      progress_dtype=dict(progress=t((4,), f32)),
      progress_device=dict(progress=t((4,), i32, OTHER)),
      status_size=dict(status=t((2,), u32)),
      done_then_ready=dict(done=t((3,), u8), ready=t((2,), i32)))
cases("expand", dict(state=STATE, actions=t((3, 3, 12)), out=t((3, 3, 4, 4, 4)), done=t((3, 3), u8), changed=t((3, 3), u8),
                     overflow=t((3, 3), u8), keys=t((3, 3), i64)),
      state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)),
      actions_dim=dict(actions=t((3, 12))),
      actions_shape=dict(actions=t((3, 3, 15))),
      out_dtype=dict(out=t((3, 3, 4, 4, 4), u8)),
      out_shape=dict(out=t((3, 2, 4, 4, 4))),
      out_device=dict(out=t((3, 3, 4, 4, 4), device=OTHER)),
      out_transposed=dict(out=view(lambda z: z.transpose(3, 4), (3, 3, 4, 4, 4))),
      out_sliced=dict(out=view(lambda z: z[:, :3], (3, 5, 4, 4, 4))),
      out_overlapping=dict(out=view(lambda z: z.as_strided((3, 3, 4, 4, 4), (96, 32, 16, 4, 1)), (512,))),
      done_shape=dict(done=t((3,), u8)),
      changed_dtype=dict(changed=t((3, 3), i8)),
      overflow_shape=dict(overflow=t((3,), u8)),
      keys_dtype=dict(keys=t((3, 3), i32)),
      keys_shape=dict(keys=t((9,), i64), want_keys=True),
      out_then_done=dict(out=t((3, 2, 4, 4, 4)), done=t((3,), u8)),
      done_then_changed=dict(done=t((3,), u8), changed=t((3,), u8)),
      overflow_then_keys=dict(overflow=t((3,), u8), keys=t((3,), i64)))
cases("done", dict(state=STATE), state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)), state_dtype=dict(state=t((3, 4, 4, 4), f32)))
cases("reset_matmul", dict(out=STATE, n=2), out_cpu=dict(out=torch.zeros((3, 4, 4, 4), dtype=i8)), n=dict(n=3))
cases("reset_broadcast", dict(out=STATE, start=t((4, 4, 4))),
      out_dim=dict(out=t((4, 4, 4))),
      start_cpu=dict(start=torch.zeros((4, 4, 4), dtype=i8)),
      start_shape=dict(start=t((1, 4, 4, 4))),
      start_dtype=dict(start=t((4, 4, 4), u8)),
      start_device=dict(start=t((4, 4, 4), device=OTHER)))
cases("gen_from_factors", dict(actions=t((3, 2, 12)), S=4, out=games(3), overflow=FLAG3),
      actions_cpu=dict(actions=torch.zeros((3, 2, 12), dtype=i8)),
      actions_dim=dict(actions=t((3, 12))),
      actions_dtype=dict(actions=t((3, 2, 12), i64)),
      actions_width=dict(S=5),
      out_dtype=dict(out=t((3, 4, 4, 4), i32)),
      out_batch=dict(out=games(2)),
      out_device=dict(out=games(3, device=OTHER)),
      overflow_shape=dict(overflow=t((2,), u8)),
      out_then_overflow=dict(out=games(2), overflow=t((2,), u8)))
cases("categorical_thresholds", dict(probs=(0.2, 0.8)),
      empty=dict(probs=()), negative=dict(probs=(0.5, -0.1)), zero=dict(probs=(0.0, 0.0)),
      too_many=dict(probs=(1.0,) * (_lib.TG_MAX_VALUES + 1)), matrix=dict(probs=((0.5, 0.5),)))
cases("gen_demos", dict(B=3, S=4, R=2, device="cuda:0", target=games(3), actions=t((3, 2, 12)), overflow=FLAG3,
                        basis=t((3, 3, 4, 4))),
      values_range=dict(values=(-200, 0, 1)),
      values_count=dict(values=(-1, 1)),
      probs_negative=dict(probs=(0.5, 0.6, -0.1)),
      never_non_zero=dict(values=(-1, 0, 1), probs=(0.0, 1.0, 0.0)),
      target_cpu=dict(target=torch.zeros((3, 4, 4, 4), dtype=i8)),
      target_batch=dict(target=games(2)),
      actions_shape=dict(actions=t((3, 3, 12))),
      actions_dtype=dict(actions=t((3, 2, 12), u8)),
      actions_device=dict(actions=t((3, 2, 12), device=OTHER)),
      overflow_dtype=dict(overflow=t((3,), i8)),
      basis_dtype=dict(basis=t((3, 3, 4, 4), i32)),
      basis_shape=dict(basis=t((3, 4, 4))),
      values_then_target=dict(values=(-1, 1), target=games(2)),
      overflow_then_basis=dict(overflow=t((2,), u8), basis=t((3, 4, 4))))
cases("sample_basis", dict(B=3, S=4, device="cuda:0"),
      values_count=dict(values=(-1, 1)),
      values_too_large=dict(values=(-6, 0, 6), probs=(0.1, 0.8, 0.1)),
      never_non_zero=dict(values=(0,), probs=(1.0,)))
CHANGE_BASIS = dict(state=STATE, basis=t((3, 3, 4, 4), i32), out=games(3), overflow=FLAG3)
cases("change_basis", CHANGE_BASIS,
      state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)),
      basis_dtype=dict(basis=t((3, 3, 4, 4), i8)),
      basis_shape=dict(basis=t((3, 3, 4, 5), i32)),
      basis_device=dict(basis=t((3, 3, 4, 4), i32, OTHER)),
      out_dtype=dict(out=t((3, 4, 4, 4), f16)),
      in_place=dict(out=STATE),
      overflow_shape=dict(overflow=t((4,), u8)),
      basis_then_out=dict(basis=t((3, 3, 4, 4), i8), out=games(4)))

# ---- the history ring ----------------------------------------------------------------------------------------------
RING = dict(ring=t((3, 2, 4, 4, 4)), head_slot=0, dtype=f32, out=t((3, 2, 4, 4, 4), f32), scalars=t((3, 1), f32))
RING_BAD = dict(
    ring_cpu=dict(ring=torch.zeros((3, 2, 4, 4, 4), dtype=i8)),
    ring_dtype=dict(ring=t((3, 2, 4, 4, 4), u8)),
    ring_dim=dict(ring=t((3, 4, 4, 4))),
    ring_not_cubic=dict(ring=t((3, 2, 4, 4, 3))),
    ring_transposed=dict(ring=view(lambda z: z.transpose(2, 3), (3, 2, 4, 4, 4))),
    dtype=dict(dtype=f64),
    dtype_int8=dict(dtype=i8),
    out_dtype=dict(out=t((3, 2, 4, 4, 4), f16)),
    out_shape=dict(out=t((3, 1, 4, 4, 4), f32)),
    out_device=dict(out=t((3, 2, 4, 4, 4), f32, OTHER)),
    out_strided=dict(out=view(lambda z: z[:, :2], (3, 3, 4, 4, 4), f32)),
    scalars_shape=dict(scalars=t((3,), f32)),
    scalars_dtype=dict(scalars=t((3, 1), f16)),
    ring_then_dtype=dict(ring=view(lambda z: z.transpose(2, 3), (3, 2, 4, 4, 4)), dtype=f64),
    dtype_then_out=dict(dtype=f64, out=t((3, 1, 4, 4, 4), f32)),
    out_then_scalars=dict(out=t((3, 1, 4, 4, 4), f32), scalars=t((3,), f32)))
cases("emit_frames", RING, **RING_BAD)
cases("step_emit", dict(RING, actions=t((3, 12)), done=FLAG3, overflow=FLAG3), **RING_BAD,
      actions_shape=dict(actions=t((3, 13))),
      actions_device=dict(actions=t((3, 12), device=OTHER)),
      done_dtype=dict(done=t((3,), i32)),
      overflow_shape=dict(overflow=t((1,), u8)),
      dtype_then_actions=dict(dtype=f64, actions=t((3, 13))),
      actions_then_out=dict(actions=t((3, 13)), out=t((3, 1, 4, 4, 4), f32)),
      scalars_then_done=dict(scalars=t((3,), f32), done=t((3,), i32)))

# ---- items ---------------------------------------------------------------------------------------------------------
ITEM_OUT = dict(out=t((5, 2, 4, 4, 4), f32), scalars=t((5, 1), f32), actions=t((5, 12)), rewards=t((5, 1), f32),
                overflow=t((5,), u8), status=t((1,), u32))
ITEM_BAD = dict(
    idx_cpu=dict(idx=torch.zeros((5,), dtype=i64)),
    idx_dtype=dict(idx=t((5,), i32)),
    idx_dim=dict(idx=t((5, 1), i64)),
    idx_device=dict(idx=t((5,), i64, OTHER)),
    dtype=dict(dtype=f64),
    out_dtype=dict(out=t((5, 2, 4, 4, 4), i8)),
    out_int8_for_int8=dict(dtype=i8, out=t((5, 2, 4, 4, 4), f32)),
    out_shape=dict(out=t((4, 2, 4, 4, 4), f32)),
    out_device=dict(out=t((5, 2, 4, 4, 4), f32, OTHER)),
    scalars_shape=dict(scalars=t((5,), f32)),
    actions_dtype=dict(actions=t((5, 12), i64)),
    rewards_shape=dict(rewards=t((5, 2), f32)),
    overflow_dtype=dict(overflow=t((5,), i8)),
    status_dtype=dict(status=t((1,), i32)),
    status_shape=dict(status=t((2,), u32)),
    idx_then_dtype=dict(idx=t((5,), i32), dtype=f64),
    dtype_then_out=dict(dtype=f64, out=t((4, 2, 4, 4, 4), f32)),
    out_then_scalars=dict(out=t((4, 2, 4, 4, 4), f32), scalars=t((5,), f32)),
    scalars_then_actions=dict(scalars=t((5,), f32), actions=t((5, 12), i64)),
    rewards_then_overflow=dict(rewards=t((5, 2), f32), overflow=t((5,), i8)))
cases("demo_items", dict(ITEM_OUT, tokens=t((3, 3, 12)), targets=games(3), idx=t((5,), i64), T=2, dtype=f32), **ITEM_BAD,
      targets_cpu=dict(targets=torch.zeros((3, 4, 4, 4), dtype=i8)),
      targets_dtype=dict(targets=t((3, 4, 4, 4), f32)),
      tokens_cpu=dict(tokens=torch.zeros((3, 3, 12), dtype=i8)),
      tokens_dim=dict(tokens=t((9, 12))),
      tokens_count=dict(tokens=t((2, 3, 12))),
      tokens_width=dict(tokens=t((3, 3, 15))),
      tokens_then_idx=dict(tokens=t((9, 12)), idx=t((5,), i32)))
PLAYED = types.SimpleNamespace(S=4, T=2, device=DEV, desc=None)
cases("replay_items", dict(ITEM_OUT, idx=t((5,), i64), T=2, S=4, device="cuda:0", tokens=t((3, 3, 12)), targets=games(3),
                           played=None, best=None, kind=None, src=None, direct_kind=0, dtype=f32), **ITEM_BAD,
      tokens_alone=dict(targets=None),
      targets_alone=dict(tokens=None),
      targets_size=dict(targets=games(3, 5)),
      targets_device=dict(targets=games(3, device=OTHER)),
      targets_dtype=dict(targets=t((3, 4, 4, 4), u8)),
      tokens_cpu=dict(tokens=torch.zeros((3, 3, 12), dtype=i8)),
      tokens_dim=dict(tokens=t((9, 12))),
      tokens_count=dict(tokens=t((2, 3, 12))),
      tokens_dtype=dict(tokens=t((3, 3, 12), i32)),
      played_size=dict(played=types.SimpleNamespace(S=5, T=2, device=DEV, desc=None)),
      best_frames=dict(played=PLAYED, best=types.SimpleNamespace(S=4, T=1, device=DEV, desc=None)),
      best_device=dict(best=types.SimpleNamespace(S=4, T=2, device=OTHER, desc=None)),
      table_and_direct=dict(kind=t((7,), u8), src=t((7,), i64)),
      table_without_src=dict(kind=t((7,), u8), direct_kind=None),
      kind_dtype=dict(kind=t((7,), i8), src=t((7,), i64), direct_kind=None),
      kind_dim=dict(kind=t((7, 1), u8), src=t((7,), i64), direct_kind=None),
      src_shape=dict(kind=t((7,), u8), src=t((6,), i64), direct_kind=None),
      direct_kind=dict(direct_kind=3),
      direct_kind_missing=dict(direct_kind=None),
      idx_then_sources=dict(idx=t((5,), i32), targets=None),
      sources_then_played=dict(targets=None, played=types.SimpleNamespace(S=5, T=2, device=DEV, desc=None)),
      played_then_kind=dict(played=types.SimpleNamespace(S=5, T=2, device=DEV, desc=None), direct_kind=3),
      kind_then_dtype=dict(direct_kind=3, dtype=f64))

# ---- keys, the seen table, as_tokens -------------------------------------------------------------------------------
cases("state_hash", dict(state=STATE), state_cpu=dict(state=torch.zeros((3, 4, 4, 4), dtype=i8)))
cases("slice_rank", dict(state=STATE), state_dtype=dict(state=t((3, 4, 4, 4), i64)))
cases("alloc_seen_table", dict(capacity=8, device="cpu"), three=dict(capacity=3), one=dict(capacity=1))
cases("seen", dict(keys=t((3, 3), i64), table=t((8,), i64), mask=t((3, 3), u8), status=t((1,), i32), fresh=t((3, 3), u8)),
      keys_cpu=dict(keys=torch.zeros((3, 3), dtype=i64)),
      table_cpu=dict(table=torch.zeros((8,), dtype=i64)),
      keys_dtype=dict(keys=t((3, 3), i32)),
      keys_strided=dict(keys=view(lambda z: z[:, :3], (3, 4), i64)),
      table_dtype=dict(table=t((8,), u8)),
      table_dim=dict(table=t((2, 4), i64)),
      table_device=dict(table=t((8,), i64, OTHER)),
      mask_shape=dict(mask=t((9,), u8)),
      fresh_dtype=dict(fresh=t((3, 3), i8)),
      status_dtype=dict(status=t((1,), f32)),
      status_size=dict(status=t((2,), i32)),
      status_device=dict(status=t((1,), u32, OTHER)),
      mask_then_fresh=dict(mask=t((9,), u8), fresh=t((9,), u8)),
      fresh_then_status=dict(fresh=t((9,), u8), status=t((2,), i32)))
cases("as_tokens", dict(actions=[1, 2]), floating=dict(actions=[0.5]), too_large=dict(actions=[1, 200]),
      too_small=dict(actions=torch.tensor([-129])))

# ---- the search forest and the replay buffers ----------------------------------------------------------------------
FOREST = types.SimpleNamespace(B=3, T=2, S=4, k=2, max_actions=5, device=DEV, desc=None)
cases("search_reset", dict(forest=FOREST, states=t((3, 2, 4, 4, 4)), n_sim=4),
      states_cpu=dict(states=torch.zeros((3, 2, 4, 4, 4), dtype=i8)),
      states_dtype=dict(states=t((3, 2, 4, 4, 4), f32)),
      states_shape=dict(states=t((3, 1, 4, 4, 4))),
      states_device=dict(states=t((3, 2, 4, 4, 4), device=OTHER)))
cases("search_select", dict(forest=FOREST, model_in=t((3, 2, 4, 4, 4), f32), scalars=t((3, 1), f32)),
      model_in_dtype=dict(model_in=t((3, 2, 4, 4, 4), f64)),
      model_in_int8=dict(model_in=t((3, 2, 4, 4, 4), i8)),
      model_in_shape=dict(model_in=t((2, 2, 4, 4, 4), f16)),
      model_in_device=dict(model_in=t((3, 2, 4, 4, 4), torch.bfloat16, OTHER)),
      model_in_strided=dict(model_in=view(lambda z: z[:, :2], (3, 3, 4, 4, 4), f32)),
      scalars_shape=dict(scalars=t((3,), f32)),
      scalars_alone=dict(model_in=None, scalars=t((3, 1), f16)),
      model_in_then_scalars=dict(model_in=t((2, 2, 4, 4, 4), f16), scalars=t((3,), f32)))
cases("search_commit", dict(forest=FOREST, tokens=t((3, 2, 12)), leaf_q=t((3,), f32), prior=t((3, 2), f32), mask=FLAG3),
      tokens_cpu=dict(tokens=torch.zeros((3, 2, 12), dtype=i8)),
      tokens_shape=dict(tokens=t((3, 12))),
      leaf_q_dtype=dict(leaf_q=t((3,), f16)),
      prior_shape=dict(prior=t((3, 3), f32)),
      mask_dtype=dict(mask=t((3,), torch.bool)),
      leaf_q_then_prior=dict(leaf_q=t((3,), f16), prior=t((3, 3), f32)))
cases("search_policy", dict(forest=FOREST, n_logits=3, n_bar=4, out=t((3, 5, 12, 3), f32)),
      out_shape=dict(out=t((3, 5, 12, 4), f32)),
      out_dtype=dict(out=t((3, 5, 12, 3), f16)))
BUF = types.SimpleNamespace(L=4, T=2, S=4, device=DEV, desc=None)
cases("replay_add", dict(buf=BUF, states=t((3, 4, 2, 4, 4, 4)), policy=t((3, 4, 12, 3), f32), rewards=t((3, 4), f32),
                         lengths=t((3,), i64), status=t((1,), u32)),
      states_cpu=dict(states=torch.zeros((3, 4, 2, 4, 4, 4), dtype=i8)),
      lengths_cpu=dict(lengths=torch.zeros((3,), dtype=i64)),
      states_dim=dict(states=t((3, 4, 4, 4, 4))),
      states_shape=dict(states=t((3, 5, 2, 4, 4, 4))),
      states_dtype=dict(states=t((3, 4, 2, 4, 4, 4), f32)),
      policy_dtype=dict(policy=t((3, 4, 12, 3), f16)),
      policy_shape=dict(policy=t((3, 4, 11, 3), f32)),
      policy_device=dict(policy=t((3, 4, 12, 3), f32, OTHER)),
      no_logits=dict(policy=t((3, 4, 12, 0), f32)),
      too_many_logits=dict(policy=t((3, 4, 12, _lib.TG_REPLAY_MAX_LOGITS + 1), f32)),
      rewards_dtype=dict(rewards=t((3, 4), i64)),
      lengths_dtype=dict(lengths=t((3,), i32)),
      status_dtype=dict(status=t((1,), i32)),
      states_then_policy=dict(states=t((3, 5, 2, 4, 4, 4)), policy=t((3, 4, 11, 3), f32)),
      logits_then_rewards=dict(policy=t((3, 4, 12, 0), f32), rewards=t((3, 4), i64)))

# ---- the network ---------------------------------------------------------------------------------------------------
M = dims(CONFIGS["a"])
CFG = _lib.NetConfig(**M)
N_W = ops.net_weights_size(CFG)
N_WS = ops.net_train_workspace_size(CFG, 3)
W = t((N_W,), f32)
FRAMES, SCAL, EE = t((3, M["T"], 4, 4, 4)), t((3, M["dim_s"]), f32), t((3, 48, M["c"]), f32)
KEEP = (3, M["blocks"], 2, M["n_steps"], M["W"])
BLOB_BAD = dict(
    weights_cpu=torch.zeros((N_W,), dtype=f32),
    weights_dtype=t((N_W,), f16),
    weights_size=t((N_W - 1,), f32),
    weights_strided=view(lambda z: z[::2], (2 * N_W,), f32))
NET_TORSO = dict(cfg=CFG, w=W, frames=FRAMES, scalars=SCAL, out=EE, flags=FLAG3, need=1)
cases("net_torso", NET_TORSO, **{k: dict(w=v) for k, v in BLOB_BAD.items()},
      frames_cpu=dict(frames=torch.zeros((3, 2, 4, 4, 4), dtype=i8)),
      frames_dtype=dict(frames=t((3, 2, 4, 4, 4), f16)),
      frames_dim=dict(frames=t((3, 4, 4, 4))),
      frames_shape=dict(frames=t((3, 1, 4, 4, 4), f32)),
      frames_device=dict(frames=t((3, 2, 4, 4, 4), device=OTHER)),
      scalars_shape=dict(scalars=t((3, 2), f32)),
      scalars_dtype=dict(scalars=t((3, 1), f64)),
      need_zero=dict(need=0),
      need_large=dict(need=256),
      flags_dtype=dict(flags=t((3,), i8)),
      flags_shape=dict(flags=t((2,), u8)),
      out_shape=dict(out=t((3, 48, 4), f32)),
      out_shape_plain=dict(out=t((3, 48, 4), f32), flags=None, need=0),
      out_dtype=dict(out=t((3, 48, 8), f16)),
      weights_then_frames=dict(w=t((N_W - 1,), f32), frames=t((3, 4, 4, 4))),
      scalars_then_need=dict(scalars=t((3, 2), f32), need=0),
      need_then_out=dict(need=0, out=t((3, 48, 4), f32)))
cases("net_sample", dict(cfg=CFG, w=W, ee=EE, rows=t((3,), i64), k=2, seed=1, call_idx=2, uniforms=t((3, 2, 12), f32),
                         tokens=t((3, 2, 12)), probs=t((3, 2), f32), q=t((3,), f32), flags=FLAG3, need=1),
      weights_size=dict(w=t((N_W + 1,), f32)),
      need_zero=dict(need=0),
      flags_device=dict(flags=t((3,), u8, OTHER)),
      ee_shape=dict(ee=t((3, 48, 4), f32)),
      rows_dtype=dict(rows=t((3,), i32)),
      uniforms_shape=dict(uniforms=t((3, 2, 11), f32)),
      tokens_dtype=dict(tokens=t((3, 2, 12), i64)),
      tokens_shape=dict(tokens=t((3, 3, 12))),
      probs_shape=dict(probs=t((3,), f32)),
      q_dtype=dict(q=t((3,), f16)),
      q_shape_plain=dict(q=t((3, 1), f32), flags=None, need=0),
      need_then_ee=dict(need=0, ee=t((3, 48, 4), f32)),
      uniforms_then_tokens=dict(uniforms=t((3, 2, 11), f32), tokens=t((3, 3, 12))),
      tokens_then_probs=dict(tokens=t((3, 3, 12)), probs=t((3,), f32)))
cases("net_logits", dict(cfg=CFG, w=W, ee=EE, g_action=t((3, 12), i64)),
      weights_dtype=dict(w=t((N_W,), f64)),
      ee_dtype=dict(ee=t((3, 48, 8), f16)),
      g_action_cpu=dict(g_action=torch.zeros((3, 12), dtype=i64)),
      g_action_float=dict(g_action=t((3, 12), f32)),
      g_action_shape=dict(g_action=t((3, 11), i8)))
cases("net_loss_grad", dict(cfg=CFG, theta=W, pos_fix=t((M["n_steps"], M["W"]), f32), frames=FRAMES, scalars=SCAL,
                            g_action=t((3, 12)), g_value=t((3, 1), f32), workspace=t((N_WS,), u8), grad=t((N_W,), f32),
                            losses=t((2,), f32), status=t((1,), i32), keep_in=t(KEEP, u8), keep_out=t(KEEP, u8)),
      theta_size=dict(theta=t((N_W - 1,), f32)),
      frames_dtype=dict(frames=t((3, 2, 4, 4, 4), u8)),
      frames_dim=dict(frames=t((3, 4, 4, 4))),
      frames_device=dict(frames=t((3, 2, 4, 4, 4), f32, OTHER)),
      no_games=dict(frames=t((0, 2, 4, 4, 4))),
      dropout_one=dict(dropout_p=1.0),
      dropout_negative=dict(dropout_p=-0.5),
      pos_fix_shape=dict(pos_fix=t((M["W"], M["n_steps"]), f32)),
      scalars_shape=dict(scalars=t((3,), f32)),
      g_action_dtype=dict(g_action=t((3, 12), i64)),
      g_value_shape=dict(g_value=t((3,), f32)),
      keep_in_shape=dict(keep_in=t(KEEP[1:], u8)),
      keep_out_dtype=dict(keep_out=t(KEEP, torch.bool)),
      grad_shape=dict(grad=t((N_W - 1,), f32)),
      losses_shape=dict(losses=t((1,), f32)),
      status_dtype=dict(status=t((1,), u32)),
      workspace_cpu=dict(workspace=torch.zeros((N_WS,), dtype=u8)),
      workspace_small=dict(workspace=t((N_WS - 1,), u8)),
      workspace_dtype=dict(workspace=t((N_WS,), i8)),
      workspace_device=dict(workspace=t((N_WS,), u8, OTHER)),
      frames_then_games=dict(frames=t((3, 4, 4, 4)), dropout_p=1.0),
      games_then_dropout=dict(frames=t((0, 2, 4, 4, 4)), dropout_p=1.0),
      dropout_then_pos_fix=dict(dropout_p=1.0, pos_fix=t((M["W"], M["n_steps"]), f32)),
      keep_then_grad=dict(keep_out=t(KEEP, torch.bool), grad=t((N_W - 1,), f32)),
      grad_then_losses=dict(grad=t((N_W - 1,), f32), losses=t((1,), f32)),
      status_then_workspace=dict(status=t((1,), u32), workspace=t((N_WS - 1,), u8)))

# ---- rollouts ------------------------------------------------------------------------------------------------------
REC = tuple(t((2,), i32) for _ in range(4))
cases("rollout_check", dict(B=4, n=2, S=4, T=2), groups=dict(n=3), size=dict(S=_lib.TG_MAX_S + 1))
cases("rollout_advance", dict(frames=t((4, 2, 4, 4, 4)), tokens=t((4, 12)), n=2, step=0, records=REC, scalars=t((4, 1), f32),
                              nnz=t((4,), i32), overflow=t((4,), u8), actions=t((4, 3, 12)), active=t((4,), u8),
                              stop_solved=True),
      frames_cpu=dict(frames=torch.zeros((4, 2, 4, 4, 4), dtype=i8)),
      active_without_stop=dict(stop_solved=False),
      frames_dtype=dict(frames=t((4, 2, 4, 4, 4), f32)),
      frames_dim=dict(frames=t((4, 4, 4, 4))),
      frames_strided=dict(frames=view(lambda z: z[:, :2], (4, 3, 4, 4, 4))),
      tokens_shape=dict(tokens=t((4, 11))),
      scalars_dim=dict(scalars=t((4,), f32)),
      scalars_dtype=dict(scalars=t((4, 1), f16)),
      actions_dim=dict(actions=t((4, 12))),
      actions_dtype=dict(actions=t((4, 3, 12), u8)),
      groups=dict(n=3),
      step_past_actions=dict(step=3),
      nnz_dtype=dict(nnz=t((4,), i64)),
      overflow_shape=dict(overflow=t((2,), u8)),
      active_dtype=dict(active=t((4,), torch.bool)),
      three_records=dict(records=REC[:3]),
      missing_record=dict(records=(REC[0], None, REC[2], REC[3])),
      hits_shape=dict(records=(REC[0], t((4,), i32), REC[2], REC[3])),
      solved_sample_dtype=dict(records=(REC[0], REC[1], REC[2], t((2,), i64))),
      active_then_frames=dict(stop_solved=False, frames=t((4, 4, 4, 4))),
      tokens_then_scalars=dict(tokens=t((4, 11)), scalars=t((4,), f32)),
      actions_then_groups=dict(actions=t((4, 12)), n=3),
      groups_then_nnz=dict(n=3, nnz=t((4,), i64)),
      nnz_then_records=dict(nnz=t((4,), i64), records=REC[:3]))

# ---- the intended difference ---------------------------------------------------------------------------------------
# change_basis never compared the device of ``out`` with the state's.  With ``out`` on another device the parent went on to
# the next check (the overflow refusal recorded as "old" of the first case) and, with a good overflow, handed a pointer
# from one device to a kernel on another.  Now the out check refuses first, and its message names the device too: the
# other three cases are the parent's refusals of a wrong batch or stride, whose text gains the two words.
OUT_RULE = dict(type="TensorGameError", code=-1,
                message="change_basis failed (-1): out must match state's shape, stride and device")
INTENDED = {
    "change_basis.out_device_then_overflow": dict(out=games(3, device=OTHER), overflow=t((4,), u8)),
    "change_basis.out_batch": dict(out=games(4)),
    "change_basis.out_stride": dict(out=padded(3, 4, 128)),
    "change_basis.out_then_in_place": dict(state=padded(3, 4, 128), out=STATE),
}


def observe(module, fn, base, bad):
    """What the call raises: type, code, message and the innermost line of ``module``'s file in the traceback."""
    try:
        getattr(module, fn)(**{**base, **bad})
    except Exception as e:  # noqa: BLE001 -- whatever it raises is the record
        lines = [f.lineno for f in traceback.extract_tb(e.__traceback__) if f.filename == module.__file__]
        return dict(type=type(e).__name__, code=getattr(e, "code", None), message=str(e), line=lines[-1] if lines else None)
    return dict(type=None, code=None, message="did not raise", line=None)


def same(got, want):
    return all(got[k] == want[k] for k in ("type", "code", "message"))


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def test_the_table_and_the_fixture_hold_the_same_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert sorted(recorded["intended"]) == sorted(INTENDED)


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_is_the_parents(name, recorded):
    want = recorded["cases"][name]
    assert want["type"] == "TensorGameError", "every case of the table is a refusal"
    got = observe(ops, *CASES[name])
    assert same(got, want), (got, want)


@pytest.mark.parametrize("name", list(INTENDED))
def test_intended_difference(name, recorded):
    old = recorded["intended"][name]
    assert old["type"] == "TensorGameError" and not same(old, OUT_RULE)  # the parent refused too, in other words
    assert same(observe(ops, "change_basis", CHANGE_BASIS, INTENDED[name]), OUT_RULE)


def test_coverage_of_the_parents_raise_lines(recorded):
    assert recorded["raise_lines"] == 80
    assert sorted(recorded["uncovered"]) == sorted(UNCOVERED) and len(UNCOVERED) <= MAX_UNCOVERED


def record(path):
    """Write the fixture from the ops.py at ``path`` (the parent's), loaded as a module of the installed package."""
    spec = importlib.util.spec_from_file_location("mat_mul_amd._ops_recorded", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = dict(cases={n: observe(module, *c) for n, c in CASES.items()},
               intended={n: observe(module, "change_basis", CHANGE_BASIS, bad) for n, bad in INTENDED.items()})
    raises = [(n.lineno, n.end_lineno) for n in ast.walk(ast.parse(Path(path).read_text())) if isinstance(n, ast.Raise)
              and isinstance(n.exc, ast.Call) and getattr(n.exc.func, "id", None) == "TensorGameError"]
    hit = {r["line"] for r in (*out["cases"].values(), *out["intended"].values()) if r["type"] == "TensorGameError"}
    out["raise_lines"] = len(raises)
    out["uncovered"] = [a for a, b in sorted(raises) if not any(a <= h <= b for h in hit if h is not None)]
    FIXTURE.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    odd = {n: r for n, r in out["cases"].items() if r["type"] != "TensorGameError"}
    print(f"{len(out['cases'])} cases, {len(raises)} raise lines, uncovered: {out['uncovered']}")
    for n, r in odd.items():
        print("NOT A REFUSAL:", n, r)
    return 0 if not odd and len(out["uncovered"]) <= MAX_UNCOVERED and set(out["uncovered"]) == set(UNCOVERED) else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--record" and sys.argv[2] == "--ops":
        sys.exit(record(sys.argv[3]))
    sys.exit("usage: test_ops_errors_cpu.py --record --ops PARENT_OPS_PY")
