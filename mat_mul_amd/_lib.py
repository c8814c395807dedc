"""ctypes binding of include/tensor_game.h.  The product has NO fallback: if the HIP
library is missing or an entry point is absent, importing this module raises."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

# TG_LIB_VARIANT=ab selects the A/B build (libtensorgame_ab.so, -DTG_AB_SWITCHES: the same entry points plus the
# TG_* environment switches that force a kernel variant) -- measurement and A/B tests only.
_VARIANT = os.environ.get("TG_LIB_VARIANT", "")  # "" or "ab"
AB_VARIANT = _VARIANT == "ab"
LIB_PATH = Path(__file__).resolve().parent / "lib" / ("libtensorgame_ab.so" if AB_VARIANT else "libtensorgame.so")

TG_ABI_VERSION = 4
TG_MAX_S = 32
TG_MAX_VALUES = 8
TG_MAX_ACTIONS = 4096


class TensorGameError(RuntimeError):
    """A tg_* entry point returned a negative code; the message is tg_last_error()."""

    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed ({code}): {msg}")
        self.code = code


_p, _i, _i64, _u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64

# name -> argtypes; every symbol include/tensor_game.h declares
SIGNATURES = {
    "tg_abi_version": [],
    "tg_last_error": [],
    "tg_debug_fallbacks": [_p],
    "tg_debug_handovers": [_p],
    "tg_step_i8": [_p, _p, _p, _p, _p, _i64, _i, _i64, _i, _p],
    "tg_step_many_i8": [_p, _p, _p, _p, _p, _i64, _i, _i, _i64, _i, _p],
    "tg_step_stream_i8": [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i64, _i, _p],
    "tg_step_stream_layout": [_i64, _i, _p, _p],
    "tg_step_stream_capacity": [_i, _p],
    "tg_expand_i8": [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _i64, _i64, _i, _p],
    "tg_expand_keyed_i8": [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i64, _i64, _i, _p],
    "tg_copy_i8": [_p, _p, _i64, _i, _i64, _i64, _p],
    "tg_done_i8": [_p, _p, _p, _i64, _i, _i64, _p],
    "tg_step_tracked_i8": [_p, _p, _p, _p, _p, _i64, _i, _i64, _i, _p],
    "tg_reset_matmul_i8": [_p, _i64, _i, _i64, _p],
    "tg_reset_broadcast_i8": [_p, _p, _i64, _i, _i64, _p],
    "tg_gen_from_factors_i8": [_p, _p, _p, _i64, _i, _i, _i64, _i, _p],
    "tg_gen_demos_i8": [_p, _p, _p, _i64, _i, _i, _p, _p, _i, _i, _u64, _u64, _p, _i64, _p],
    "tg_sample_basis_i8": [_p, _p, _p, _i64, _i, _p, _p, _i, _u64, _u64, _p],
    "tg_change_basis_i8": [_p, _p, _p, _p, _i64, _i, _i64, _p],
    "tg_emit_frames": [_p, _p, _p, _i, _i64, _i, _i, _i, C.c_float, _i64, _i64, _p],
    "tg_step_emit": [_p, _p, _p, _p, _p, _p, _i, _i64, _i, _i, _i, C.c_float, _i64, _i64, _i, _p],
    "tg_hash_u64": [_p, _p, _i64, _i, _i64, _p],
    "tg_seen_u64": [_p, _p, _i64, _p, _p, _p, _i64, _i, _p],
    "tg_rank_i32": [_p, _p, _i64, _i, _i64, _p],
}

# name -> argtypes; every symbol include/tensor_game_demos.h declares
DEMO_SIGNATURES = {
    "tg_demo_items": [_p, _p, _i64, _i, _i, _i64, _p, _i64, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p],
}


# name -> argtypes; every symbol include/tensor_game_search.h declares (the forest descriptor goes by pointer)
SEARCH_SIGNATURES = {
    "tg_search_reset": [_p, _p, _i, _p],
    "tg_search_select": [_p, _p, _i, _p, _p],
    "tg_search_commit": [_p, _p, _p, _p, _p, _p],
    "tg_search_advance": [_p, _i, _p],
    "tg_search_policy": [_p, _p, _i, _i, _p],
}

# flags of tg_search_select / tg_search_commit (include/tensor_game_search.h)
TG_SEARCH_EXPAND, TG_SEARCH_TERMINAL, TG_SEARCH_HORIZON, TG_SEARCH_RETRY, TG_SEARCH_PENDING = 1, 2, 4, 8, 128
TG_SEARCH_MAX_K, TG_SEARCH_MAX_T, TG_SEARCH_MAX_DEPTH, TG_SEARCH_MAX_ACTIONS = 64, 16, 4096, 4096


class SearchForestDesc(C.Structure):
    """``tg_search_forest`` of include/tensor_game_search.h (sizes, then device pointers)."""

    _fields_ = [("B", C.c_int64), ("S", C.c_int32), ("T", C.c_int32), ("k", C.c_int32), ("M", C.c_int32),
                ("index_capacity", C.c_int64), ("max_actions", C.c_int32), ("horizon", C.c_int32),
                ("max_depth", C.c_int32), ("shift", C.c_int32)] + [(name, C.c_void_p) for name in (
                    "node_key", "node_frames", "node_nchild", "child_tokens", "child_key", "child_n", "child_q",
                    "child_prior", "index_key", "index_node", "node_count", "root_frames", "root_key", "move", "done",
                    "sims_left", "status", "overflow", "leaf_frames", "leaf_key", "path_node", "path_slot", "depth",
                    "flags", "attempt", "traj_frames", "traj_node", "traj_choice")]


# name -> argtypes; every symbol include/tensor_game_replay.h declares (buffer descriptors go by pointer)
REPLAY_SIGNATURES = {
    "tg_replay_add": [_p, _p, _p, _i, _p, _p, _i64, _i, _p, _p],
    "tg_replay_items": [_p, _p, _i64, _i, _i, _i64, _i, _p, _p, _p, _p, _i64, _i, _p, _i64, _i, _i, _p, _p, _p, _p, _p,
                        _p, _p],
}

# limits and row kinds of include/tensor_game_replay.h
TG_REPLAY_MAX_CAPACITY, TG_REPLAY_MAX_ACTIONS, TG_REPLAY_MAX_T, TG_REPLAY_MAX_LOGITS = 65536, 4096, 16, 128
TG_REPLAY_SYNTH, TG_REPLAY_PLAYED, TG_REPLAY_BEST = 0, 1, 2


# name -> argtypes; every symbol include/tensor_game_replay_io.h declares
REPLAY_IO_SIGNATURES = {
    "tg_replay_pack": [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _p],
    "tg_replay_add_packed": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _p],
}
# status bits of include/tensor_game_replay_io.h
TG_REPLAY_IO_BAD_LENGTH, TG_REPLAY_IO_TRUNCATED = 1, 2

# name -> argtypes; every symbol include/tensor_game_replay_lists.h declares
REPLAY_LISTS_SIGNATURES = {
    "tg_replay_add_lists": [_p, _p, _i64, _p, _p, _p, _i64, _i, _i, _i, _p, _p, _p],
}
# status bits and the shift limit of include/tensor_game_replay_lists.h
TG_REPLAY_LISTS_BAD_LENGTH, TG_REPLAY_LISTS_BAD_GROUP, TG_REPLAY_LISTS_BAD_RANGE, TG_REPLAY_LISTS_NOT_ZERO = 1, 4, 8, 16
TG_REPLAY_LISTS_MAX_SHIFT = 64


class ReplayBufferDesc(C.Structure):
    """``tg_replay_buffer`` of include/tensor_game_replay.h (sizes, then device pointers)."""

    _fields_ = [("C", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("S", C.c_int32)] + [
        (name, C.c_void_p) for name in ("frames", "tokens", "rewards", "length", "offset", "ring")]


# name -> argtypes; every symbol include/tensor_game_net.h declares (the configuration goes by pointer)
NET_SIGNATURES = {
    "tg_net_check": [_p],
    "tg_net_weights_size": [_p, _p],
    "tg_net_torso": [_p, _p, _p, _i, _p, _p, _i64, _p],
    "tg_net_sample": [_p, _p, _p, _p, _i64, _i, _u64, _u64, _p, _p, _p, _p, _p],
    "tg_net_torso_masked": [_p, _p, _p, _i, _p, _p, _i64, _p, _i, _p],
    "tg_net_sample_masked": [_p, _p, _p, _p, _i64, _i, _u64, _u64, _p, _p, _p, _p, _p, _i, _p],
    "tg_net_logits": [_p, _p, _p, _p, _i64, _p, _p, _p, _p],
}

# name -> argtypes; every symbol include/tensor_game_net_s25.h declares (the same at S = TG_NET_WIDE3_S; torso and sample
# are the masked forms)
NET_S25_SIGNATURES = {
    "tg_net_s25_check": NET_SIGNATURES["tg_net_check"],
    "tg_net_s25_weights_size": NET_SIGNATURES["tg_net_weights_size"],
    "tg_net_s25_torso": NET_SIGNATURES["tg_net_torso_masked"],
    "tg_net_s25_sample": NET_SIGNATURES["tg_net_sample_masked"],
    "tg_net_s25_logits": NET_SIGNATURES["tg_net_logits"],
}

# name -> argtypes; every symbol include/tensor_game_train.h declares
TRAIN_SIGNATURES = {
    "tg_net_train_check": [_p],
    "tg_net_train_workspace_size": [_p, _i64, _p],
    "tg_net_loss_grad": [_p, _p, _p, _p, _i, _p, _p, _p, _i64, C.c_float, C.c_float, C.c_float, _u64, _u64, _p, _p, _p,
                         _i64, _p, _p, _p, _p],
}
# name -> argtypes; every symbol include/tensor_game_train_sliced.h declares (the same three at S = TG_NET_WIDE2_S)
TRAIN_SLICED_SIGNATURES = {
    "tg_net_train_sliced_check": TRAIN_SIGNATURES["tg_net_train_check"],
    "tg_net_train_sliced_workspace_size": TRAIN_SIGNATURES["tg_net_train_workspace_size"],
    "tg_net_loss_grad_sliced": TRAIN_SIGNATURES["tg_net_loss_grad"],
}
# name -> argtypes; every symbol include/tensor_game_train_s25.h declares (the same three at S = TG_NET_WIDE3_S)
TRAIN_S25_SIGNATURES = {
    "tg_net_train_s25_check": TRAIN_SIGNATURES["tg_net_train_check"],
    "tg_net_train_s25_workspace_size": TRAIN_SIGNATURES["tg_net_train_workspace_size"],
    "tg_net_loss_grad_s25": TRAIN_SIGNATURES["tg_net_loss_grad"],
}
# name -> argtypes; every symbol include/tensor_game_rollout.h declares
ROLLOUT_SIGNATURES = {
    "tg_rollout_advance": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _p],
    "tg_rollout_check": [_i64, _i, _i, _i, _i, _i, _i, _i],
}
# name -> argtypes; every symbol include/tensor_game_rollout_masked.h declares
ROLLOUT_MASKED_SIGNATURES = {
    "tg_rollout_advance_masked": ROLLOUT_SIGNATURES["tg_rollout_advance"][:10] + [_p] +
                                 ROLLOUT_SIGNATURES["tg_rollout_advance"][10:],
}
# name -> argtypes; every symbol include/tensor_game_rollout_slots.h declares
ROLLOUT_SLOTS_SIGNATURES = {
    # the masked entry with (slot_state, slot_step) behind `active` and without the host `step`
    "tg_rollout_advance_slots": [_p] * 13 + [_i64, _i, _i, _i, _i, _i, _i, _p],
    "tg_rollout_refill": [_p, _p, _i64, _p, _i64, _u64, _i] + [_p] * 21 + [_i64, _i, _i, _i, _i, _i, _p],
}
# name -> argtypes; every symbol include/tensor_game_symmetry.h declares
SYMMETRY_SIGNATURES = {
    "tg_symmetry_apply": [_p, _p, _p, _i64, _i, _i, _i, _i, _p, _p, _p, _p, _p],
    "tg_symmetry_sample": [_p, _i64, _i, _u64, _u64, _i, _p],
}
# name -> argtypes; every symbol include/tensor_game_solutions.h declares
SOLUTION_SIGNATURES = {
    "tg_solution_check": [_i64, _i, _i, _i],
    "tg_solution_canon": [_p, _p, _p, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _p],
}
# limits and status bits of include/tensor_game_solutions.h
TG_SOL_MAX_K, TG_SOL_MAX_SHIFT, TG_SOL_BAD_LENGTH, TG_SOL_BAD_NEGATION = 256, 64, 1, 2
# name -> argtypes; every symbol include/tensor_game_bases.h declares
BASES_SIGNATURES = {
    "tg_basis_inverse_check": [_i64, _i],
    "tg_solution_rebase_check": [_i64, _i, _i, _i64, _i],
    "tg_basis_inverse_i32": [_p, _p, _i64, _i, _p, _p, _p, _p],
    "tg_solution_rebase": [_p, _p, _p, _p, _i64, _i, _i, _i64, _i, _p, _p, _p, _p, _p],
}
# status bits of include/tensor_game_bases.h (the limits are TG_MAX_S, TG_SOL_MAX_K and TG_SOL_MAX_SHIFT)
TG_BASIS_BAD_DIAGONAL, TG_BASIS_BAD_RANGE = 1, 2
TG_REBASE_BAD_LENGTH, TG_REBASE_BAD_INDEX, TG_REBASE_BAD_RANGE = 1, 2, 4
# name -> argtypes; every symbol include/tensor_game_orbits.h declares
ORBIT_SIGNATURES = {
    "tg_orbit_check": [_i64, _i, _i, _i, _i],
    "tg_orbit_workspace_size": [_i64, _i, _i, _i, _p],
    "tg_orbit_fixes": [_p, _i64, _i, _p, _i, _p, _p, _p],
    "tg_orbit_canon": [_p, _p, _p, _i64, _i, _i, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p],
}
# limits and status bits of include/tensor_game_orbits.h
TG_ORBIT_MAX_G, TG_ORBIT_MAX_ROW = 2048, 24576
TG_ORBIT_BAD_LENGTH, TG_ORBIT_BAD_NEGATION, TG_ORBIT_BAD_GROUP = 1, 2, 4
# name -> argtypes; every symbol include/tensor_game_flips.h declares
FLIP_SIGNATURES = {
    "tg_flip_check": [_i64, _i64, _i, _i, _i, _i, _i64, _i64],
    "tg_flip_begin": [_p, _p, _i64, _p, _i64, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "tg_flip_advance": [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _u64, _u64, _i64, _i64, _p],
}
# name -> argtypes; every symbol include/tensor_game_flips_plus.h declares
FLIP_PLUS_SIGNATURES = {
    "tg_flip_plus_check": [_i64, _i, _i, _i, _i, _i64, _i64, _i64, _i64],
    "tg_flip_advance_plus": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _u64, _u64, _i64, _i64, _i64, _i64, _p],
}
TG_FLIP_MAX_PLUS_AFTER = 2 ** 31 - 1
# name -> argtypes; every symbol include/tensor_game_flips_mod2.h declares
FLIP2_SIGNATURES = {
    "tg_flip2_check": [_i64, _i64, _i, _i, _i, _i64, _i64, _i64, _i64],
    "tg_flip2_begin": [_p, _p, _i64, _p, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "tg_flip2_advance": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _u64, _u64, _i64, _i64, _i64, _i64, _p],
    "tg_flip2_residual": [_p, _p, _p, _i64, _i, _i, _p, _p],
}
TG_FLIP2_DOMAIN, TG_FLIP2_MAX_PLUS_AFTER = 0x46320000, 2 ** 31 - 1
# name -> argtypes; every symbol include/tensor_game_lift.h declares (tg_lift2_workspace_bytes returns an int64)
LIFT2_SIGNATURES = {
    "tg_lift2_workspace_bytes": [_i, _i],
    "tg_lift2_check": [_i64, _i, _i, _i, _i64, _i64],
    "tg_lift2_signs": [_p, _p, _p, _i64, _i, _i, _i, _u64, _u64, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, _p],
}
# limits and status values of include/tensor_game_lift.h
TG_LIFT2_DOMAIN, TG_LIFT2_MAX_TRIES, TG_LIFT2_MAX_WS_LISTS = 0x4C320000, 1024, 65536
TG_LIFT2_OK, TG_LIFT2_NOT_MOD2, TG_LIFT2_INCONSISTENT, TG_LIFT2_NOT_EXACT = 0, 1, 2, 3
# name -> argtypes; every symbol include/tensor_game_bilinear.h declares
BILINEAR_SIGNATURES = {
    "tg_bilinear_check": [_i64, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i],
    "tg_bilinear_encode_f32": [_p, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _i, _i, _p, _p],
    "tg_bilinear_decode_f32": [_p, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _i, _p, _p],
}
BILINEAR_SIGNATURES["tg_bilinear_encode_f64"] = BILINEAR_SIGNATURES["tg_bilinear_encode_f32"]
BILINEAR_SIGNATURES["tg_bilinear_decode_f64"] = BILINEAR_SIGNATURES["tg_bilinear_decode_f32"]
# limits of include/tensor_game_bilinear.h (R and shift are held to TG_SOL_MAX_K and TG_SOL_MAX_SHIFT)
TG_BILINEAR_MIN_N, TG_BILINEAR_MAX_N = 2, 5
# name -> argtypes; every symbol include/tensor_game_rect.h declares (its limits are TG_MAX_S, TG_SOL_MAX_K, TG_SOL_MAX_SHIFT)
RECT_SIGNATURES = {
    "tg_reset_matmul_rect_i8": [_p, _i64, _i, _i, _i, _i, _i64, _p],
    "tg_bilinear_rect_check": [_i64, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i, _i, _i],
    "tg_bilinear_rect_encode_f32": [_p, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _i, _i, _i, _i, _p, _p],
    "tg_bilinear_rect_decode_f32": [_p, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _i, _i, _i, _p, _p],
}
RECT_SIGNATURES["tg_bilinear_rect_encode_f64"] = RECT_SIGNATURES["tg_bilinear_rect_encode_f32"]
RECT_SIGNATURES["tg_bilinear_rect_decode_f64"] = RECT_SIGNATURES["tg_bilinear_rect_decode_f32"]
# name -> argtypes; every symbol include/tensor_game_products.h declares (limits: TG_MAX_S, TG_SOL_MAX_K, TG_SOL_MAX_SHIFT)
PRODUCTS_SIGNATURES = {
    "tg_bilinear_products_check": [_i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i, _i],
    "tg_bilinear_products_bf16": [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _i, _i, _i, _i, _p, _p],
}
PRODUCTS_SIGNATURES["tg_bilinear_products_f16"] = PRODUCTS_SIGNATURES["tg_bilinear_products_bf16"]
# limits and status bits of include/tensor_game_flips.h
TG_FLIP_MAX_K, TG_FLIP_MAX_BOUND, TG_FLIP_MAX_STEPS = 128, 63, 65536
TG_FLIP_BAD_LENGTH, TG_FLIP_BAD_RANGE, TG_FLIP_BAD_SRC = 1, 2, 4
# flags of tg_symmetry_sample (include/tensor_game_symmetry.h)
TG_SYM_MODES, TG_SYM_PERMS, TG_SYM_SIGNS = 1, 2, 4
TG_ROLLOUT_MAX_SLOTS = 65536
TG_NET_TRAIN_PARTIALS = 256
TG_TRAIN_STATUS_BAD_TOKEN = 1

# the supported family of include/tensor_game_net.h
NET_LIMITS = {"S": 5, "T": 8, "dim_s": 4, "c": 32, "torso_layers": 16, "torso_heads": 8, "torso_d": 64, "torso_ff": 128,
              "W": 64, "heads": 8, "d": 64, "ff": 256, "blocks": 4, "n_steps": 16, "n_logits": 8, "n_hidden": 512,
              "n_quantile": 16}
TG_NET_MAX_SAMPLES = 64
# the first state size outside NET_LIMITS["S"]: the 3x3 matmul tensor, with its own n_steps bound
TG_NET_WIDE_S, TG_NET_WIDE_MAX_STEPS = 9, 27
# and the second: the 4x4 matmul tensor (the torso runs by slices there; training through tensor_game_train_sliced.h)
TG_NET_WIDE2_S, TG_NET_WIDE2_MAX_STEPS = 16, 48
# the 5x5 matmul tensor has entries of its own (include/tensor_game_net_s25.h, training through
# tensor_game_train_s25.h); tg_net_check refuses the size
TG_NET_WIDE3_S, TG_NET_WIDE3_MAX_STEPS = 25, 75


class NetConfig(C.Structure):
    """``tg_net_config`` of include/tensor_game_net.h."""

    _fields_ = [(name, C.c_int32) for name in ("S", "T", "dim_s", "c", "torso_layers", "torso_heads", "torso_d",
                                                "torso_ff", "W", "heads", "d", "ff", "blocks", "n_steps", "n_logits",
                                                "n_hidden", "n_quantile")]


def _preload_torch_hip_runtime() -> None:
    """PyTorch-ROCm ships its own libamdhip64 (SONAME libamdhip64.so.7).  Two HIP runtimes in
    one process do not share devices or streams (the second one reports "no ROCm-capable
    device"), so torch's copy must be the one libtensorgame.so binds to: load it first; the
    dynamic linker then satisfies our NEEDED libamdhip64.so.7 by SONAME."""
    import torch  # noqa: F401  (maps torch/lib/libamdhip64.so)

    cand = Path(torch.__file__).resolve().parent / "lib" / "libamdhip64.so"
    if cand.exists():
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)


def _hip_runtimes_mapped():
    with open("/proc/self/maps") as f:
        return sorted({line.split()[-1] for line in f if "libamdhip64" in line})


def _load() -> C.CDLL:
    _preload_torch_hip_runtime()
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library is not built.  Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `python -m mat_mul_amd.build [--ab]`). "
            "mat_mul_amd has no CPU fallback."
        )
    lib = C.CDLL(str(LIB_PATH))
    for name, argtypes in {**SIGNATURES, **DEMO_SIGNATURES, **SEARCH_SIGNATURES, **REPLAY_SIGNATURES,
                           **REPLAY_IO_SIGNATURES, **REPLAY_LISTS_SIGNATURES,
                           **NET_SIGNATURES, **NET_S25_SIGNATURES, **TRAIN_SIGNATURES, **TRAIN_SLICED_SIGNATURES,
                           **TRAIN_S25_SIGNATURES,
                           **ROLLOUT_SIGNATURES, **ROLLOUT_MASKED_SIGNATURES, **ROLLOUT_SLOTS_SIGNATURES,
                           **SYMMETRY_SIGNATURES, **SOLUTION_SIGNATURES, **BASES_SIGNATURES,
                           **ORBIT_SIGNATURES, **FLIP_SIGNATURES, **FLIP_PLUS_SIGNATURES, **FLIP2_SIGNATURES,
                           **LIFT2_SIGNATURES, **BILINEAR_SIGNATURES, **RECT_SIGNATURES, **PRODUCTS_SIGNATURES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.argtypes = argtypes
        fn.restype = C.c_char_p if name == "tg_last_error" else C.c_int64 if name == "tg_lift2_workspace_bytes" else C.c_int
    rts = _hip_runtimes_mapped()
    if len(rts) > 1:
        raise ImportError(f"two HIP runtimes are mapped ({rts}); libtensorgame.so must share PyTorch's")
    if lib.tg_abi_version() != TG_ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.tg_abi_version()} != {TG_ABI_VERSION}; rebuild it")
    return lib


lib = _load()


def call(name: str, *args) -> None:
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise TensorGameError(name, rc, lib.tg_last_error().decode("utf-8", "replace"))
