"""mat_mul_amd -- MI355X-native batched tensor-decomposition environment.

The hot path of kurtosis/mat_mul (AlphaTensor re-implementation) -- the per-game state update
``state <- state - u(x)v(x)w`` with the all-zero terminal check, and the synthetic-demonstration
generator -- as hand-written HIP kernels for gfx950 behind the C ABI of ``include/tensor_game.h``.

There is no CPU fallback: the first use of anything below loads
``mat_mul_amd/lib/libtensorgame.so`` (through ``mat_mul_amd._lib``) and raises ImportError if the
library or one of its entry points is missing.  Only ``mat_mul_amd.build`` (which compiles that
library) and ``mat_mul_amd.sharding`` can be imported without it, which is why attributes are
resolved lazily.
"""
import importlib

__version__ = "0.1.0"
__all__ = ["TensorGameEnv", "SyntheticDemos", "TranspositionTable", "TensorGameError", "functional", "ops", "demo_io",
           "shard_range", "SearchForest", "search", "GameBuffer", "TensorGameData", "replay",
           "FusedAlphaTensor", "FusedAlphaTensor25", "net", "FusedTrainer", "SlicedTrainer", "SlicedTrainer25", "train", "rollout", "sample_rollouts", "RolloutResult",
           "solve_states", "solve_stream", "replay_io", "PackedGames", "save_run", "load_run", "Augment", "augment",
           "SolutionArchive", "solutions", "BasisSet", "solve_in_bases", "bases", "SymmetryGroup", "orbits",
           "FlipWalks", "reduce_archive", "flips", "BilinearMatmul", "RectBilinearMatmul", "FusedBilinearMatmul", "standard_rect", "bilinear",
           "Mod2Walks", "Mod2Result", "reduce_mod2", "reduce_archive_mod2", "flips_mod2",
           "lift_signs", "LiftResult", "reduce_archive_lifted", "lift"]

_SUBMODULES = {"_lib", "ops", "functional", "env", "generator", "sharding", "demo_io", "build", "tree", "search", "replay", "net", "train", "rollout", "replay_io", "augment", "solutions", "bases", "orbits", "flips", "bilinear", "flips_mod2", "lift"}
_ATTRS = {
    "TensorGameEnv": "env",
    "SyntheticDemos": "generator",
    "TranspositionTable": "tree",
    "TensorGameError": "_lib",
    "shard_range": "sharding",
    "SearchForest": "search",
    "GameBuffer": "replay",
    "TensorGameData": "replay",
    "FusedAlphaTensor": "net",
    "FusedAlphaTensor25": "net",
    "FusedTrainer": "train",
    "SlicedTrainer": "train",
    "SlicedTrainer25": "train",
    "sample_rollouts": "rollout",
    "RolloutResult": "rollout",
    "solve_states": "rollout",
    "solve_stream": "rollout",
    "PackedGames": "replay_io",
    "save_run": "replay_io",
    "load_run": "replay_io",
    "Augment": "augment",
    "SolutionArchive": "solutions",
    "BasisSet": "bases",
    "solve_in_bases": "bases",
    "SymmetryGroup": "orbits",
    "FlipWalks": "flips",
    "reduce_archive": "flips",
    "BilinearMatmul": "bilinear",
    "RectBilinearMatmul": "bilinear",
    "FusedBilinearMatmul": "bilinear",
    "standard_rect": "bilinear",
    "Mod2Walks": "flips_mod2",
    "Mod2Result": "flips_mod2",
    "reduce_mod2": "flips_mod2",
    "reduce_archive_mod2": "flips_mod2",
    "lift_signs": "lift",
    "LiftResult": "lift",
    "reduce_archive_lifted": "lift",
}


def __getattr__(name):
    if name in _SUBMODULES:
        return importlib.import_module(f"{__name__}.{name}")
    if name in _ATTRS:
        return getattr(importlib.import_module(f"{__name__}.{_ATTRS[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(set(globals()) | _SUBMODULES | set(_ATTRS))
