"""The network at the 3x3 matmul tensor (S = TG_NET_WIDE_S = 9, include/tensor_game_net.h): two reference
configurations for the S = 9 tests and fixtures, on top of net_ref and train_ref (weights, float64 restatement,
batches), which work at any S.

* ``A9``: the training app's configuration (net_ref.CONFIGS["a"]) at dim_3d = 9, n_steps = 27;
* ``B9``: a second one with three torso layers and three policy blocks, T = 1, two heads.
"""
from net_ref import CONFIGS as CONFIGS_S4

CONFIGS = {
    "a9": dict(CONFIGS_S4["a"], dim_3d=9, n_steps=27),
    "b9": dict(dim_3d=9, dim_t=1, dim_s=1, dim_c=8, n_steps=27, n_logits=3, n_samples=4, n_feats=16, n_heads=2,
               n_hidden=64, n_layers=3),
}
SEEDS_NET = {"a9": 31, "b9": 32}    # make_weights' seeds of tests/golden/net_s9_cases.npz
SEEDS_TRAIN = {"a9": 41, "b9": 42}  # and of tests/golden/train_s9_cases.npz

__all__ = ["CONFIGS", "SEEDS_NET", "SEEDS_TRAIN"]
