"""The network at the 4x4 matmul tensor (S = TG_NET_WIDE2_S = 16, include/tensor_game_net.h; inference only): two
reference configurations for the S = 16 tests and fixtures, on top of net_ref (weights, float64 restatement), which
works at any S, and a restatement of the LDS plans that tg_net_check compares with 160 KiB at this size.

* ``a16``: the training app's configuration (net_ref.CONFIGS["a"]) at dim_3d = 16, n_steps = 48;
* ``b16``: the shape of net_s9_ref's b9 (three torso layers and three policy blocks, T = 1, two heads) at the same size.
"""
from net_family import LDS, dec_plan
from net_ref import CONFIGS as CONFIGS_S4

CONFIGS = {
    "a16": dict(CONFIGS_S4["a"], dim_3d=16, n_steps=48),
    "b16": dict(dim_3d=16, dim_t=1, dim_s=1, dim_c=8, n_steps=48, n_logits=3, n_samples=4, n_feats=16, n_heads=2,
                n_hidden=64, n_layers=3),
}
SEEDS_NET = {"a16": 51, "b16": 52}  # make_weights' seeds of tests/golden/net_s16_cases.npz


def slice_plan(m):
    """net_torso_slice_kernel's LDS (floats): the 3S rows of one slice of the three grids, four buffers of a pair's 2S
    tokens, the larger of one head's q, k, v / the MLP's hidden rows / the 3S input rows, and one head's scores."""
    S, L, cin = m["S"], 2 * m["S"], m["S"] * m["T"] + 1
    qkv = max(3 * L * m["torso_d"], L * m["torso_ff"], 3 * S * cin)
    return 3 * S * m["c"] + 4 * L * m["c"] + qkv + L * L


def inference_bytes(m):
    """(torso, decoder) bytes tg_net_check compares with 160 KiB at S = 16: the slice plan and the decoder at R = 1."""
    return 4 * slice_plan(m), 4 * dec_plan(m, 1)


__all__ = ["CONFIGS", "SEEDS_NET", "LDS", "slice_plan", "inference_bytes"]
