"""The network at the 5x5 matmul tensor (S = TG_NET_WIDE3_S = 25, include/tensor_game_net_s25.h; inference only): three
reference configurations for the S = 25 tests and fixtures, on top of net_ref (weights, float64 restatement), which
works at any S, and a restatement of the LDS plans that tg_net_s25_check compares with 160 KiB.

* ``a25``: the training app's configuration (net_ref.CONFIGS["a"]) at dim_3d = 25, n_steps = 75;
* ``b25``: net_s16_ref's b16 (three torso layers and three policy blocks, T = 1, two heads) at the same size;
* ``c25``: a small one without a recorded fixture, whose decoder workgroups hold R = 4 rows at k = 4 (a25 and b25 hold
  one).
"""
from net_family import LDS, MAX_LOGITS
from net_ref import CONFIGS as CONFIGS_S4
from net_s16_ref import CONFIGS as CONFIGS_S16
from net_s16_ref import slice_plan

CONFIGS = {
    "a25": dict(CONFIGS_S4["a"], dim_3d=25, n_steps=75),
    "b25": dict(CONFIGS_S16["b16"], dim_3d=25, n_steps=75),
    "c25": dict(dim_3d=25, dim_t=1, dim_s=1, dim_c=4, n_steps=75, n_logits=3, n_samples=4, n_feats=8, n_heads=2,
                n_hidden=64, n_layers=2),
}
SEEDS_NET = {"a25": 61, "b25": 62, "c25": 63}  # make_weights' seeds (a25, b25: tests/golden/net_s25_cases.npz)
RECORDED = ("a25", "b25")
EE_SLICES = (0, 12, 24)  # the slices i of the torso output the fixture keeps: rows i*75 .. i*75 + 74


def dec_plan_shared(m, R):
    """The shared-normalisation decoder's LDS (floats) for R rows per workgroup: net_family.dec_plan with ONE
    normalised copy of the game's ee (J x c) where that plan holds one per policy block."""
    J, hd, W = 3 * m["S"] ** 2, m["heads"] * m["d"], m["W"]
    wq, nsc = max(W, m["c"]), max(J, m["n_steps"])
    return (J * m["c"] + R * m["blocks"] * m["n_steps"] * W + 3 * R * W + R * hd
            + R * m["heads"] * wq + R * m["heads"] * nsc + R * m["heads"] * wq + R * hd + 2 * R * W + R * m["ff"]
            + R * MAX_LOGITS + R * W + m["n_hidden"] + max(m["n_hidden"], m["n_quantile"]) + 2 * R)


def decoder_rows(m, k):
    """The rows per workgroup tg_net_s25_sample takes for k samples per game (the workgroups per game are ceil(k / R))."""
    R = min(k, 8)
    while R > 1 and 4 * dec_plan_shared(m, R) > LDS:
        R -= 1
    return R


def inference_bytes(m):
    """(torso, decoder) bytes tg_net_s25_check compares with 160 KiB: the slice plan and the decoder at R = 1."""
    return 4 * slice_plan(m), 4 * dec_plan_shared(m, 1)


__all__ = ["CONFIGS", "SEEDS_NET", "RECORDED", "EE_SLICES", "LDS", "slice_plan", "dec_plan_shared", "decoder_rows",
           "inference_bytes"]
