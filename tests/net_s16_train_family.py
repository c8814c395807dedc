"""Training at the 4x4 matmul tensor (S = 16, include/tensor_game_train_sliced.h): the LDS plans of tg_train_sliced.hip
at that size restated in floats, what the host code derives from them, the workspace formula, and the rows of the S = 16 training
tests.

* ``slice_tplan``: the torso kernels' plan for one slice (3S grid rows, 3S input rows, three buffers of a pair's 2S
  tokens, the scalar slot, 3S projections, one sequence of attention scratch);
* ``sliced_dplan(m, nq)``: the decoder kernel's plan with the cross-attention on nq positions without keys and values
  (ee, dL/dee and the saved block inputs are in the workspace and take no room);
* ``decoder_chunk``: positions per chunk of the cross-attention, the fewest chunks whose plan fits, evened out;
  ``chunks(m)``: (chunk, number of chunks, positions of the last);
* ``sliced_bytes``: the (torso, decoder) byte counts tg_net_train_sliced_check compares with 160 KiB (the decoder at
  nq = 1) and prints when it refuses;
* ``workspace_bytes(m, B)``: the header's workspace formula, each part rounded up to 256 bytes;
* ``torso_runs(B)`` and ``decoder_runs(B)``: the runs of (game, slice) units of launch 3's Pt workgroups and the runs of
  games of launch 2's Pd workgroups;
* ``ROWS``: name -> configuration of every accepted row the tests use: a16 and b16 of net_s16_ref, ones16, odd16, c13
  and t8 of net_s16_family.FAMILY16 (all four fit), and ``tail16``, added here because none of the others reaches the one
  plan-derived loop, the cross-attention's chunks, with a partial last chunk: a16 and b16 run six chunks of 8, and
  odd16 (n_steps 7), c13 (5), t8 (3) and ones16 (1) fit their positions in one chunk.  tail16 (c 16, W 40, n_steps 11)
  takes chunks of 6 and 5.  The other rows of FAMILY16 are outside the training family or not needed: wide16
  (c 32) is refused, the two J x c buffers alone pass 160 KiB.
"""
from net_family import LDS, MAX_DIM_S, scr_plan, scr_plan_kv, self_geo, torso_geo
from net_ref import dims
from net_s16_family import FAMILY16
from net_s16_ref import CONFIGS

PARTIALS = 256  # TG_NET_TRAIN_PARTIALS

ROWS = {
    "a16": CONFIGS["a16"],
    "b16": CONFIGS["b16"],
    "ones16": FAMILY16["ones16"].cfg,
    "odd16": FAMILY16["odd16"].cfg,
    "c13": FAMILY16["c13"].cfg,
    "t8": FAMILY16["t8"].cfg,
    "tail16": dict(S=16, T=1, dim_s=2, c=16, torso_layers=1, torso_heads=2, torso_d=8, torso_ff=24, W=40, heads=2, d=12,
                   ff=48, blocks=2, n_steps=11, n_logits=4, n_hidden=24, n_quantile=6),
}


def slice_tplan(m):
    S, c, cin = m["S"], m["c"], m["S"] * m["T"] + 1
    return 3 * S * c + 3 * S * cin + 3 * 2 * S * c + MAX_DIM_S + 3 * S + scr_plan(*torso_geo(m, 1))


def cross_geo(m, nq):
    return (1, nq, 3 * m["S"] ** 2, m["W"], m["c"], m["heads"], m["d"], m["ff"])


def sliced_dplan(m, nq):
    N, W, nh, nqt = m["n_steps"], m["W"], m["n_hidden"], m["n_quantile"]
    rows = (5 * N * W + N * m["n_logits"] + 5 * nh + 3 * nqt + N + W + (m["blocks"] * 2 * N * W + 3) // 4 + 2 * N + 1)
    return rows + max(scr_plan(*self_geo(m)), scr_plan_kv(*cross_geo(m, nq)))


def decoder_chunk(m):
    n = m["n_steps"]
    while n > 0 and 4 * sliced_dplan(m, n) > LDS:
        n -= 1
    if n == 0:
        return 0
    count = -(-m["n_steps"] // n)
    return -(-m["n_steps"] // count)


def chunks(m):
    """(positions per chunk, chunks, positions of the last chunk)."""
    nq = decoder_chunk(m)
    count = -(-m["n_steps"] // nq)
    return nq, count, m["n_steps"] - (count - 1) * nq


def sliced_bytes(m):
    return 4 * slice_tplan(m), 4 * sliced_dplan(m, 1)


def n_theta(m):
    def mha(c1, c2, H, d, ff):
        hd = H * d
        return 2 * c1 + 2 * c2 + c1 * hd + hd * c2 + c2 * hd + hd * c1 + c1 + 2 * c1 + c1 * ff + ff + ff * c1 + c1
    S2, cin, W, nh = m["S"] ** 2, m["S"] * m["T"] + 1, m["W"], m["n_hidden"]
    torso = 3 * (m["dim_s"] * S2 + S2) + 3 * (cin * m["c"] + m["c"]) + m["torso_layers"] * mha(
        m["c"], m["c"], m["torso_heads"], m["torso_d"], m["torso_ff"])
    block = 2 * W + mha(W, W, m["heads"], m["d"], m["ff"]) + 2 * W + mha(W, m["c"], m["heads"], m["d"], m["ff"])
    policy = (m["n_logits"] + 1) * W + m["n_steps"] * W + m["blocks"] * block + W * m["n_logits"] + m["n_logits"]
    value = W * nh + nh + 2 * (nh * nh + nh) + nh * m["n_quantile"] + m["n_quantile"]
    return torso + policy + value


def workspace_bytes(m, B):
    S2 = m["S"] ** 2
    Pd, Pt = min(B, PARTIALS), min(B * m["S"], PARTIALS)
    parts = [B * 3 * S2 * m["c"], B * 3 * S2 * m["c"], B * m["torso_layers"] * 3 * 2 * S2 * m["c"], 2 * B, B,
             Pd * m["blocks"] * 2 * m["n_steps"] * m["W"], Pt * n_theta(m)]
    return sum(-(-4 * p // 256) * 256 for p in parts)


def runs(n, P):
    """[n*p/P, n*(p+1)/P) for p < P: the contiguous runs the kernels cut n items into."""
    return [(n * p // P, n * (p + 1) // P) for p in range(P)]


def torso_runs(B, S=16):
    """(u0, u1) per workgroup of launch 3: the units u = g * S + i of Pt = min(B * S, PARTIALS) workgroups."""
    return runs(B * S, min(B * S, PARTIALS))


def decoder_runs(B):
    """(g0, g1) per workgroup of launch 2: the games of Pd = min(B, PARTIALS) workgroups."""
    return runs(B, min(B, PARTIALS))


__all__ = ["ROWS", "LDS", "PARTIALS", "dims", "slice_tplan", "sliced_dplan", "decoder_chunk", "chunks", "sliced_bytes",
           "n_theta", "workspace_bytes", "torso_runs", "decoder_runs"]
