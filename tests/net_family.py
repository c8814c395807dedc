"""The supported family of the fused network (include/tensor_game_net.h, include/tensor_game_train.h) beyond the five
configurations of net_ref and net_s9_ref, and a restatement of the kernels' LDS plans:

* ``FAMILY``: name -> ``Row`` (a configuration in either form of net_ref.dims, whether it is inside the training family,
  and the samples per game k of its sampling tests).  Each row reaches index arithmetic or control flow the five others
  share one value of: decoder rows per workgroup R < 8 and a partial last chunk, k > 8, torso_d != d, torso_heads !=
  heads, ff != 4W, dim_s > 1, W % 4 != 0, n_quantile != 8, n_logits 1 and 8, every dimension 1, every bound, the S = 9
  training torso in one chunk, and the training decoder plan at the LDS limit;
* ``CHUNKED``: three more S = 9 training rows, apart from ``FAMILY``, whose training torso runs a partial last chunk
  (5 + 4 and 2 + 2 + 2 + 2 + 1 sequences) or nine chunks of one, the plan tg_net_train_check compares with 160 KiB;
  ``train_config(name)`` finds a training row's configuration by name in net_ref, net_s9_ref, ``FAMILY`` or ``CHUNKED``;
* the LDS plans in floats, as tg_net.hip (``torso_plan``, ``dec_plan``) and tg_train.hip (``scr_plan``,
  ``scr_plan_kv``, ``tplan``, ``dplan``, ``dplan_kv``) lay them out, and what the host code derives from them:
  ``decoder_rows`` (launch_decode's R), ``torso_chunk`` (the S = 9 training torso's sequences per chunk) and the byte
  counts tg_net_check and tg_net_train_check compare with 160 KiB (``inference_bytes``, ``training_bytes``).
"""
from typing import NamedTuple

from net_ref import CONFIGS, FIELDS, dims
from net_s9_ref import CONFIGS as CONFIGS_S9

LDS = 160 * 1024      # bytes of dynamic LDS per workgroup (gfx950)
MAX_LOGITS = 8        # TG_NET_MAX_LOGITS: the decoder's logits stride
MAX_DIM_S = 4         # TG_NET_MAX_DIM_S: the training torso's scalar slot
WIDE_S = 9            # TG_NET_WIDE_S


class Row(NamedTuple):
    cfg: dict
    train: bool   # inside the training family (tg_net_train_check accepts it)
    k: int        # samples per game of the sampling tests


_R2_9 = dict(S=9, T=1, dim_s=1, c=8, torso_layers=2, torso_heads=2, torso_d=32, torso_ff=32, W=64, heads=8, d=32,
             ff=256, blocks=4, n_steps=27, n_logits=3, n_hidden=64, n_quantile=8)
_A9 = dict(S=9, T=2, dim_s=1, c=8, torso_layers=8, torso_heads=4, torso_d=32, torso_ff=32, W=32, heads=4, d=32,
           ff=128, blocks=2, n_steps=27, n_logits=3, n_hidden=128, n_quantile=8)  # net_ref.dims(net_s9_ref a9)
_LIM = dict(S=5, T=8, dim_s=4, c=32, torso_layers=16, torso_heads=8, torso_d=64, torso_ff=128, W=64, heads=8, d=64,
            ff=256, blocks=4, n_steps=16, n_logits=8, n_hidden=512, n_quantile=16)  # _lib.NET_LIMITS

FAMILY = {
    # reference constructor kwargs
    "e": Row(dict(dim_3d=2, dim_t=8, dim_s=4, dim_c=12, n_steps=6, n_logits=8, n_samples=13, n_feats=6, n_heads=3,
                  n_hidden=40, n_quantile=5, d=16, w=2, n_layers=3), True, 13),
    "g": Row(dict(dim_3d=5, dim_t=8, dim_s=4, dim_c=32, n_steps=12, n_logits=8, n_samples=8, n_feats=8, n_heads=8,
                  n_hidden=512, n_quantile=16, w=4, n_layers=4), True, 8),
    "f": Row(dict(dim_3d=5, dim_t=3, dim_s=2, dim_c=32, n_steps=16, n_logits=2, n_samples=64, n_feats=8, n_heads=8,
                  n_hidden=512, n_quantile=16, d=64, w=4, n_layers=4), False, 64),
    # fused dims (state_dicts the reference cannot build)
    "odd": Row(dict(S=3, T=5, dim_s=3, c=7, torso_layers=2, torso_heads=3, torso_d=5, torso_ff=9, W=15, heads=5, d=3,
                    ff=7, blocks=3, n_steps=7, n_logits=5, n_hidden=33, n_quantile=3), True, 11),
    "ones": Row({k: 1 for k in FIELDS}, True, 1),
    "lim": Row(_LIM, False, 64),
    "w9": Row(dict(_A9, c=4, T=1, torso_heads=1, torso_d=8, torso_ff=16, W=32, heads=2, ff=128, blocks=1,
                   torso_layers=2), True, 4),
    "r2_9": Row(_R2_9, False, 8),
    "r1_9": Row(dict(_R2_9, c=24), False, 8),
}
REFERENCE_ROWS = ("e", "f", "g")  # recorded by tests/golden/make_golden_net_family.py

# S = 9 rows by the training torso's sequences per chunk (c and torso_d set the chunk; the plans depend on neither
# torso_layers nor torso_heads).  c1 sits just inside 160 KiB in both families.
_C9 = dict(S=9, T=4, dim_s=1, torso_layers=2, torso_heads=2, torso_ff=16, W=8, heads=1, d=8, ff=16, blocks=1, n_steps=5,
           n_logits=3, n_hidden=16, n_quantile=8)
CHUNKED = {
    "c5": Row(dict(_C9, c=4, torso_d=16), True, 4),   # chunks of 5, 4
    "c2": Row(dict(_C9, c=24, torso_d=8), True, 4),   # chunks of 2, 2, 2, 2, 1
    "c1": Row(dict(_C9, c=32, torso_d=8), True, 4),   # nine chunks of 1
}
CHUNKS = {"c5": 5, "c2": 2, "c1": 1}                  # torso_chunk of each


def train_config(name):
    """The configuration (either form of net_ref.dims) of the training row ``name``."""
    for table in (CONFIGS, CONFIGS_S9):
        if name in table:
            return table[name]
    row = FAMILY[name] if name in FAMILY else CHUNKED[name]
    assert row.train, name
    return row.cfg


# ---- tg_net.hip ------------------------------------------------------------------------------------------------------
def torso_plan(m):
    """net_torso_kernel's LDS (floats)."""
    S2 = m["S"] ** 2
    T2, cin = 2 * S2, m["S"] * m["T"] + 1
    qkv = max(3 * T2 * m["torso_d"], T2 * m["torso_ff"], 3 * S2 * cin)
    return 3 * S2 * m["c"] + 4 * T2 * m["c"] + qkv + m["S"] * 4 * S2


def dec_plan(m, R):
    """net_decode_kernel's LDS (floats) for R rows per workgroup."""
    J, hd, W = 3 * m["S"] ** 2, m["heads"] * m["d"], m["W"]
    wq, nsc = max(W, m["c"]), max(J, m["n_steps"])
    return (m["blocks"] * J * m["c"] + R * m["blocks"] * m["n_steps"] * W + 3 * R * W + R * hd
            + R * m["heads"] * wq + R * m["heads"] * nsc + R * m["heads"] * wq + R * hd + 2 * R * W + R * m["ff"]
            + R * MAX_LOGITS + R * W + m["n_hidden"] + max(m["n_hidden"], m["n_quantile"]) + 2 * R)


def decoder_rows(m, k):
    """launch_decode's rows per workgroup for k samples per game (the workgroups per game are ceil(k / R))."""
    R = min(k, 8)
    while R > 1 and 4 * dec_plan(m, R) > LDS:
        R -= 1
    return R


def inference_bytes(m):
    """(torso, decoder) bytes tg_net_check compares with 160 KiB (the decoder at R = 1)."""
    return 4 * torso_plan(m), 4 * dec_plan(m, 1)


# ---- tg_train.hip ----------------------------------------------------------------------------------------------------
def scr_plan(nseq, Lx, Ly, c1, c2, H, d, ff):
    """One attention block's scratch (floats), keys and values held."""
    N, M = nseq * Lx, nseq * Ly
    PS = nseq * Lx * Ly
    u = 2 * N * c1 + M * c2 + 3 * N * c1 + M * c2 + 2 * max(N, M)
    heads_end = u + 4 * N * d + 4 * M * d + 2 * PS
    return max(heads_end, u + 2 * N * ff)


def scr_plan_kv(nseq, Lx, Ly, c1, c2, H, d, ff):
    """The same without keys and values (the decoder's cross-attention at S = 9)."""
    N, M = nseq * Lx, nseq * Ly
    PS = nseq * Lx * Ly
    u = 2 * N * c1 + M * c2 + 3 * N * c1 + M * c2 + 2 * max(N, M)
    heads_end = u + 2 * N * d + 4 * N * c2 + 2 * PS
    return max(heads_end, u + 2 * N * ff)


def torso_geo(m, nseq):
    return (nseq, 2 * m["S"], 2 * m["S"], m["c"], m["c"], m["torso_heads"], m["torso_d"], m["torso_ff"])


def self_geo(m):
    return (1, m["n_steps"], m["n_steps"], m["W"], m["W"], m["heads"], m["d"], m["ff"])


def cross_geo(m):
    return (1, m["n_steps"], 3 * m["S"] ** 2, m["W"], m["c"], m["heads"], m["d"], m["ff"])


def tplan(m, nseq=None):
    """The training torso kernels' LDS (floats), with scratch for nseq sequences of a pair (default: all S)."""
    S2 = m["S"] ** 2
    cin = m["S"] * m["T"] + 1
    return (3 * S2 * m["c"] + 3 * S2 * cin + 3 * 2 * S2 * m["c"] + MAX_DIM_S + 3 * S2
            + scr_plan(*torso_geo(m, m["S"] if nseq is None else nseq)))


def _dplan_scr_start(m):
    J, N, W = 3 * m["S"] ** 2, m["n_steps"], m["W"]
    nh, nq = m["n_hidden"], m["n_quantile"]
    return (2 * J * m["c"] + m["blocks"] * 2 * N * W + 5 * N * W + N * m["n_logits"] + 5 * nh + 3 * nq + N + W
            + (m["blocks"] * 2 * N * W + 3) // 4 + 2 * N + 1)


def dplan(m):
    """The training decoder kernel's LDS (floats)."""
    return _dplan_scr_start(m) + max(scr_plan(*self_geo(m)), scr_plan(*cross_geo(m)))


def dplan_kv(m):
    """The same with the cross-attention without keys and values (S = 9)."""
    return _dplan_scr_start(m) + max(scr_plan(*self_geo(m)), scr_plan_kv(*cross_geo(m)))


def torso_chunk(m):
    """Sequences per chunk of the S = 9 training torso: the fewest chunks whose plan fits, evened out (0: none fits)."""
    n = m["S"]
    while n > 0 and 4 * tplan(m, n) > LDS:
        n -= 1
    if n == 0:
        return 0
    chunks = -(-m["S"] // n)
    return -(-m["S"] // chunks)


def training_bytes(m):
    """(torso, decoder) bytes tg_net_train_check compares with 160 KiB."""
    if m["S"] == WIDE_S:
        return 4 * tplan(m, 1), 4 * dplan_kv(m)
    return 4 * tplan(m), 4 * dplan(m)


def fits(nbytes):
    return all(b <= LDS for b in nbytes)


__all__ = ["FAMILY", "CHUNKED", "CHUNKS", "train_config", "REFERENCE_ROWS", "Row", "LDS", "dims", "torso_plan",
           "dec_plan", "decoder_rows", "inference_bytes", "scr_plan", "scr_plan_kv", "tplan", "dplan", "dplan_kv",
           "torso_chunk", "training_bytes", "fits"]
