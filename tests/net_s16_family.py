"""The supported family of the fused network at the 4x4 matmul tensor (S = TG_NET_WIDE2_S = 16; inference only) beyond
a16 and b16 of net_s16_ref, which share dim_s = 1, T <= 2, c = 8 < W, W % 4 == 0, torso_d == d, torso_heads == heads,
n_logits = 3, n_quantile = 8, n_steps = 48 and two decoder workgroups per game.

``FAMILY16``: name -> ``Row`` (a configuration in either form of net_ref.dims and the samples per game k of its sampling
tests).  The three paths that run at this size only are net_torso_slice_kernel (one workgroup per (game, slice)), the
32-lane team softmax of net_decode_kernel<true> over J = 768 keys, and launch_decode near the 160 KiB LDS limit, where
the rows per workgroup R drop below 8.  Each row reaches index arithmetic there that the others share one value of:

* ``e16``  T = 8 (3*S*cin is the slice plan's largest qkv term), dim_s = 4, W = 18 (W % 4 = 2), n_logits 8, n_quantile 5,
           n_steps 6, torso_d != d; k = 13 at R = 4: four workgroups per game, a last chunk of 1, 12 team-softmax rows;
* ``f16``  T = 3, dim_s = 2, odd c = 5, n_logits 2, n_quantile 16, n_steps 48; k = 64 at R = 8: eight full workgroups;
* ``odd16`` every dimension odd (c = 7, W = 15, d = 3, ff = 7, dim_s = 3, heads 5 != torso_heads 3, n_hidden 33, n_quantile
           3, n_logits 5); k = 11 at R = 5: 25 team-softmax rows, more than the 8 teams and no multiple of 8;
* ``ones16`` every field 1 (n_steps = 1: no second position, n_logits = 1, one key per head);
* ``wide16`` every bound but T, dim_s, torso_layers and blocks, the decoder plan 150 056 bytes at R = 1; k = 64: 64
           workgroups per game of one row each.  ``WIDE16_OUTSIDE`` (blocks = 2) is its refused partner;
* ``t8``   T = 8 with c = torso_d = 4 (the input rows set the slice plan), heads 8 at d = 4; k = 19 at R = 5: a last
           chunk of 4, 40 team-softmax rows;
* ``c13``  c = 13 > W = 12 (the wq = max(W, c) stride of QK and YB), n_steps 5; k = 7 at R = 4: a last chunk of 3.

R, the workgroups per game and the last chunk's size are derived here from net_family.decoder_rows (launch_decode's
rule), never stated; tests/test_net_s16_family_cpu.py asserts what the table reaches.  ``sample_own`` is the restatement
sampling its own tokens position by position, for the count of draws near a cumulative boundary.
"""
from typing import NamedTuple

import numpy as np
import torch

from net_family import LDS, dec_plan, decoder_rows
from net_ref import FIELDS, P, dims, make_inputs, pick
from net_s16_ref import inference_bytes, slice_plan


class Row(NamedTuple):
    cfg: dict
    k: int        # samples per game of the sampling tests


FAMILY16 = {
    # reference constructor kwargs (n_samples is the reference's own k; the fused network takes k per call)
    "e16": Row(dict(dim_3d=16, dim_t=8, dim_s=4, dim_c=12, n_steps=6, n_logits=8, n_samples=13, n_feats=6, n_heads=3,
                    n_hidden=40, n_quantile=5, d=16, w=2, n_layers=3), 13),
    "f16": Row(dict(dim_3d=16, dim_t=3, dim_s=2, dim_c=5, n_steps=48, n_logits=2, n_samples=64, n_feats=8, n_heads=2,
                    n_hidden=24, n_quantile=16, d=8, w=3, n_layers=2), 64),
    # fused dims (state_dicts the reference cannot build)
    "odd16": Row(dict(S=16, T=3, dim_s=3, c=7, torso_layers=2, torso_heads=3, torso_d=5, torso_ff=9, W=15, heads=5, d=3,
                      ff=7, blocks=3, n_steps=7, n_logits=5, n_hidden=33, n_quantile=3), 11),
    "ones16": Row(dict({k: 1 for k in FIELDS}, S=16), 1),
    "wide16": Row(dict(S=16, T=1, dim_s=1, c=32, torso_layers=1, torso_heads=8, torso_d=64, torso_ff=128, W=64, heads=8,
                       d=64, ff=256, blocks=1, n_steps=48, n_logits=8, n_hidden=512, n_quantile=16), 64),
    "t8": Row(dict(S=16, T=8, dim_s=4, c=4, torso_layers=1, torso_heads=1, torso_d=4, torso_ff=8, W=8, heads=8, d=4,
                   ff=16, blocks=1, n_steps=3, n_logits=2, n_hidden=8, n_quantile=4), 19),
    "c13": Row(dict(S=16, T=1, dim_s=1, c=13, torso_layers=1, torso_heads=2, torso_d=8, torso_ff=16, W=12, heads=3, d=8,
                    ff=32, blocks=3, n_steps=5, n_logits=3, n_hidden=16, n_quantile=8), 7),
}
REFERENCE_ROWS = ("e16", "f16")        # recorded by tests/golden/make_golden_net_s16_family.py
SEEDS_NET = {"e16": 66, "f16": 67}     # make_weights' seeds of tests/golden/net_s16_family_cases.npz
WIDE16_OUTSIDE = dict(FAMILY16["wide16"].cfg, blocks=2)  # just outside: the decoder plan at R = 1 passes 160 KiB


def seed(name):
    """make_weights' seed of a row: the fixture's where one was recorded."""
    return SEEDS_NET.get(name, 90 + sorted(FAMILY16).index(name))


def geometry(name):
    """(R, workgroups per game, samples of the last workgroup, R * heads) of the row's sampling launch."""
    row = FAMILY16[name]
    m = dims(row.cfg)
    R = decoder_rows(m, row.k)
    chunks = -(-row.k // R)
    return R, chunks, row.k - (chunks - 1) * R, R * m["heads"]


def states(name, B):
    """B input states of a row (int8 frames, float32 scalars) and a g_action int8 (B,n_steps) for teacher forcing."""
    m = dims(FAMILY16[name].cfg)
    xx, ss = make_inputs(m, B, 500 + B)
    ga = np.random.default_rng(600 + B).integers(0, m["n_logits"], size=(B, m["n_steps"])).astype(np.int8)
    return xx, ss, ga


def sample_states(name):
    """States of the sampling tests: 6, or as many as give 2000 draws (B * k * n_steps), 37 at the most.  The tests cap
    the draws nearer than 1e-5 to a cumulative boundary at a share of all draws (0.1 % for the restatement's own
    tokens); a boundary is that near for about 2e-5 of the draws per boundary, so below a thousand draws one unlucky
    draw would decide the outcome."""
    m = dims(FAMILY16[name].cfg)
    return min(37, max(6, -(-2000 // (FAMILY16[name].k * m["n_steps"]))))


def uniforms(name):
    """The given uniforms of the sampling tests, float32 (sample_states, k, n_steps)."""
    m = dims(FAMILY16[name].cfg)
    return np.random.default_rng(5).random((sample_states(name), FAMILY16[name].k, m["n_steps"])).astype(np.float32)


def sample_own(ref, ee, u):
    """The restatement ``ref`` sampling its own tokens: position t's logits from the tokens it drew before, by the rule
    of net_ref.pick on uniforms u float64 (B,k,n).  Each position runs ref's own attention block on the new row alone
    against the block inputs kept so far (under the causal mask the last row of the rerun prefix is exactly that).
    Returns tokens (B,k,n), the probabilities (B,k,n,n_logits) and the distances to the nearest cumulative boundary."""
    m = ref.m
    B, k, n = u.shape
    w = ref.w
    tok = torch.full((B, k, 1), m["n_logits"], dtype=torch.long, device=ref.device)  # START
    kept = [None] * m["blocks"]
    tokens, probs, dists = [], [], []
    for t in range(n):
        x = w[P + "emb1.weight"][tok] + w[P + "pos_enc"][t] + w[P + "pos_enc_fix"][t]
        for b in range(m["blocks"]):
            p = f"{P}blocks.{b}."
            xb = ref._ln(x, p + "ln1")
            kept[b] = xb if t == 0 else torch.cat([kept[b], xb], 2)
            x = xb + ref._attn(p + "att1.", xb, kept[b], m["heads"], causal=False)
            xb = ref._ln(x, p + "ln2")[:, :, 0]                      # the k samples of a game: k queries on its ee
            x = (xb + ref._attn(p + "att2.", xb, ee, m["heads"], causal=False)).unsqueeze(2)
        pr = torch.softmax(ref._lin(torch.relu(x), P + "li1"), -1)[:, :, 0].cpu().numpy()
        got, dist = pick(u[:, :, t], pr)
        tok = torch.from_numpy(got).long().unsqueeze(-1).to(ref.device)
        tokens.append(got)
        probs.append(pr)
        dists.append(dist)
    return np.stack(tokens, -1), np.stack(probs, 2), np.stack(dists, -1)


__all__ = ["FAMILY16", "REFERENCE_ROWS", "SEEDS_NET", "WIDE16_OUTSIDE", "Row", "LDS", "dims", "dec_plan", "decoder_rows",
           "slice_plan", "inference_bytes", "seed", "geometry", "states", "sample_states", "uniforms", "sample_own"]
