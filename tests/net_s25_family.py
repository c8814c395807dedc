"""The supported family of the fused network at the 5x5 matmul tensor (S = TG_NET_WIDE3_S = 25; inference) beyond a25,
b25 and c25 of net_s25_ref, which share dim_s = 1, T <= 2, n_steps = 75, n_logits = 3, n_quantile = 8, W % 4 == 0,
c < W, torso_d == d, torso_heads == heads, even dimensions, at most R * heads = 8 team rows per decoder workgroup (one
pass of the team loops), no last chunk below 5 + 1 and a decoder plan far from 160 KiB.

``FAMILY25``: name -> ``Row`` (a configuration in either form of net_ref.dims and the samples per game k of its sampling
tests).  The paths that run at this size only are net_torso_slice_kernel with 25 slices of 50 tokens and the
shared-normalisation decoder net_decode_kernel<true, true>: one normalised copy of ee (J = 1875 rows), each block's
LayerNorm scale folded into the QK rows, and the weighted sum over the keys by 32-lane teams.  Each row reaches index
arithmetic there that the three others share one value of (plans in bytes; the decoder's at R = 1):

* ``e25``  e16 at dim_3d = 25: T = 8 and dim_s = 4 in the slice torso (83 500 bytes, 3*S*cin its qkv term), W = 18
           (W % 4 = 2), n_logits 8, n_quantile 5, n_steps 6 (n_steps % 4 = 2), torso_d 16 != d; k = 13 at R = 2: seven
           workgroups per game, a last chunk of 1;
* ``f25``  f16 at dim_3d = 25, n_steps = 75: T = 3, dim_s = 2, odd c = 5, n_logits 2, n_quantile 16; k = 64 at R = 4:
           16 full workgroups per game;
* ``odd25`` odd16 at S = 25, every dimension odd (c 7, W 15, d 3, ff 7, heads 5 != torso_heads 3, n_steps 7, n_logits 5,
           n_hidden 33, n_quantile 3, three blocks); k = 11 at R = 2: 10 team rows, a second pass of the team loops
           that does not fill the 8 teams;
* ``ones25`` every field 1 (n_steps = 1, n_logits = 1, c = 1: a LayerNorm over one entry, z = 0, only the bias is left);
* ``t8_25`` t8 at S = 25: c = torso_d = 4 with T = 8, heads 8; k = 19 at R = 2: 16 team rows, a last chunk of 1 among 10;
* ``c13_25`` c13 at S = 25: c = 13 > W = 12, the wq = max(W, c) stride of QK (its scaling by the block's ln2 weight too)
           and of YB; n_steps 5 (n_steps % 4 = 1); k = 7;
* ``r8_25`` R = 8, the cap, at k = 20: chunks of 8, 8, 4, 16 team rows, n_steps 8 (n_steps % 4 = 0), four blocks on the
           one shared copy;
* ``lim25`` every bound but T, dim_s, c, torso_layers and blocks: the decoder plan 161 588 bytes; k = 64: 64 workgroups
           per game of one row each;
* ``c20_25`` the widest resident copy, J x c = 150 000 of the decoder plan's 158 180 bytes, and the largest slice plan an
           accepted row has (T = 8, torso_ff 128: 92 300 bytes); c = 20 > W = 8.

``OUTSIDE25``: name -> (the accepted row, the one field changed, its value), the refused partners.  R, the workgroups
per game and the last chunk's size are derived here from net_s25_ref.decoder_rows (tg_net_s25_sample's rule), never
stated; tests/test_net_s25_family_cpu.py asserts what the table reaches.  ``sample_own`` is net_s16_family's.
"""
import numpy as np

from net_ref import FIELDS, dims, make_inputs
from net_s16_family import FAMILY16, Row, sample_own
from net_s25_ref import LDS, dec_plan_shared, decoder_rows, inference_bytes, slice_plan

FAMILY25 = {
    # reference constructor kwargs (n_samples is the reference's own k; the fused network takes k per call)
    "e25": Row(dict(FAMILY16["e16"].cfg, dim_3d=25), 13),
    "f25": Row(dict(FAMILY16["f16"].cfg, dim_3d=25, n_steps=75), 64),
    # fused dims (state_dicts the reference cannot build)
    "odd25": Row(dict(FAMILY16["odd16"].cfg, S=25), 11),
    "ones25": Row(dict({k: 1 for k in FIELDS}, S=25), 1),
    "t8_25": Row(dict(FAMILY16["t8"].cfg, S=25), 19),
    "c13_25": Row(dict(FAMILY16["c13"].cfg, S=25), 7),
    "r8_25": Row(dict(S=25, T=1, dim_s=1, c=4, torso_layers=1, torso_heads=2, torso_d=8, torso_ff=16, W=8, heads=2, d=8,
                      ff=32, blocks=4, n_steps=8, n_logits=3, n_hidden=16, n_quantile=8), 20),
    "lim25": Row(dict(S=25, T=1, dim_s=1, c=9, torso_layers=1, torso_heads=8, torso_d=64, torso_ff=128, W=64, heads=8,
                      d=64, ff=256, blocks=1, n_steps=75, n_logits=8, n_hidden=512, n_quantile=16), 64),
    "c20_25": Row(dict(S=25, T=8, dim_s=4, c=20, torso_layers=1, torso_heads=8, torso_d=64, torso_ff=128, W=8, heads=1,
                       d=8, ff=16, blocks=1, n_steps=3, n_logits=2, n_hidden=8, n_quantile=4), 4),
}
REFERENCE_ROWS = ("e25", "f25")        # recorded by tests/golden/make_golden_net_s25_family.py
SEEDS_NET = {"e25": 71, "f25": 72}     # make_weights' seeds of tests/golden/net_s25_family_cases.npz
OUTSIDE25 = {                          # each one field away from an accepted row
    "lim25_c10": ("lim25", "c", 10),          # the decoder plan at R = 1 passes 160 KiB
    "c20_25_c21": ("c20_25", "c", 21),        # likewise, by the resident copy
    "e25_n76": ("e25", "n_steps", 76),        # TG_NET_WIDE3_MAX_STEPS
}


def outside(name):
    """The fused dims of a refused partner."""
    row, field, value = OUTSIDE25[name]
    return dict(dims(FAMILY25[row].cfg), **{field: value})


def seed(name):
    """make_weights' seed of a row: the fixture's where one was recorded."""
    return SEEDS_NET.get(name, 110 + sorted(FAMILY25).index(name))


def geometry(name, k=None):
    """(R, workgroups per game, samples of the last workgroup, R * heads) of the row's sampling launch (at k samples)."""
    row = FAMILY25[name]
    k = row.k if k is None else k
    m = dims(row.cfg)
    R = decoder_rows(m, k)
    chunks = -(-k // R)
    return R, chunks, k - (chunks - 1) * R, R * m["heads"]


def states(name, B):
    """B input states of a row (int8 frames, float32 scalars) and a g_action int8 (B,n_steps) for teacher forcing."""
    m = dims(FAMILY25[name].cfg)
    xx, ss = make_inputs(m, B, 500 + B)
    ga = np.random.default_rng(600 + B).integers(0, m["n_logits"], size=(B, m["n_steps"])).astype(np.int8)
    return xx, ss, ga


def sample_states(name):
    """States of the sampling tests: 6, or as many as give 2000 draws (B * k * n_steps): net_s16_family.sample_states'
    rule and its reason.  Its cap of 37 states holds only where n_logits = 1 and no boundary exists (ones25, one draw a
    state); c20_25 (k = 4, n_steps = 3) takes 167 states, where 37 would leave 444 draws and one unlucky draw would
    decide the outcome."""
    m = dims(FAMILY25[name].cfg)
    want = max(6, -(-2000 // (FAMILY25[name].k * m["n_steps"])))
    return min(37, want) if m["n_logits"] == 1 else want


def uniforms(name):
    """The given uniforms of the sampling tests, float32 (sample_states, k, n_steps)."""
    m = dims(FAMILY25[name].cfg)
    return np.random.default_rng(5).random((sample_states(name), FAMILY25[name].k, m["n_steps"])).astype(np.float32)


__all__ = ["FAMILY25", "OUTSIDE25", "REFERENCE_ROWS", "SEEDS_NET", "Row", "LDS", "dims", "dec_plan_shared",
           "decoder_rows", "slice_plan", "inference_bytes", "outside", "seed", "geometry", "states", "sample_states",
           "uniforms", "sample_own"]
