"""Training at the 5x5 matmul tensor (S = 25, include/tensor_game_train_s25.h): the LDS plans of tg_train_sliced.hip
at that size restated in floats, what the host code derives from them, the workspace formula, and the rows of the S = 25 training
tests.

* ``slice_tplan``: the torso kernels' plan for one slice (net_s16_train_family's: the kernels are the same);
* ``rows(m)``: the decoder kernel's per-game rows (five n_steps x W buffers, logits, value head, keep mask, tokens);
* ``self_scr(m, nq)``: the self-attention block's scratch for nq query positions against n_steps keys and values;
  ``cross_scr(m, nq)``: the resident ln2(ee) (J x c) and the cross-attention block's scratch for nq query positions
  without keys and values, without the layer-normed keys and their gradient (``scr_plan_kv_ext``);
* ``decoder_chunks(m)``: (Ns, Nx), per block the fewest chunks whose plan fits, evened out (0: not even one position
  fits); ``chunks(m)``: per block (positions per chunk, chunks, positions of the last);
* ``plan_bytes(m)``: the (torso, decoder at Ns = 1, decoder at Nx = 1) byte counts tg_net_train_s25_check compares with
  160 KiB and prints when it refuses; ``decoder_bytes(m)``: launch 2's LDS at the chunks chosen;
* ``workspace_bytes(m, B)``: the header's workspace formula, each part rounded up to 256 bytes;
* ``torso_runs(B)`` and ``decoder_runs(B)``: the runs of (game, slice) units of launch 3's Pt workgroups and the runs of
  games of launch 2's Pd workgroups;
* ``ROWS``: name -> configuration of every accepted row the tests use: a25, b25 and c25 of net_s25_ref (a25 and b25 run
  4 self-attention chunks of 19, 19, 19, 18 positions and 38 cross-attention chunks of 2, 2, .., 1; c25 runs 38 + 37 and
  twelve chunks of 6 with a last of 3), and four small rows derived from c25 that reach the other cases of the two
  chunk loops: ``one25`` (n_steps 1) and ``odd25`` (n_steps 5) take one chunk in both blocks; ``xtail25`` (n_steps 5,
  c 16, whose resident ln2(ee) leaves the cross-attention two positions) takes one chunk in the self-attention and
  chunks of 2, 2 and 1 positions in the cross-attention; ``stail25`` (n_steps 31 with W 64, d 64, ff 256, one block)
  takes chunks of 16 and 15 in the self-attention (and seven of 5, 5, .., 1 in the cross-attention).  ``t2_25`` is c25
  with T = 2 frames (c25's chunks): the small row for float32 frames with T > 1.  ``REFUSED``: a25
  at dim_c 12 (inside the inference family), whose resident ln2(ee) leaves no room for one cross-attention position.
"""
from net_family import LDS, scr_plan
from net_ref import dims
from net_s16_train_family import PARTIALS, n_theta, runs, slice_tplan
from net_s25_ref import CONFIGS

S25 = 25  # TG_NET_WIDE3_S
_C25 = dims(CONFIGS["c25"])

ROWS = {
    "a25": CONFIGS["a25"],
    "b25": CONFIGS["b25"],
    "c25": CONFIGS["c25"],
    "one25": dict(_C25, n_steps=1),
    "odd25": dict(_C25, n_steps=5),
    "xtail25": dict(_C25, c=16, n_steps=5),
    "stail25": dict(_C25, n_steps=31, W=64, d=64, ff=256, blocks=1),
    "t2_25": dict(_C25, T=2),
}
REFUSED = {"wide25": dict(dims(CONFIGS["a25"]), c=12)}


def scr_plan_kv_ext(nseq, Lx, Ly, c1, c2, H, d, ff):
    """scr_plan_kv without the layer-normed keys, their gradient and their statistics (the caller holds them)."""
    N, PS = nseq * Lx, nseq * Lx * Ly
    u = 5 * N * c1 + 2 * N
    return max(u + 2 * N * d + 4 * N * c2 + 2 * PS, u + 2 * N * ff)


def rows(m):
    N, W, nh, nqt = m["n_steps"], m["W"], m["n_hidden"], m["n_quantile"]
    return 5 * N * W + N * m["n_logits"] + 5 * nh + 3 * nqt + N + W + (m["blocks"] * 2 * N * W + 3) // 4 + 2 * N + 1


def self_scr(m, nq):
    return scr_plan(1, nq, m["n_steps"], m["W"], m["W"], m["heads"], m["d"], m["ff"])


def cross_scr(m, nq):
    J = 3 * m["S"] ** 2
    return J * m["c"] + scr_plan_kv_ext(1, nq, J, m["W"], m["c"], m["heads"], m["d"], m["ff"])


def _chunk(m, scr):
    n, room = m["n_steps"], LDS // 4 - rows(m)
    while n > 0 and scr(m, n) > room:
        n -= 1
    if n == 0:
        return 0
    count = -(-m["n_steps"] // n)
    return -(-m["n_steps"] // count)


def decoder_chunks(m):
    """(Ns, Nx): query positions per chunk of the self- and of the cross-attention block."""
    return _chunk(m, self_scr), _chunk(m, cross_scr)


def chunks(m):
    """Per block (self, cross): (positions per chunk, chunks, positions of the last chunk)."""
    out = []
    for nq in decoder_chunks(m):
        count = -(-m["n_steps"] // nq)
        out.append((nq, count, m["n_steps"] - (count - 1) * nq))
    return tuple(out)


def plan_bytes(m):
    return 4 * slice_tplan(m), 4 * (rows(m) + self_scr(m, 1)), 4 * (rows(m) + cross_scr(m, 1))


def decoder_bytes(m):
    ns, nx = decoder_chunks(m)
    return 4 * (rows(m) + max(self_scr(m, ns), cross_scr(m, nx)))


def workspace_bytes(m, B):
    S2 = m["S"] ** 2
    Pd, Pt = min(B, PARTIALS), min(B * m["S"], PARTIALS)
    parts = [B * 3 * S2 * m["c"], B * 3 * S2 * m["c"], B * m["torso_layers"] * 3 * 2 * S2 * m["c"], 2 * B, B,
             Pd * m["blocks"] * 2 * m["n_steps"] * m["W"], Pt * n_theta(m), Pd * 3 * S2 * m["c"]]
    return sum(-(-4 * p // 256) * 256 for p in parts)


def torso_runs(B):
    """(u0, u1) per workgroup of launch 3: the units u = g * 25 + i of Pt = min(B * 25, PARTIALS) workgroups."""
    return runs(B * S25, min(B * S25, PARTIALS))


def decoder_runs(B):
    """(g0, g1) per workgroup of launch 2: the games of Pd = min(B, PARTIALS) workgroups."""
    return runs(B, min(B, PARTIALS))


__all__ = ["ROWS", "REFUSED", "LDS", "PARTIALS", "dims", "slice_tplan", "rows", "self_scr", "cross_scr", "scr_plan_kv_ext",
           "decoder_chunks", "chunks", "plan_bytes", "decoder_bytes", "n_theta", "workspace_bytes", "torso_runs",
           "decoder_runs"]
