"""CPU checks behind tests/test_gpu_train_s25_paths.py: that its inputs reach the paths of training at the 5x5 tensor
(train_decode_s25_kernel / Game25 in mat_mul_amd/csrc/tg_train_sliced.hip, include/tensor_game_train_s25.h) it is about,
and that they can tell a wrong kernel from a right one.  Everything here is the float64 restatement (train_ref.TrainRef)
and the restated partitions of net_s25_train_family.  No GPU needed.  This file holds the constants the GPU file imports
(rows, batch sizes, seeds, loss weights).

* the run partitions: launch 3's Pt = min(B * 25, 256) runs of (game, slice) units and launch 2's Pd = min(B, 256) runs
  of games at the batch sizes of the GPU cases, every unit and game taken once and in order;
* the bound's floor (TRAIN-S25-FLOOR): under the default weights (1, 1000) the bound 1e-4 * max(1, max |ref|) is absolute
  on most ``torso.*`` tensors; under SCALE[row] times the pair, the smallest power of two that lifts every ``torso.*``
  tensor of the row to max |ref| >= 1 at the batch sizes used, it is relative on all of them;
* two-sided rewards fill the quantile loss's four branches on c25, stail25 and xtail25 (TRAIN-S25-BRANCH);
* the power check (TRAIN-S25-MUTANT prints the ratio): wrong versions of the work-cutting that only S = 25 has
  (``carried_dyn_games``, ``carried_dyn_blocks``, ``self_seam``, ``last_chunk_self``, ``last_chunk_cross``,
  ``ln_tile_tail``) and of the torso's (``drop_unit``, ``li1_drop_unit``) each move some gradient tensor by more than
  ten times its bound on the inputs of the GPU case meant to catch them, and what the inputs of
  tests/test_gpu_train_s25.py miss.
"""
import functools

import numpy as np
import pytest
import torch

from net_ref import P, dims, make_weights
from net_s25_train_family import PARTIALS, ROWS, chunks, decoder_runs, torso_runs
from test_train_s16_paths_cpu import EditsDee, LastChunkLost, lengths, ratio, torso_share
from train_ref import TrainRef, bound, make_batch, two_sided_batch, value_branches

TOL = 1e-4
S = 25
J = 3 * S * S                          # 1875 keys of the cross-attention
LN_TILE = 256                          # kLnTile: keys per tile of ln2's backward into dL/dee
B, SEED_BATCH, SEED_BRANCH = 37, 11, 11
# the decoder-run case's batches, per row the first seed from 11 on with room for float32 under the bound
# (test_eager_float32_leaves_the_decoder_cases_headroom)
SEED_DECODER = {"odd25": 13, "c25": 17}
WEIGHTS_DEFAULT = (1.0, 1000.0)
# make_weights' seeds, those of tests/test_gpu_train_s25.py before t2_25 joined ROWS (t2_25's is new)
SEEDS_NET = {"a25": 250, "c25": 252, "odd25": 253, "stail25": 255, "xtail25": 256, "t2_25": 257}
# per row the smallest power of two times (1, 1000) that lifts every torso.* tensor of the float64 reference to
# max |ref| >= 1 at the batch sizes of B_SCALED[row] (test_the_scaled_weights_are_the_smallest_that_lift_...)
SCALE = {"c25": 2.0 ** 7, "odd25": 2.0 ** 12, "stail25": 2.0 ** 8, "xtail25": 2.0 ** 12}
B_TORSO = (10, 11, 21)                 # the torso-run case: Pt < 256, runs of {1, 2}, runs of {2, 3} that straddle games
B_DECODER = (255, 256, 257, 513)       # the decoder-run case: Pd < Pt, Pd == Pt, runs of two and of three games
B_WORKSPACE = (300, B, 5)
DECODER_CASES = [("odd25", b) for b in B_DECODER] + [("c25", 513)]
B_SCALED = {"c25": (B, 513), "odd25": B_TORSO + B_DECODER, "stail25": (B,), "xtail25": (B,)}
ROWS_PATHS = ("c25", "stail25", "xtail25")  # each loss alone, the branches
ROWS_WORKSPACE = ("c25", "stail25")
B_USED = sorted(set(B_TORSO + B_DECODER + B_WORKSPACE + (2,)))  # every batch size of the GPU file (a25 runs at B = 2)


def weights_scaled(name):
    return WEIGHTS_DEFAULT[0] * SCALE[name], WEIGHTS_DEFAULT[1] * SCALE[name]


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(ROWS[name], SEEDS_NET[name])


def batch_seed(name, b):
    """The seed of the GPU cases' two-sided batch of B = b on row ``name``."""
    return SEED_DECODER[name] if (name, b) in DECODER_CASES else SEED_BATCH


def ref(name, cls=TrainRef, **kw):
    r = cls(weights(name), ROWS[name])
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@functools.lru_cache(maxsize=None)
def true_grads(name, b, seed=None, two_sided=True):
    """The float64 gradient of a batch under the default weights (shared, never modified); seed None: the GPU cases'
    two-sided batch of that size."""
    if seed is None:
        return true_grads(name, b, batch_seed(name, b))
    batch = (two_sided_batch if two_sided else make_batch)(ROWS[name], b, seed)
    return ref(name).loss_grad(*batch)[2]


def scaled(grads, by):
    """The gradient under both weights times ``by``: the loss is linear in the pair (and ``by`` is a power of two)."""
    return {k: g * by for k, g in grads.items()}


# ---- the run partitions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", sorted(set(B_USED) | {1, 5, 37, 300}))
def test_every_unit_and_game_is_taken_once_and_in_order(b):
    for rs, n, count in ((torso_runs(b), b * S, min(b * S, PARTIALS)), (decoder_runs(b), b, min(b, PARTIALS))):
        assert len(rs) == count and rs[0][0] == 0 and rs[-1][1] == n
        assert all(a[1] == z[0] for a, z in zip(rs, rs[1:])) and all(u1 > u0 for u0, u1 in rs)
        assert [u for u0, u1 in rs for u in range(u0, u1)] == list(range(n))


def straddling(rs):
    """The runs of units that hold units of two games."""
    return [(u0, u1) for u0, u1 in rs if u0 // S != (u1 - 1) // S]


def test_the_torso_case_reaches_each_kind_of_run():
    assert len(torso_runs(10)) == 250 < PARTIALS and lengths(torso_runs(10)) == [1]
    rs = torso_runs(11)
    assert len(rs) == 256 and lengths(rs) == [1, 2] and sum(u1 - u0 == 2 for u0, u1 in rs) == 19
    rs = torso_runs(21)
    assert len(rs) == 256 and lengths(rs) == [2, 3] and straddling(rs)
    assert len(straddling(rs)) == 10 and all(u1 == u0 + 2 for u0, u1 in straddling(rs))  # the second unit starts a game
    assert len(torso_runs(5)) == 125 and len(decoder_runs(5)) == 5  # the workspace case's smallest batch


def test_the_decoder_case_reaches_each_kind_of_run():
    assert len(decoder_runs(255)) == 255 < len(torso_runs(255)) == 256  # slab 255 is zeroed whole by launch 3
    for b in (256, 257, 513):
        assert len(decoder_runs(b)) == len(torso_runs(b)) == 256
    assert lengths(decoder_runs(255)) == lengths(decoder_runs(256)) == [1]
    assert lengths(decoder_runs(257)) == [1, 2] and sum(g1 - g0 == 2 for g0, g1 in decoder_runs(257)) == 1
    assert lengths(decoder_runs(513)) == [2, 3] and sum(g1 - g0 == 3 for g0, g1 in decoder_runs(513)) == 1
    assert lengths(decoder_runs(300)) == [1, 2]  # the workspace case's and the bad-token case's batch
    assert lengths(torso_runs(513)) == [50, 51]


def test_the_rows_reach_the_chunks_and_tiles_they_are_there_for():
    table = {name: chunks(dims(ROWS[name])) for name in ("c25", "stail25", "xtail25", "odd25", "t2_25")}
    assert table["c25"] == table["t2_25"] == ((38, 2, 37), (6, 13, 3))  # three games of 2 self and 13 cross chunks
    assert table["stail25"][0] == (16, 2, 15) and table["xtail25"] == ((5, 1, 5), (2, 3, 1))
    assert table["odd25"] == ((5, 1, 5), (5, 1, 5))
    assert divmod(J, LN_TILE) == (7, 83)  # seven full tiles of keys and a last one of 83: keys 1792 .. 1874
    assert all(dims(ROWS[name])["blocks"] == 2 for name in ("c25", "odd25", "xtail25"))
    assert dims(ROWS["t2_25"])["T"] == dims(ROWS["a25"])["T"] == 2


def straddle_unit(b):
    """The first unit of the second game in the first run that straddles two games."""
    u0, u1 = straddling(torso_runs(b))[0]
    u = (u0 // S + 1) * S
    assert u0 < u < u1
    return u


# ---- the bound's floor -----------------------------------------------------------------------------------------------
def admitted(grads, by=1.0):
    """The largest relative error the bound admits on a torso.* tensor: the bound over the tensor's own max |ref|."""
    return max(bound(TOL, g * by) / np.abs(g * by).max() for k, g in grads.items() if k.startswith("torso."))


@pytest.mark.parametrize("name, b", [("odd25", 3), ("odd25", 11), ("xtail25", 3), ("stail25", 3), ("c25", 3), ("c25", 15)])
def test_the_default_weights_leave_the_first_suites_bound_absolute(name, b):
    """The inputs of tests/test_gpu_train_s25.py (make_batch's integer rewards, seed 1, the default weights)."""
    grads = true_grads(name, b, 1, False)
    share, adm = torso_share(grads), admitted(grads)
    print(f"TRAIN-S25-FLOOR {name} B={b} integer rewards weights=(1, 1000) share {share:.2f} admitted {adm:.3g}")
    assert share < 1.0
    assert adm > 1e-2 or name != "odd25", adm


@pytest.mark.parametrize("name", sorted(SCALE))
def test_the_scaled_weights_are_the_smallest_that_lift_every_torso_gradient_above_the_floor(name):
    lowest = np.inf
    for b in B_SCALED[name]:
        grads = true_grads(name, b)
        low = min(float(np.abs(g).max()) for k, g in grads.items() if k.startswith("torso."))
        big = scaled(grads, SCALE[name])
        print(f"TRAIN-S25-FLOOR {name} B={b} weights=(1, 1000) share {torso_share(grads):.2f} admitted "
              f"{admitted(grads):.3g} smallest {low:.3g}; weights=({weights_scaled(name)[0]:g}, "
              f"{weights_scaled(name)[1]:g}) share {torso_share(big):.2f} admitted {admitted(big):.3g}")
        assert torso_share(big) == 1.0 and admitted(big) <= TOL * (1.0 + 1e-12)
        assert torso_share(grads) < 1.0
        lowest = min(lowest, low)
    assert lowest * SCALE[name] >= 1.0 > lowest * SCALE[name] / 2.0  # the smallest power of two


def test_the_gradient_is_linear_in_the_weight_pair():
    """What ``scaled`` rests on: 2^k times both weights is 2^k times every gradient tensor, bit for bit in float64."""
    for name, b in (("odd25", 11), ("c25", 5)):
        batch = two_sided_batch(ROWS[name], b, SEED_BATCH)
        wp, wv = weights_scaled(name)
        got = ref(name).loss_grad(*batch, weight_pol=wp, weight_val=wv)[2]
        want = scaled(true_grads(name, b), SCALE[name])
        assert all(np.array_equal(got[k], want[k]) for k in want)


# ---- float32's own error on the decoder-run batches ------------------------------------------------------------------
@pytest.mark.parametrize("name, b", DECODER_CASES)
def test_eager_float32_leaves_the_decoder_cases_headroom(name, b):
    """How SEED_DECODER was chosen.  Under the scaled weights the bound is 1e-4 of every torso tensor's own maximum, and
    on a batch of hundreds of games that is where float32 itself stands: with batch seed 11 the float32 restatement on
    the CPU misses it at odd25 B = 256 and 257 (1.09 and 1.02 times the bound on torso.li1.1.bias).  There one game's
    term at one element carries the whole error (game 102, element 528 at B = 256: 0.82 of the tensor's maximum, with a
    relative float32 error of 1.3e-4 where every other game's is about 1e-6), the same under every order of the games.
    So the batch seed of these cases is, per row, the first from 11 on at which the float32 restatement stays within
    half the bound on every tensor at every batch size of the row: float32 arithmetic can meet the bound there with a
    factor of two to spare.  odd25: seed 12 gives 0.69 at B = 255, seed 13 at most 0.43.  c25 at B = 513: seeds 11 to
    16 give 0.58, 1.76, 2.20, 0.67, 2.34, 0.64, seed 17 gives 0.42."""
    batch = two_sided_batch(ROWS[name], b, batch_seed(name, b))
    f32 = TrainRef(weights(name), ROWS[name], dtype=torch.float32).loss_grad(*batch)[2]
    r, k = ratio(scaled(true_grads(name, b), SCALE[name]), scaled(f32, SCALE[name]))
    print(f"TRAIN-S25-F32 {name} B={b} seed={batch_seed(name, b)} weights=({weights_scaled(name)[0]:g}, "
          f"{weights_scaled(name)[1]:g}) eager float32 on the CPU at {r:.3g} of the bound, {k}")
    assert r <= 0.5, (r, k)


# ---- the value branches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_PATHS)
def test_two_sided_rewards_fill_the_four_branches_away_from_the_kinks(name):
    shares, margin = value_branches(ref(name), *two_sided_batch(ROWS[name], B, SEED_BRANCH))
    print(f"TRAIN-S25-BRANCH {name} B={B} seed={SEED_BRANCH} {shares} margin {margin:.3g}")
    assert min(shares.values()) >= 0.10, shares
    assert margin >= 1e-4, margin


def test_the_first_suites_rewards_leave_branches_empty():
    for name, b in (("c25", 3), ("odd25", 3), ("odd25", 11)):
        shares, margin = value_branches(ref(name), *make_batch(ROWS[name], b, 1))
        print(f"TRAIN-S25-BRANCH {name} B={b} integer rewards {shares} margin {margin:.3g}")
        assert min(shares.values()) == 0.0, shares


# ---- the power check -------------------------------------------------------------------------------------------------
class DropUnit(EditsDee):
    """``drop_unit``: dL/dee of unit u = g * S + i (the 3S rows of slice i of game g) does not reach the torso."""
    unit = 0

    def edit(self, dee):
        g, i = divmod(self.unit, S)
        dee = dee.clone()
        dee[g, i * 3 * S:(i + 1) * 3 * S] = 0.0
        return dee


class Li1DropsUnit(TrainRef):
    """``li1_drop_unit``: the scalar projections' columns of unit u = g * S + i get no gradient from game g (everything
    else is the true gradient): an error of one unit's share in torso.li1 alone."""
    unit = 0

    def _lin(self, x, p):
        y = super()._lin(x, p)
        if p.startswith("torso.li1.") and y.requires_grad:
            g, i = divmod(self.unit, S)

            def edit(dy):
                dy = dy.clone()
                dy[g, i * S:(i + 1) * S] = 0.0
                return dy
            y.register_hook(edit)
        return y


class EditsDyn(TrainRef):
    """A TrainRef whose cross-attention block ``blk`` passes ``edit(blk, dL/d ln2(ee))`` (B, 3S^2, c) on to ln2's
    backward in place of dL/d ln2(ee): both losses and every gradient before ln2's backward are the true ones."""

    def edit(self, blk, dyn):
        return dyn

    def _ln(self, x, p):
        out = super()._ln(x, p)
        if p.endswith(".att2.ln2") and out.requires_grad:
            out.register_hook(functools.partial(self.edit, int(p.split(".")[-3])))
        return out


class CarriedDynGames(EditsDyn):
    """``carried_dyn_games``: within one decoder run, a game's dL/d ln2(ee) accumulator of a block starts from the
    previous game's of that block instead of zero."""

    def edit(self, blk, dyn):
        dyn = dyn.clone()
        for g0, g1 in decoder_runs(dyn.shape[0]):
            dyn[g0:g1] = dyn[g0:g1].cumsum(0)
        return dyn


class CarriedDynBlocks(EditsDyn):
    """``carried_dyn_blocks``: the accumulator is zeroed once per game, so that a block's starts from what the block
    before it in the backward's order (the next one of the network) left."""

    def edit(self, blk, dyn):
        if blk < self.m["blocks"] - 1:
            assert self.left[0] == blk + 1  # the backward takes the blocks in reverse
            dyn = dyn + self.left[1]
        self.left = (blk, dyn)
        return dyn


class SelfSeam(TrainRef):
    """``self_seam``: a self-attention chunk of rows r0 .. r0 + n - 1 with r0 > 0 gives no gradient to the rows before r0
    through its keys and values (the weight gradients and the chunk's own rows are the true ones)."""

    def _attn(self, p, x, y, H, causal):
        if ".att1." not in p:
            return super()._attn(p, x, y, H, causal)
        nq, count, _ = chunks(self.m)[0]
        assert count > 1 and x is y and causal
        outs = []
        for r0 in range(0, x.shape[1], nq):
            rows = x if r0 == 0 else torch.cat([x[:, :r0].detach(), x[:, r0:]], 1)
            outs.append(super()._attn(p, rows, rows, H, causal)[:, r0:r0 + nq])  # causal: no later row has a weight
        return torch.cat(outs, 1)


class Frozen(TrainRef):
    """``with self.frozen(prefix)``: the weights under ``prefix`` take no gradient from what is computed inside."""
    frozen = LastChunkLost.frozen


class LastChunkLost25(Frozen):
    """``last_chunk_self`` (block ".att1.") and ``last_chunk_cross`` (block ".att2."): the decoder positions of the
    block's last chunk add nothing through the keys and values (to dL/dee, or to the other rows' dL/dx) and nothing to
    the block's weight gradients; what reaches their own rows through the queries and the residual is the true one."""
    block = ".att2."

    def _attn(self, p, x, y, H, causal):
        out = super()._attn(p, x, y, H, causal)
        if self.block not in p:
            return out
        nq, count, last = chunks(self.m)[self.block == ".att2."]
        assert count > 1 and 0 < last < nq
        with self.frozen(p):
            lost = super()._attn(p, x, y.detach(), H, causal)
        return torch.cat([out[:, :x.shape[1] - last], lost[:, x.shape[1] - last:]], 1)


class LnTileTail(Frozen):
    """``ln_tile_tail``: the keys of ln2's last, partial tile (1792 .. 1874) add nothing to dL/dee and nothing to the
    cross-attention's ln2 weight and bias gradients."""

    def _ln(self, x, p):
        if not p.endswith(".att2.ln2"):
            return super()._ln(x, p)
        full = x.shape[1] // LN_TILE * LN_TILE
        assert x.shape[1] == J and full == 1792
        head = super()._ln(x[:, :full], p)
        with self.frozen(p):
            tail = super()._ln(x[:, full:].detach(), p)
        return torch.cat([head, tail], 1)


def told(what, name, true, wrong):
    """The mutant's ratio under the default and under the row's scaled weights (both linear in the pair)."""
    out = []
    for by in (1.0, SCALE[name]):
        r, k = ratio(scaled(true, by), scaled(wrong, by))
        print(f"TRAIN-S25-MUTANT {what} weights=({by:g}, {1000.0 * by:g}) ratio {r:.3g} at {k}")
        out.append(r)
    return out


def mutant(what, name, b, cls, **kw):
    """(ratio under the default weights, ratio under the scaled ones, true gradient, mutant's) on the GPU cases' batch."""
    batch = two_sided_batch(ROWS[name], b, batch_seed(name, b))
    true = true_grads(name, b)
    wrong = ref(name, cls, **kw).loss_grad(*batch)[2]
    return told(f"{what} {name} B={b}", name, true, wrong) + [true, wrong]


def only(true, wrong, changed):
    """Every tensor outside ``changed`` (a predicate on names) is the true one bit for bit, and some tensor differs."""
    assert all(np.array_equal(wrong[k], g) for k, g in true.items() if not changed(k))
    assert any(not np.array_equal(wrong[k], g) for k, g in true.items())


@pytest.mark.parametrize("b", [257, 513])
def test_carried_dyn_games_is_told_by_the_decoder_case(b):
    """At B = 257 one decoder run holds two games, at B = 513 every run holds two or three.  odd25 under the scaled
    weights is the GPU case; the decoder's own gradients are the true ones, the fault shows in torso.* and att2.ln2."""
    default, big, true, wrong = mutant("carried_dyn_games", "odd25", b, CarriedDynGames)
    assert big > 10.0, (default, big)
    only(true, wrong, lambda k: k.startswith("torso.") or ".att2.ln2." in k)


def test_carried_dyn_games_cannot_show_below_257_games():
    """Every decoder run of tests/test_gpu_train_s25.py's float64 comparisons but c25 at B = 257 is one game."""
    for b in (3, 15, 21, 256):
        assert lengths(decoder_runs(b)) == [1]
    _, _, true, wrong = mutant("carried_dyn_games", "odd25", 21, CarriedDynGames)
    assert all(np.array_equal(wrong[k], g) for k, g in true.items())


@pytest.mark.parametrize("name, b", [("odd25", 11), ("c25", B), ("xtail25", B)])
def test_carried_dyn_blocks_is_told_wherever_there_are_two_blocks(name, b):
    default, big, true, wrong = mutant("carried_dyn_blocks", name, b, CarriedDynBlocks)
    assert default > 10.0 and big > 10.0, (default, big)
    only(true, wrong, lambda k: k.startswith("torso.") or ".blocks.0.att2.ln2." in k)


@pytest.mark.parametrize("name", ["c25", "stail25"])
def test_self_seam_is_told_on_the_rows_with_two_self_chunks(name):
    """c25 runs self-attention chunks of 38 + 37 rows, stail25 of 16 + 15; B = 37 is the each-loss-alone and the branch
    case (one batch: the two seeds are equal)."""
    default, big, true, wrong = mutant("self_seam", name, B, SelfSeam)
    assert default > 10.0 and big > 10.0, (default, big)
    for k in (P + "li1.weight", P + "li1.bias"):  # the forward pass is the true one
        np.testing.assert_allclose(wrong[k], true[k], rtol=1e-12, atol=0, err_msg=k)


@pytest.mark.parametrize("what, name, block", [("last_chunk_self", "stail25", ".att1."),
                                               ("last_chunk_cross", "xtail25", ".att2.")])
def test_last_chunk_is_told_per_block_kind(what, name, block):
    default, big, true, wrong = mutant(what, name, B, LastChunkLost25, block=block)
    assert default > 10.0 and big > 10.0, (default, big)
    for k, g in true.items():  # the forward pass is the true one
        assert not (k == P + "li1.weight" or k.startswith("value_head.")) or np.array_equal(wrong[k], g), k


@pytest.mark.parametrize("name, b", [("odd25", 11), ("c25", B), ("xtail25", B)])
def test_ln_tile_tail_is_told(name, b):
    default, big, true, wrong = mutant("ln_tile_tail", name, b, LnTileTail)
    assert big > 10.0 and (default > 10.0 or name == "odd25"), (default, big)
    only(true, wrong, lambda k: k.startswith("torso.") or ".att2.ln2." in k)


@pytest.mark.parametrize("b", [21, 257])
def test_drop_unit_is_told_by_the_run_cases(b):
    """B = 21 is in the torso-run case under both weight pairs, B = 257 in the decoder-run case under the scaled ones."""
    for unit in (straddle_unit(b), b * S - 1):
        default, big, true, wrong = mutant(f"drop_unit unit={unit}", "odd25", b, DropUnit, unit=unit)
        assert big > 10.0 and (b != 21 or default > 10.0), (unit, default, big)
        only(true, wrong, lambda k: k.startswith("torso."))


@pytest.mark.parametrize("b", [21, 257])
def test_one_units_share_of_li1_is_told_by_the_run_cases(b):
    """The smallest fault of the torso's gradient code (the li1 columns of one unit).  The default weights do not reach
    ten times the bound at B = 21 (4.2 and 6.5 times; 28 and 25 times at B = 257); the scaled ones tell it at 461 to
    4000 times, and the torso-run case runs B = 21 under both."""
    for unit in (straddle_unit(b), b * S - 1):
        default, big, true, wrong = mutant(f"li1_drop_unit unit={unit}", "odd25", b, Li1DropsUnit, unit=unit)
        assert big > 10.0, (unit, default, big)
        only(true, wrong, lambda k: k.startswith("torso.li1."))


def test_a_runs_second_unit_cannot_show_at_the_first_suites_small_batches():
    """tests/test_gpu_train_s25.py's rows odd25, one25, xtail25 and stail25 run at B = 3 and a25 at B = 1: every torso
    run there is one unit and none straddles two games, so a fault of a run's second unit (``drop_unit`` at
    straddle_unit) has no unit to act on."""
    for b in (1, 3):
        assert lengths(torso_runs(b)) == [1] and not straddling(torso_runs(b))
    assert straddling(torso_runs(21)) and not straddling(torso_runs(11))  # a25 at B = 11: runs of two, none straddles
