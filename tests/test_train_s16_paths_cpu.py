"""CPU checks behind tests/test_gpu_train_s16_paths.py: that its inputs reach the paths of the sliced training kernels
(mat_mul_amd/csrc/tg_train_sliced.hip) it is about, and that they can tell a wrong kernel from a right one.  Everything
here is the float64 restatement (train_ref.TrainRef) and the restated partitions of net_s16_train_family.  No GPU
needed.  This file holds the constants the GPU file imports (rows, batch sizes, seeds, loss weights).

* the run partitions: launch 3's Pt = min(B * S, 256) runs of (game, slice) units and launch 2's Pd = min(B, 256) runs of
  games at the batch sizes of the GPU cases, every unit and game taken once and in order;
* the bound's floor: under the loss weights (1024, 1 024 000) every ``torso.*`` gradient tensor of row odd16 has
  max |ref| >= 1, so the bound 1e-4 * max(1, max |ref|) is relative there; under (1, 1000) few do (TRAIN-S16-FLOOR);
* two-sided rewards fill the quantile loss's four branches on odd16 and tail16 (TRAIN-S16-BRANCH);
* the power check: wrong versions of the sliced work-cutting (``drop_unit``, ``li1_shift``, ``last_chunk``,
  ``carried_dee``) each move some gradient tensor by more than ten times the bound on the inputs of the GPU case meant
  to catch them (TRAIN-S16-MUTANT prints the ratio), and what the inputs of tests/test_gpu_train_s16.py tell and miss.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from net_ref import P, dims, make_weights
from net_s16_train_family import PARTIALS, ROWS, chunks, decoder_runs, torso_runs
from train_ref import TrainRef, bound, make_batch, two_sided_batch, value_branches

TOL = 1e-4
S = 16
B, SEED_BATCH, SEED_BRANCH = 37, 11, 79
WEIGHTS_DEFAULT = (1.0, 1000.0)
WEIGHTS_SCALED = (1024.0, 1024000.0)  # 2^10 times the default: every torso.* tensor of odd16 at or above the floor
B_TORSO = (15, 16, 17, 31)            # the torso-run case: B * S below, at and just above 256, runs of one and two units
B_DECODER = (255, 256, 257, 513)      # the decoder-run case: Pd < Pt, Pd == Pt, runs of two and of three games
ROWS_PATHS = ("odd16", "tail16")      # each loss alone, the branches, the workspace


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(ROWS[name], 160 + sorted(ROWS).index(name))


def ref(name, cls=TrainRef, **kw):
    r = cls(weights(name), ROWS[name])
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@functools.lru_cache(maxsize=None)
def true_grads(name, b, seed=SEED_BATCH, two_sided=True):
    """The float64 gradient of a batch under the default weights (shared, never modified)."""
    batch = (two_sided_batch if two_sided else make_batch)(ROWS[name], b, seed)
    return ref(name).loss_grad(*batch)[2]


def scaled(grads, by=WEIGHTS_SCALED[0] / WEIGHTS_DEFAULT[0]):
    """The gradient under both weights times ``by``: the loss is linear in the pair (and 1024 is a power of two)."""
    return {k: g * by for k, g in grads.items()}


# ---- the run partitions ----------------------------------------------------------------------------------------------
def lengths(rs):
    return sorted({u1 - u0 for u0, u1 in rs})


@pytest.mark.parametrize("b", sorted(set(B_TORSO + B_DECODER + (1, 5, 19, 37, 273, 300))))
def test_every_unit_and_game_is_taken_once_and_in_order(b):
    for rs, n, count in ((torso_runs(b), b * S, min(b * S, PARTIALS)), (decoder_runs(b), b, min(b, PARTIALS))):
        assert len(rs) == count and rs[0][0] == 0 and rs[-1][1] == n
        assert all(a[1] == z[0] for a, z in zip(rs, rs[1:])) and all(u1 > u0 for u0, u1 in rs)
        assert [u for u0, u1 in rs for u in range(u0, u1)] == list(range(n))


def straddling(rs):
    """The runs of units that hold units of two games."""
    return [(u0, u1) for u0, u1 in rs if u0 // S != (u1 - 1) // S]


def test_the_torso_case_reaches_each_kind_of_run():
    assert len(torso_runs(15)) == 240 and lengths(torso_runs(15)) == [1]
    assert len(torso_runs(16)) == 256 and lengths(torso_runs(16)) == [1]
    rs = torso_runs(17)
    assert len(rs) == 256 and lengths(rs) == [1, 2] and sum(u1 - u0 == 2 for u0, u1 in rs) == 16
    assert straddling(rs) and all(u1 - u0 == 2 for u0, u1 in straddling(rs))
    assert lengths(torso_runs(31)) == [1, 2] and straddling(torso_runs(31))
    assert len(torso_runs(5)) == 80 and len(decoder_runs(5)) == 5  # the workspace case's smallest batch


def test_the_decoder_case_reaches_each_kind_of_run():
    assert len(decoder_runs(255)) == 255 < len(torso_runs(255)) == 256  # slab 255 is zeroed whole by launch 3
    for b in (256, 257, 513):
        assert len(decoder_runs(b)) == len(torso_runs(b)) == 256
    assert lengths(decoder_runs(255)) == lengths(decoder_runs(256)) == [1]
    assert lengths(decoder_runs(257)) == [1, 2]
    assert lengths(decoder_runs(513)) == [2, 3]
    assert lengths(torso_runs(255)) == [15, 16] and lengths(torso_runs(513)) == [32, 33]


def straddle_unit(b):
    """The first unit of the second game in the first run that straddles two games (at B = 17 the second unit of a run of
    two)."""
    u0, u1 = straddling(torso_runs(b))[0]
    u = (u0 // S + 1) * S
    assert u0 < u < u1
    return u


# ---- the bound's floor -----------------------------------------------------------------------------------------------
def torso_share(grads):
    """Share of the torso.* gradient tensors with max |ref| >= 1 (where the bound is relative)."""
    return float(np.mean([np.abs(g).max() >= 1.0 for k, g in grads.items() if k.startswith("torso.")]))


@pytest.mark.parametrize("b", [17, 257])
def test_the_scaled_weights_lift_every_torso_gradient_above_the_floor(b):
    batch = two_sided_batch(ROWS["odd16"], b, SEED_BATCH)
    r = ref("odd16")
    wp, wv = WEIGHTS_SCALED
    share = torso_share(r.loss_grad(*batch, weight_pol=wp, weight_val=wv)[2])
    default = torso_share(true_grads("odd16", b))
    print(f"TRAIN-S16-FLOOR odd16 B={b} weights=({wp:g}, {wv:g}) share {share:.2f} weights=(1, 1000) share {default:.2f}")
    assert share == 1.0, share
    assert default < 0.75, default  # what the default weights leave under the floor


def test_the_gradient_is_linear_in_the_weight_pair():
    """What ``scaled`` rests on: 1024 times both weights is 1024 times every gradient tensor, bit for bit in float64."""
    batch = two_sided_batch(ROWS["odd16"], 17, SEED_BATCH)
    got = ref("odd16").loss_grad(*batch, weight_pol=WEIGHTS_SCALED[0], weight_val=WEIGHTS_SCALED[1])[2]
    want = scaled(true_grads("odd16", 17))
    assert all(np.array_equal(got[k], want[k]) for k in want)


# ---- the value branches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_PATHS)
def test_two_sided_rewards_fill_the_four_branches_away_from_the_kinks(name):
    shares, margin = value_branches(ref(name), *two_sided_batch(ROWS[name], B, SEED_BRANCH))
    print(f"TRAIN-S16-BRANCH {name} {shares} margin {margin:.3g}")
    assert min(shares.values()) >= 0.10, shares
    assert margin >= 1e-4, margin


# ---- the power check -------------------------------------------------------------------------------------------------
class EditsDee(TrainRef):
    """A TrainRef whose torso receives ``edit(dL/dee)`` (B, 3S^2, c) in place of dL/dee: the decoder's gradients and
    both losses are the true ones."""

    def edit(self, dee):
        return dee

    def torso(self, xx, ss):
        ee = super().torso(xx, ss)
        if ee.requires_grad:
            ee.register_hook(self.edit)
        return ee


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


class CarriedDee(EditsDee):
    """``carried_dee``: within one decoder run, a game's dL/dee starts from the previous game's instead of zero."""

    def edit(self, dee):
        dee = dee.clone()
        for g0, g1 in decoder_runs(dee.shape[0]):
            dee[g0:g1] = dee[g0:g1].cumsum(0)
        return dee


class LastChunkLost(TrainRef):
    """``last_chunk``: the decoder positions of the cross-attention's last chunk add nothing to dL/dee and nothing to
    the cross-attention block's weight gradients (their own dL/dx is the true one)."""

    @contextlib.contextmanager
    def frozen(self, prefix):
        kept = {k: v for k, v in self.w.items() if k.startswith(prefix)}
        self.w.update({k: v.detach() for k, v in kept.items()})
        try:
            yield
        finally:
            self.w.update(kept)

    def _attn(self, p, x, y, H, causal):
        out = super()._attn(p, x, y, H, causal)
        if ".att2." not in p:
            return out
        nq, count, last = chunks(self.m)
        assert count > 1
        with self.frozen(p):
            lost = super()._attn(p, x, y.detach(), H, causal)
        return torch.cat([out[:, :x.shape[1] - last], lost[:, x.shape[1] - last:]], 1)


def li1_shift(grads):
    """``li1_shift``: the torso.li1.m weight and bias gradient of slice i lands in slice i + 1's columns (the blob's
    columns tok = i * S + j are the rows of torch's (S^2, dim_s) weight)."""
    out = dict(grads)
    for m in range(3):
        for k in (f"torso.li1.{m}.weight", f"torso.li1.{m}.bias"):
            out[k] = np.roll(grads[k], S, axis=0)
    return out


def ratio(true, wrong):
    """The largest |wrong - true| of a tensor over its bound, and that tensor."""
    r = {k: float(np.abs(wrong[k] - g).max()) / bound(TOL, g) for k, g in true.items()}
    k = max(r, key=r.get)
    return r[k], k


def told(what, true, wrong, least=10.0):
    """The mutant's ratio under the default and under the scaled weights (both linear in the pair)."""
    out = []
    for label, by in (("(1, 1000)", 1.0), ("(1024, 1024000)", WEIGHTS_SCALED[0])):
        r, k = ratio(scaled(true, by), scaled(wrong, by))
        print(f"TRAIN-S16-MUTANT {what} weights={label} ratio {r:.3g} at {k}")
        out.append(r)
    return out


@pytest.mark.parametrize("b", [17, 257])
def test_drop_unit_is_told_by_the_run_cases(b):
    """B = 17 is in the torso-run case under both weight pairs, B = 257 in the decoder-run case under the scaled ones."""
    batch = two_sided_batch(ROWS["odd16"], b, SEED_BATCH)
    true = true_grads("odd16", b)
    for unit in (straddle_unit(b), b * S - 1):
        wrong = ref("odd16", DropUnit, unit=unit).loss_grad(*batch)[2]
        default, big = told(f"drop_unit odd16 B={b} unit={unit}", true, wrong)
        assert big > 10.0 and (b != 17 or default > 10.0), (unit, default, big)
        assert all(np.array_equal(wrong[k], g) for k, g in true.items() if not k.startswith("torso."))


@pytest.mark.parametrize("b", B_TORSO)
def test_li1_shift_is_told_by_the_torso_case(b):
    true = true_grads("odd16", b)
    default, big = told(f"li1_shift odd16 B={b}", true, li1_shift(true))
    assert default > 10.0 and big > 10.0, (default, big)


@pytest.mark.parametrize("b", [17, 257])
def test_one_units_share_of_li1_is_told_by_the_run_cases(b):
    """The smallest fault of the sliced-only gradient code (the li1 columns of one unit): the default weights tell it at
    27 to 54 times the bound, the scaled ones at 472 to 3330 times."""
    batch = two_sided_batch(ROWS["odd16"], b, SEED_BATCH)
    true = true_grads("odd16", b)
    for unit in (straddle_unit(b), b * S - 1):
        wrong = ref("odd16", Li1DropsUnit, unit=unit).loss_grad(*batch)[2]
        default, big = told(f"li1_drop_unit odd16 B={b} unit={unit}", true, wrong)
        assert big > 10.0 * default > 100.0, (default, big)  # told under both; the scaled weights give ten times the margin
        assert all(np.array_equal(wrong[k], g) for k, g in true.items() if not k.startswith("torso.li1."))


def test_last_chunk_is_told_on_tail16():
    """tail16 runs chunks of 6 and 5 positions; B = 37 with both batch seeds is the each-loss-alone and the branch case."""
    assert chunks(dims(ROWS["tail16"])) == (6, 2, 5)
    for seed in (SEED_BATCH, SEED_BRANCH):
        batch = two_sided_batch(ROWS["tail16"], B, seed)
        true = true_grads("tail16", B, seed)
        wrong = ref("tail16", LastChunkLost).loss_grad(*batch)[2]
        default, big = told(f"last_chunk tail16 B={B} seed={seed}", true, wrong)
        assert default > 10.0 and big > 10.0, (default, big)
        for k, g in true.items():  # the forward pass is the true one
            assert not (k == P + "li1.weight" or k.startswith("value_head.")) or np.array_equal(wrong[k], g), k


def test_carried_dee_is_told_by_the_decoder_case():
    """At B = 513 every decoder run holds two or three games; at B = 257 one run holds two."""
    for b in (257, 513):
        batch = two_sided_batch(ROWS["odd16"], b, SEED_BATCH)
        true = true_grads("odd16", b)
        wrong = ref("odd16", CarriedDee).loss_grad(*batch)[2]
        default, big = told(f"carried_dee odd16 B={b}", true, wrong)
        assert big > 10.0, (b, default, big)


def test_what_the_first_suites_inputs_tell_and_miss():
    """The same mutants on the inputs of tests/test_gpu_train_s16.py: make_batch's integer rewards (seed 1), the default
    weights, odd16 and tail16 at B = 5, whose bound is 1e-4 * max(1, max |ref|) too.  Outcome, asserted below:

    * ``last_chunk`` is told on tail16 at B = 5: the policy loss alone moves the cross-attention's weight gradients;
    * ``drop_unit`` (the last unit) and ``li1_shift`` are told on odd16 at B = 5; its 80 runs hold one unit each and
      none straddles two games, so a fault of a run's second unit cannot show there;
    * ``carried_dee`` cannot show below B = 257: every decoder run is one game and the mutant is the true gradient;
    * the relative error the bound admits on a torso.* tensor (bound over the tensor's own max |ref|) reaches more than
      1 % there, a hundred times the 1e-4 it is under the scaled weights."""
    true = true_grads("tail16", 5, 1, False)
    batch = make_batch(ROWS["tail16"], 5, 1)
    assert told("last_chunk tail16 B=5 integer rewards", true, ref("tail16", LastChunkLost).loss_grad(*batch)[2])[0] > 10.0
    true = true_grads("odd16", 5, 1, False)
    batch = make_batch(ROWS["odd16"], 5, 1)
    assert lengths(torso_runs(5)) == [1] and not straddling(torso_runs(5))
    wrong = ref("odd16", DropUnit, unit=5 * S - 1).loss_grad(*batch)[2]
    assert told("drop_unit odd16 B=5 integer rewards", true, wrong)[0] > 10.0
    assert told("li1_shift odd16 B=5 integer rewards", true, li1_shift(true))[0] > 10.0
    wrong = ref("odd16", CarriedDee).loss_grad(*batch)[2]
    assert all(np.array_equal(wrong[k], g) for k, g in true.items())
    admitted = {by: max(bound(TOL, g * by) / np.abs(g * by).max() for k, g in true.items() if k.startswith("torso."))
                for by in (1.0, WEIGHTS_SCALED[0])}
    print(f"TRAIN-S16-FLOOR odd16 B=5 integer rewards: relative error admitted on a torso tensor "
          f"{admitted[1.0]:.3g} under (1, 1000), {admitted[WEIGHTS_SCALED[0]]:.3g} under the scaled weights")
    assert admitted[1.0] > 1e-2 and admitted[WEIGHTS_SCALED[0]] <= TOL * (1.0 + 1e-12)
