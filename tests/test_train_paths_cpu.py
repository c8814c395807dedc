"""CPU checks behind tests/test_gpu_train_paths.py: that its inputs reach the paths it is about, and that they can
tell a wrong kernel from a right one.  Everything here is the float64 restatement (train_ref.TrainRef) and the library's host
entries.  No GPU needed.

* the ``CHUNKED`` rows of net_family: sequences per chunk, LDS bytes, accepted by both checks;
* the loss weights of the each-loss-alone case lift the gradients above the bound's floor max(1, max |ref|);
* two-sided rewards fill the quantile loss's four branches, away from the kinks;
* ``skip_rows`` of TrainRef.losses;
* the power check: four wrong versions of the loss (``MUTANTS``) each move some gradient tensor by more than ten times
  the bound on the GPU cases' inputs, and what make_batch's integer rewards with the default weights tell and miss.
"""
import functools

import numpy as np
import pytest
import torch

from mat_mul_amd import ops
from mat_mul_amd.net import check_config, infer_config

import net_family as F
from net_ref import dims, make_weights
from train_ref import TrainRef, bad_tokens, bound, make_batch, two_sided_batch, value_branches

TOL = 1e-4
ROWS_WEIGHTS = ("a", "odd", "a9")                   # the each-loss-alone rows of test_gpu_train_paths
ROWS_BRANCH = ("a", "b", "c", "odd", "e")           # its value-branch rows
ROWS_POWER = ("a", "odd")
B, SEED_BATCH = 37, 11
# Seeds chosen for what this file asserts of the inputs, and fixed.  The branch case's batch: 77 and 78 leave a class
# of some row under 10 % (B = 37 rewards are few), 79 is the first seed that fills all four on every row.  The weights:
# under two-sided rewards the (0, 8000) floor share of rows a and a9 is 0.35 - 0.6 for most seeds (the quadratic branch
# has |dl/dq| < 1); 7 and 45 are the first of make_weights' seeds 1, 2, ... at which the row meets both floor shares.
SEED_BRANCH = 79
SEED_WEIGHTS = {"a": 7, "a9": 45}  # every other row: 200


@functools.lru_cache(maxsize=None)
def weights(name):
    return make_weights(F.train_config(name), SEED_WEIGHTS.get(name, 200))


def ref(name, cls=TrainRef):
    return cls(weights(name), F.train_config(name))


# ---- the chunked rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.CHUNKED))
def test_chunked_rows_take_the_partial_chunks_and_fit(name):
    m = dims(F.CHUNKED[name].cfg)
    assert F.torso_chunk(m) == F.CHUNKS[name] == {"c5": 5, "c2": 2, "c1": 1}[name]
    assert (m["S"] % F.CHUNKS[name] != 0) == (name != "c1")  # a partial last chunk; c1: nine chunks of one
    assert 4 * F.tplan(m, F.CHUNKS[name]) <= F.LDS and (name == "c5" or 4 * F.tplan(m, F.CHUNKS[name] + 1) > F.LDS)
    assert F.fits(F.training_bytes(m)) and F.fits(F.inference_bytes(m))
    if name == "c1":  # just inside 160 KiB in both families
        assert F.training_bytes(m)[0] == 153_736 and F.inference_bytes(m)[0] == 161_676 <= F.LDS
    assert infer_config(make_weights(m, 0)) == m
    c = check_config(m)
    ops.net_check(c)
    ops.net_train_check(c)
    for b in (1, 37):
        assert ops.net_train_workspace_size(c, b) % 256 == 0


# ---- the weights and the bound's floor -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_WEIGHTS)
def test_the_loss_weights_lift_the_gradients_above_the_floor(name):
    """Share of the gradient tensors with max |ref| >= 1 (where the bound is relative): at least 0.9 under (16, 0) and
    0.6 under (0, 8000)."""
    batch = two_sided_batch(F.train_config(name), B, SEED_BATCH)
    r = ref(name)
    for (wp, wv), least in (((16.0, 0.0), 0.9), ((0.0, 8000.0), 0.6)):
        grads = r.loss_grad(*batch, weight_pol=wp, weight_val=wv)[2]
        share = np.mean([np.abs(g).max() >= 1.0 for g in grads.values()])
        print(f"TRAIN-PATHS-FLOOR {name} weights=({wp:g}, {wv:g}) share {share:.3f}")
        assert share >= least, (name, wp, wv, share)


# ---- the value branches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS_BRANCH)
def test_two_sided_rewards_fill_the_four_branches_away_from_the_kinks(name):
    shares, margin = value_branches(ref(name), *two_sided_batch(F.train_config(name), B, SEED_BRANCH))
    print(f"TRAIN-PATHS-BRANCH {name} {shares} margin {margin:.3g}")
    assert min(shares.values()) >= 0.10, shares
    assert margin >= 1e-4, margin


def test_integer_rewards_leave_the_branches_nearly_empty():
    """What make_batch's rewards reach, for the record: the quadratic branch and d > 0 each hold under 15 %."""
    for name in ("a", "b", "c"):
        for b in (37, 7):
            shares, _ = value_branches(ref(name), *make_batch(F.train_config(name), b, 1))
            assert shares["quad", "pos"] + shares["quad", "neg"] < 0.15, (name, b, shares)
            assert shares["quad", "pos"] + shares["lin", "pos"] < 0.15, (name, b, shares)


# ---- skip_rows -------------------------------------------------------------------------------------------------------
def test_skip_rows_drop_the_rows_from_the_policy_loss_only():
    cfg = F.train_config("odd")
    xx, ss, aa, rr = two_sided_batch(cfg, 6, 3)
    r = ref("odd")
    rows = [r.losses(xx[i:i + 1], ss[i:i + 1], aa[i:i + 1], rr[i:i + 1])[0].item() for i in range(6)]
    lp, lv = r.losses(xx, ss, aa, rr)
    bad = aa.copy()
    bad[2, 3], bad[4, -1] = dims(cfg)["n_logits"], -5  # an input read as START and a last target
    skip = np.array([False, False, True, False, True, False])
    lps, lvs = r.losses(xx, ss, bad, rr, skip_rows=skip)
    assert abs(lps.item() - (sum(rows) - rows[2] - rows[4])) <= 1e-12 * sum(rows)
    assert lvs.item() == lv.item()  # position 0 sees START alone
    assert abs(r.losses(xx, ss, aa, rr, skip_rows=np.zeros(6, bool))[0].item() - lp.item()) <= 1e-12 * lp.item()
    g = r.loss_grad(xx, ss, bad, rr, skip_rows=np.ones(6, bool))
    assert g[0] == 0.0 and not g[2]["policy_head.predict_action_logits.li1.weight"].any()
    assert g[2]["value_head.mlp.6.bias"].any()


# ---- the power check -------------------------------------------------------------------------------------------------
class FlippedSign(TrainRef):
    """(1) The quantile weight with 1[d <= 0] where the loss has 1[d > 0]."""

    def quantile_loss(self, q, gv):
        n = q.shape[-1]
        tau = (torch.arange(n, dtype=torch.float32, device=self.device) + 0.5) / n
        dd = gv - q
        ad = dd.abs()
        hh = torch.where(ad < 1.0, 0.5 * dd * dd, ad - 0.5)
        return (hh * (tau - (dd <= 0).float()).abs().to(self.dtype)).mean()


class LinearHuber(TrainRef):
    """(2) The linear Huber branch everywhere."""

    def quantile_loss(self, q, gv):
        n = q.shape[-1]
        tau = (torch.arange(n, dtype=torch.float32, device=self.device) + 0.5) / n
        dd = gv - q
        return ((dd.abs() - 0.5) * (tau - (dd > 0).float()).abs().to(self.dtype)).mean()


class CountsBadRows(TrainRef):
    """(3) A row with a bad token still counted in l_pol (its out-of-range targets clipped into range)."""

    def losses(self, xx, ss, g_action, g_value, masks=None, skip_rows=None):
        g = torch.as_tensor(g_action, device=self.device).long()
        gv = torch.as_tensor(g_value, device=self.device).to(self.dtype).reshape(-1, 1)
        oo, q = self.forward(xx, ss, g_action, masks)
        NL = self.m["n_logits"]
        l_pol = torch.nn.functional.cross_entropy(oo.reshape(-1, NL), g.clamp(0, NL - 1).reshape(-1), reduction="sum")
        return l_pol, self.quantile_loss(q, gv)


class IgnoresWeightVal(TrainRef):
    """(4) weight_val ignored: the gradient of weight_pol * l_pol + l_val."""

    def loss_grad(self, *args, weight_val=1000.0, **kw):
        return super().loss_grad(*args, weight_val=1.0, **kw)


MUTANTS = {"sign": FlippedSign, "linear": LinearHuber, "bad_row": CountsBadRows, "weight_val": IgnoresWeightVal}


def detects(name, mutant, batch, **kw):
    """Whether some gradient tensor of the mutant differs from the true float64 one by more than ten times the bound."""
    true = ref(name).loss_grad(*batch, **kw)[2]
    wrong = ref(name, MUTANTS[mutant]).loss_grad(*batch, **kw)[2]
    return any(np.abs(wrong[k] - g).max() > 10.0 * bound(TOL, g) for k, g in true.items())


def bad_batch(name, rewards=two_sided_batch):
    """The bad-token case's inputs (B = 300) and its skipped rows."""
    cfg = F.train_config(name)
    xx, ss, aa, rr = rewards(cfg, 300, SEED_BATCH)
    bad, skip = bad_tokens(aa, dims(cfg)["n_logits"])
    return (xx, ss, bad, rr), skip


@pytest.mark.parametrize("name", ROWS_POWER)
def test_the_gpu_cases_inputs_tell_each_mutant_from_the_loss(name):
    cfg = F.train_config(name)
    branch = two_sided_batch(cfg, B, SEED_BRANCH)
    for mutant in ("sign", "linear"):
        assert detects(name, mutant, branch), mutant
        assert detects(name, mutant, branch, weight_pol=0.0, weight_val=8000.0), mutant
    batch, skip = bad_batch(name)
    assert detects(name, "bad_row", batch, skip_rows=skip)
    alone = two_sided_batch(cfg, B, SEED_BATCH)
    for wp, wv in ((0.0, 8000.0), (0.25, 3.0)):
        assert detects(name, "weight_val", alone, weight_pol=wp, weight_val=wv), (wp, wv)


class HardCodedWeights(TrainRef):
    """The weights (1, 1000) whatever the call passes: what the older tests cannot tell from the loss."""

    def loss_grad(self, *args, weight_pol=1.0, weight_val=1000.0, **kw):
        return super().loss_grad(*args, weight_pol=1.0, weight_val=1000.0, **kw)


class LinearWherePositive(TrainRef):
    """The linear Huber branch wherever g_value - q > 0 (wrong on one of the four classes only)."""

    def quantile_loss(self, q, gv):
        n = q.shape[-1]
        tau = (torch.arange(n, dtype=torch.float32, device=self.device) + 0.5) / n
        dd = gv - q
        ad = dd.abs()
        hh = torch.where((ad < 1.0) & (dd <= 0), 0.5 * dd * dd, ad - 0.5)
        return (hh * (tau - (dd > 0).float()).abs().to(self.dtype)).mean()


MUTANTS.update(hard_coded=HardCodedWeights, linear_pos=LinearWherePositive)


@pytest.mark.parametrize("name", ROWS_POWER)
def test_what_the_integer_rewards_and_default_weights_tell(name):
    """The same check on the older tests' inputs: make_batch's integer rewards in [-12, 0] at B = 37 (seed 1), the
    weights (1, 1000).  Outcome on rows a and odd, asserted below:

    * mutants (1) sign, (2) linear and (4) weight_val are told from the loss there too: the sign flip changes the
      weight of every pair whichever side it lies on, the 5 - 14 % of pairs on the quadratic branch carry a weight of
      1000, and a weight of 1 for 1000 moves every value gradient;
    * mutant (3) bad_row is missed by construction: no older test compares a gradient computed with a bad token;
    * a kernel that ignores its weight arguments for (1, 1000) (``hard_coded``) returns the true gradient exactly, and
      differs under each of the GPU case's three weight pairs;
    * a loss wrong on the class (quadratic, d > 0) alone (``linear_pos``) returns the true gradient exactly on row b at
      B = 7, where no pair has d > 0, and differs on the two-sided inputs."""
    cfg = F.train_config(name)
    batch = make_batch(cfg, B, 1)
    for mutant in ("sign", "linear", "weight_val"):
        assert detects(name, mutant, batch), mutant
    true = ref(name).loss_grad(*batch)[2]
    hard = ref(name, HardCodedWeights).loss_grad(*batch)[2]
    assert all(np.array_equal(true[k], hard[k]) for k in true)
    alone = two_sided_batch(cfg, B, SEED_BATCH)
    for wp, wv in ((16.0, 0.0), (0.0, 8000.0), (0.25, 3.0)):
        assert detects(name, "hard_coded", alone, weight_pol=wp, weight_val=wv), (wp, wv)
    assert detects(name, "linear_pos", two_sided_batch(cfg, B, SEED_BRANCH))


def test_a_one_sided_batch_cannot_see_a_loss_wrong_on_the_other_side():
    name = "b"
    batch = make_batch(F.train_config(name), 7, 1)
    shares, _ = value_branches(ref(name), *batch)
    assert shares["quad", "pos"] + shares["lin", "pos"] == 0.0
    true = ref(name).loss_grad(*batch)
    wrong = ref(name, LinearWherePositive).loss_grad(*batch)
    assert true[1] == wrong[1] and all(np.array_equal(true[2][k], wrong[2][k]) for k in true[2])
    assert detects(name, "linear_pos", two_sided_batch(F.train_config(name), B, SEED_BRANCH))
