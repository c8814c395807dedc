"""CPU checks of the solution search that stops solved groups: the host checks of tg_rollout_advance_masked through
ctypes, the relation between the plain and the masked restatement (tests/rollout_masked_ref.py) on the recorded
factorisations, and the argument errors of sample_rollouts / solve_states."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib

import rollout_masked_ref as M
import rollout_ref as R
from rollout_ref import demo_cases, strassen_scripts

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "tensor_game_rollout_masked.h"


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_masked_entry_is_declared_bound_and_exported():
    syms = re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HEADER.read_text(), flags=re.M)
    assert syms == ["tg_rollout_advance_masked"] == sorted(_lib.ROLLOUT_MASKED_SIGNATURES)
    # tensor_game_rollout.h brings the declaration with it
    assert '#include "tensor_game_rollout_masked.h"' in (ROOT / "include" / "tensor_game_rollout.h").read_text()
    plain = _lib.ROLLOUT_SIGNATURES["tg_rollout_advance"]
    assert _lib.ROLLOUT_MASKED_SIGNATURES["tg_rollout_advance_masked"] == plain[:10] + [C.c_void_p] + plain[10:]
    from mat_mul_amd import build
    assert HEADER in build.HEADERS
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        assert hasattr(C.CDLL(str(path)), "tg_rollout_advance_masked"), path
    assert _lib.lib.tg_abi_version() == _lib.TG_ABI_VERSION == 4   # additive: the version stays


def test_masked_entry_host_checks_in_order():
    lib = _lib.lib
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch

    def adv(frames=p, tokens=p, scalars=p, nnz=p, overflow=p, best=p, hits=p, sstep=p, ssample=p, actions=p, active=p,
            B=8, n=4, S=4, T=2, dim_s=1, step=0, max_actions=4, shift=1):
        return lib.tg_rollout_advance_masked(frames, tokens, scalars, nnz, overflow, best, hits, sstep, ssample, actions,
                                             active, B, n, S, T, dim_s, step, max_actions, shift, None)

    # every bad argument alone: the message names it and the entry
    for bad, word in ((dict(S=0), b"S=0"), (dict(S=33), b"S=33"), (dict(T=0), b"T=0"), (dict(T=9), b"TG_NET_MAX_T"),
                      (dict(n=0), b"n=0"), (dict(n=65), b"TG_NET_MAX_SAMPLES"), (dict(B=9), b"multiple of n"),
                      (dict(B=-4), b"B=-4"), (dict(dim_s=-1), b"dim_s"), (dict(dim_s=65), b"dim_s"),
                      (dict(step=-1), b"step=-1"), (dict(step=4), b"max_actions"), (dict(max_actions=0), b"max_actions"),
                      (dict(frames=None), b"null frames"), (dict(tokens=None), b"null tokens"),
                      (dict(nnz=None), b"null nnz"), (dict(best=None), b"group record"),
                      (dict(hits=None), b"group record"), (dict(sstep=None), b"group record"),
                      (dict(ssample=None), b"group record"), (dict(nnz=C.c_void_p(66)), b"aligned"),
                      (dict(scalars=C.c_void_p(66)), b"aligned")):
        assert adv(**bad) == -1, bad
        msg = lib.tg_last_error()
        assert word in msg and msg.startswith(b"tg_rollout_advance_masked:"), (bad, msg)
    # the order of tg_rollout_advance: with everything wrong at once the first check speaks, and each one that is put
    # right hands over to the next
    wrong = dict(S=0, T=0, n=0, B=-3, dim_s=-1, step=-1, max_actions=0, frames=None, tokens=None, nnz=None, best=None,
                 scalars=C.c_void_p(66))
    for fix, word in ((dict(S=4), b"S=0"), (dict(T=2), b"T=0"), (dict(n=4), b"n=0"), (dict(B=9), b"B=-3"),
                      (dict(B=8), b"multiple of n"), (dict(dim_s=1), b"dim_s=-1"), (dict(step=5), b"step=-1"),
                      (dict(max_actions=6), b"max_actions=0"), (dict(frames=p), b"null frames"),
                      (dict(tokens=p), b"null tokens"), (dict(nnz=p), b"null nnz"), (dict(best=p), b"group record"),
                      (dict(scalars=p), b"aligned")):
        assert adv(**wrong) == -1
        assert word in lib.tg_last_error(), (fix, lib.tg_last_error())
        wrong.update(fix)
    # B = 0 returns 0 at once, with or without pointers, NULL `active` included; the sizes are still checked
    assert adv(B=0) == 0
    assert adv(B=0, active=None) == 0
    assert adv(B=0, frames=None, tokens=None, nnz=None, best=None, hits=None, sstep=None, ssample=None, active=None) == 0
    assert adv(B=0, actions=None, step=100, max_actions=0) == 0
    assert adv(B=0, S=0) == -1
    # a NULL `active` is not among the refusals: with it the first complaint is still about another argument
    assert adv(active=None, nnz=None) == -1 and b"null nnz" in lib.tg_last_error()


# ---- the restatements against each other on recorded data -----------------------------------------------------------
def both(policy_maker, states, n, K, shift):
    G = len(states)
    scal = np.arange(G, dtype=np.float32)[:, None]
    plain = M.plain_trace(policy_maker(), states, scal, n, K, shift)
    masked = M.rollout_masked(policy_maker(), states, scal, n, K, shift)
    return plain, masked


@pytest.mark.parametrize("shift,n,slot", [(1, 1, 0), (2, 1, 0), (1, 4, 2)])
def test_property_on_the_strassen_states(golden, shift, n, slot):
    states, scripts, lengths = strassen_scripts(golden, shift)
    states, scripts, lengths = states[::3], scripts[::3], lengths[::3]
    K = 9                                       # two steps past the latest solve (step 6)
    # every fifth group gets a script that never ends (the null action): it cannot be solved when n = 1
    stuck = np.arange(len(scripts)) % 5 == 4
    scripts = [[R.null_action(4, shift)] if s else sc for s, sc in zip(stuck, scripts)]
    plain, masked = both(lambda: R.scripted_policy(scripts, 4, n, slot, shift, seed=5), states, n, K, shift)
    n_solved, n_unsolved = M.check_property(masked, plain, plain.after)
    assert len(set(plain.solved_step[plain.solved_step >= 0])) >= 2 and n_unsolved >= 1
    if n == 1:
        assert np.array_equal(plain.solved_step >= 0, ~stuck)
        assert np.array_equal(plain.solved_step[~stuck], lengths[~stuck] - 1)
    assert plain.num_hits > masked.num_hits == n_solved == masked.num_solved == plain.num_solved
    for a, b in zip(R.solutions(masked), R.solutions(plain)):
        assert np.array_equal(a, b)
    for g, tok, L in zip(*R.solutions(masked)):
        assert not R.O.take_actions(list(tok[:L]), states[g, 0], shift).any()


def test_property_on_the_recorded_demonstrations(golden):
    for name, target, script in demo_cases(golden):
        S, K, T, n = target.shape[-1], len(script) + 2, 2, 4
        states = np.zeros((2, T, S, S, S), np.int8)
        states[:, 0] = target[:, 0]
        states[1, 0, 0, 0, 0] += 1              # one entry off: the same script leaves this group unsolved
        scripts = [script, script]
        plain, masked = both(lambda: R.scripted_policy(scripts, S, n, 2, 1, seed=3), states, n, K, 1)
        assert M.check_property(masked, plain, plain.after)[0] >= 1, name
        assert plain.solved_step[0] >= 0
        for a, b in zip(R.solutions(masked), R.solutions(plain)):
            assert np.array_equal(a, b)


def test_masked_restatement_check_every_and_first_row(golden):
    states, scripts, lengths = strassen_scripts(golden, 1)
    states, scripts, lengths = states[::9], scripts[::9], lengths[::9]
    G, K, k = len(scripts), 12, int(lengths.max()) - 1
    scal = np.zeros((G, 1), np.float32)
    full = M.rollout_masked(R.scripted_policy(scripts, 4, 1, 0, 1), states, scal, 1, K, 1)
    assert full.steps_run == K and full.num_solved == G
    for m in (1, 2, 3, 4, 5):
        got = M.rollout_masked(R.scripted_policy(scripts, 4, 1, 0, 1), states, scal, 1, K, 1, check_every=m)
        assert got.steps_run == -(-(k + 1) // m) * m <= K
        for name in M.RECORDS + M.ROWS + ("active",):
            assert np.array_equal(getattr(got, name), getattr(full, name)), (m, name)
    seen = []
    M.rollout_masked(lambda f, s, rows, step: seen.append(rows.copy()) or np.ones((len(rows), 12), np.int8),
                     states[:2], scal[:2], 3, 1, 1, first_row=30)
    assert list(seen[0]) == list(range(30, 36))


# ---- Python argument errors (no device) -------------------------------------------------------------------------------
def test_sample_rollouts_argument_errors():
    import torch
    from mat_mul_amd import TensorGameError, ops, rollout
    import mat_mul_amd
    assert mat_mul_amd.solve_states is rollout.solve_states
    states, scal = torch.zeros((2, 1, 4, 4, 4), dtype=torch.int8), torch.zeros((2, 1))
    policy = lambda *a, **k: None  # noqa: E731
    # the device check still comes first
    with pytest.raises(TensorGameError, match="no CPU path"):
        rollout.sample_rollouts(policy, states, scal, 4, 3, stop_solved=True, check_every=2, graph=True)
    with pytest.raises(TensorGameError, match="check_every=2.*graph=True"):
        rollout.sample_rollouts(policy, _Cuda(states), _Cuda(scal), 4, 3, stop_solved=True, check_every=2, graph=True)
    with pytest.raises(TensorGameError, match="check_every=2 needs stop_solved"):
        rollout.sample_rollouts(policy, _Cuda(states), _Cuda(scal), 4, 3, check_every=2)
    with pytest.raises(TensorGameError, match="check_every=-1"):
        rollout.sample_rollouts(policy, _Cuda(states), _Cuda(scal), 4, 3, stop_solved=True, check_every=-1)
    with pytest.raises(TensorGameError, match="first_row=-8"):
        rollout.sample_rollouts(policy, _Cuda(states), _Cuda(scal), 4, 3, first_row=-8)
    with pytest.raises(TensorGameError, match="chunk_groups=0"):
        rollout.solve_states(policy, states, scal, 4, 3, chunk_groups=0)
    with pytest.raises(TensorGameError, match="no CPU path"):
        rollout.solve_states(policy, states, scal, 4, 3, chunk_groups=1)
    with pytest.raises(TensorGameError, match="stop_solved=True"):
        ops.rollout_advance(_Cuda(torch.zeros((4, 1, 4, 4, 4), dtype=torch.int8)), torch.zeros((4, 12), dtype=torch.int8),
                            2, 0, ops.rollout_records(2, 4, "cpu"), active=torch.ones(4, dtype=torch.uint8))
    res = rollout.RolloutResult(*([None] * 15))
    assert res.graph is None and res.active is None and res.steps_run == 0      # the new fields come last, with defaults


class _Cuda:
    """A tensor that says it lives on a ROCm device, for the checks that sample_rollouts makes before it touches one."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    @property
    def device(self):
        import torch
        return torch.device("cuda:0")

    def __getattr__(self, name):
        return getattr(self._t, name)
