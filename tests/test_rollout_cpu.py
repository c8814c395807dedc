"""CPU checks of the sampled policy rollout: the numpy restatement (tests/rollout_ref.py) against reference-recorded
factorisations, and the C ABI of include/tensor_game_rollout.h (plain C, exported, validated without a device)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mat_mul_amd import _lib
from oracle import tensor_game as O

import rollout_ref as R
from rollout_ref import demo_cases, strassen_scripts

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "tensor_game_rollout.h"


# ---- the restatement against recorded data --------------------------------------------------------------------------
def check_scripted(res, scripts, lengths, n, slot, start_states, shift, K):
    """What a scripted rollout must show: solved at exactly the script's last step, hits growing by one per step from
    there on (the null action keeps the zero tensor), and solutions() replaying the start state to zero."""
    lengths = np.asarray(lengths)
    G = len(scripts)
    for g in range(G):
        L = int(lengths[g])
        if L == 0:  # an all-zero start: nothing to find before step 0 ends; the null action keeps it solved
            assert res.solved_step[g] == 0
            continue
        assert res.solved_step[g] <= L - 1
        if n == 1:
            assert res.solved_step[g] == L - 1
            assert res.trace[L - 1][1][g] == 1                      # hits == 1 at that point
            assert res.hits[g] == K - (L - 1)                       # then one more per step
            assert res.solved_sample[g] == 0
    groups, tokens, lens = R.solutions(res)
    assert len(groups) == G
    for g, tok, L in zip(groups, tokens, lens):
        final = O.take_actions(list(tok[:L]), start_states[g, 0], shift)
        assert not final.any(), g
        assert not tok[L:].any()
        if L > 1:  # not solved one step earlier
            assert O.take_actions(list(tok[:L - 1]), start_states[g, 0], shift).any()


@pytest.mark.parametrize("shift", [1, 2])
def test_strassen_states_are_solved_in_exactly_minus_reward_steps(golden, shift):
    states, scripts, lengths = strassen_scripts(golden, shift)
    assert states.shape == (448, 1, 4, 4, 4) and sorted(set(lengths)) == list(range(1, 8))
    K = 9
    pol = R.scripted_policy(scripts, 4, 1, 0, shift)
    res = R.rollout(pol, states, np.zeros((448, 1), np.float32), 1, K, shift)
    check_scripted(res, scripts, lengths, 1, 0, states, shift, K)
    assert res.num_solved == 448 and res.lowest_rank == 0
    assert res.num_hits == int((K - (lengths - 1)).sum())
    assert np.array_equal(res.scalars, np.full((448, 1), K, np.float32))
    assert not res.overflow.any() and not res.frames.any()


def test_recorded_demonstrations_are_solved_by_their_action_lists(golden):
    for name, target, script in demo_cases(golden):
        S, K = target.shape[-1], len(script) + 2
        for T in (1, 3):
            states = np.zeros((1, T, S, S, S), np.int8)
            states[:, 0] = target[:, 0]
            res = R.rollout(R.scripted_policy([script], S, 1, 0, 1), states, np.zeros((1, 1), np.float32), 1, K, 1)
            groups, tokens, lens = R.solutions(res)
            assert list(groups) == [0], name
            assert not O.take_actions(list(tokens[0][:lens[0]]), target[0, 0], 1).any()
            assert res.solved_step[0] <= len(script) - 1
            assert np.array_equal(tokens[0][:lens[0]], np.stack(script)[:lens[0]])


def test_scripted_slot_among_random_samples(golden):
    """n = 4, the script in sample slot 2, seeded random tokens elsewhere: solved_sample is 2 unless a lower slot is at
    zero at that step too -- which the per-row counts of the restatement itself decide."""
    states, scripts, lengths = strassen_scripts(golden, 1)
    states, scripts, lengths = states[::7], scripts[::7], lengths[::7]
    G, n, K = len(scripts), 4, 8
    pol = R.scripted_policy(scripts, 4, n, 2, 1, seed=5)
    res = R.rollout(pol, states, np.zeros((G, 1), np.float32), n, K, 1)
    assert res.num_solved == G
    # replay the rows independently and decide the expected records from the per-row histories
    pol2 = R.scripted_policy(scripts, 4, n, 2, 1, seed=5)
    heads = np.repeat(states[:, 0], n, axis=0)
    zero_at = np.zeros((K, G * n), bool)
    for k in range(K):
        heads = O.step_i8(heads, pol2(None, None, None, k), 1)[0]
        zero_at[k] = ~heads.reshape(G * n, -1).any(axis=1)
    for g in range(G):
        per_step = zero_at[:, g * n:(g + 1) * n]
        first_step = int(np.argmax(per_step.any(axis=1)))
        assert res.solved_step[g] == first_step <= lengths[g] - 1
        assert res.solved_sample[g] == int(np.argmax(per_step[first_step]))
        assert res.solved_sample[g] <= 2
        assert res.hits[g] == int(per_step.any(axis=1).sum())
    check_scripted(res, scripts, lengths, n, 2, states, 1, K)
    assert (res.solved_sample == 2).sum() > G // 2  # the random slots rarely get there first


def test_restatement_step_equals_the_reference_arithmetic():
    """advance() against training.py:253-268 written out with the oracle's layer-1 functions (no int8 narrowing at
    these magnitudes), T = 3, n = 2."""
    rng = np.random.default_rng(1)
    frames = rng.integers(-2, 3, size=(6, 3, 3, 3, 3)).astype(np.int8)
    tokens = rng.integers(0, 3, size=(6, 9)).astype(np.int8)
    new, nnz, rec, sc, ovf, act = R.advance(frames, tokens, 2, 0, R.fresh_records(3, 3), np.zeros((6, 1), np.float32),
                                            np.zeros(6, np.uint8), np.zeros((6, 2, 9), np.int8), 1)
    want_head = frames[:, 0].astype(np.int64) - O.action_to_tensor(tokens, 1)
    assert np.array_equal(new[:, 0], want_head) and np.array_equal(new[:, 1:], frames[:, :-1])
    assert np.array_equal(nnz, (want_head != 0).reshape(6, -1).sum(1))
    assert np.array_equal(rec[0], nnz.reshape(3, 2).min(1)) and not ovf.any() and (sc == 1).all()
    assert np.array_equal(act[:, 0], tokens) and not act[:, 1].any()


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def declared_symbols():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(tg_[a-z0-9_]+)\s*\(", HEADER.read_text(), flags=re.M)))


def test_rollout_header_symbols_all_exported():
    syms = declared_symbols()
    assert syms == ["tg_rollout_advance", "tg_rollout_check"]
    assert sorted(_lib.ROLLOUT_SIGNATURES) == syms
    lib = C.CDLL(str(_lib.LIB_PATH))
    for s in syms:
        assert hasattr(lib, s), s
    from mat_mul_amd import build
    assert HEADER in build.HEADERS
    ab = C.CDLL(str(build.lib_path(ab=True)))
    for s in syms:
        assert hasattr(ab, s), s


def test_rollout_header_is_plain_c():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang")
    gcc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert gcc is not None, "a C compiler is needed to check that the header is plain C"
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror", str(HEADER)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_abi_argument_validation_without_gpu_rollout():
    lib = _lib.lib
    p = C.c_void_p(64)  # never dereferenced: every call below is refused before any launch

    def adv(frames=p, tokens=p, scalars=p, nnz=p, overflow=p, best=p, hits=p, sstep=p, ssample=p, actions=p, B=8, n=4,
            S=4, T=2, dim_s=1, step=0, max_actions=4, shift=1):
        return lib.tg_rollout_advance(frames, tokens, scalars, nnz, overflow, best, hits, sstep, ssample, actions, B, n,
                                      S, T, dim_s, step, max_actions, shift, None)

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
        assert word in lib.tg_last_error(), (bad, lib.tg_last_error())
    # without the optional outputs the step bound of the actions record does not apply
    assert adv(B=0, actions=None, step=100, max_actions=0) == 0
    assert adv(B=0) == 0                                                   # B = 0 is a no-op
    assert adv(B=0, frames=None, tokens=None, nnz=None, best=None, hits=None, sstep=None, ssample=None) == 0
    assert adv(B=0, S=0) == -1                                             # but still a checked one
    assert lib.tg_rollout_check(8, 4, 4, 2, 1, 0, 4, 1) == 0
    assert lib.tg_rollout_check(128, 64, 32, 8, 64, 0, 1, 1) == 0
    assert lib.tg_rollout_check(8, 3, 4, 2, 1, 0, 4, 1) == -1
    assert lib.tg_rollout_check(8, 4, 4, 2, 1, 7, 4, 0) == 0
    assert lib.tg_rollout_check(8, 4, 4, 2, 1, 7, 4, 1) == -1


def test_python_entry_points_refuse_without_a_device():
    import torch
    from mat_mul_amd import TensorGameError, ops, rollout
    import mat_mul_amd
    assert mat_mul_amd.sample_rollouts is rollout.sample_rollouts and mat_mul_amd.RolloutResult is rollout.RolloutResult
    states = torch.zeros((2, 1, 4, 4, 4), dtype=torch.int8)
    with pytest.raises(TensorGameError, match="no CPU path"):
        rollout.sample_rollouts(lambda *a: None, states, torch.zeros((2, 1)), 4, 3)
    with pytest.raises(TensorGameError, match="no CPU path"):
        ops.rollout_advance(torch.zeros((4, 1, 4, 4, 4), dtype=torch.int8), torch.zeros((4, 12), dtype=torch.int8), 2, 0,
                            ops.rollout_records(2, 4, "cpu"))
    with pytest.raises(TensorGameError, match="multiple of n"):
        ops.rollout_check(9, 4, 4, 1)
    ops.rollout_check(8, 4, 4, 1)
