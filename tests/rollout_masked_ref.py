"""numpy restatement of the solution search that stops solved groups (tg_rollout_advance_masked of
include/tensor_game_rollout_masked.h, ``sample_rollouts(stop_solved=True)`` and ``solve_states`` of
mat_mul_amd/rollout.py), on top of tests/rollout_ref.py, and the relation between a masked and a plain run that makes
the feature checkable.  Shared by test_rollout_masked_cpu.py and test_gpu_rollout_masked.py."""
import numpy as np

import rollout_ref as R

RECORDS = ("best_nnz", "hits", "solved_step", "solved_sample")
ROWS = ("frames", "scalars", "nnz", "overflow", "actions")


def advance_masked(frames, tokens, n, step, records, nnz, scalars=None, overflow=None, actions=None, active=None,
                   shift=1):
    """One masked step.  A group is active iff its solved_step is negative on entry; active groups get what
    ``rollout_ref.advance`` gives them, the others keep everything.  The tokens of inactive rows are replaced before
    they reach ``advance``: they cannot matter.  Returns (frames, nnz, records, scalars, overflow, actions, active); no
    input is modified."""
    frames, tokens, nnz = np.asarray(frames), np.array(tokens, np.int8), np.asarray(nnz, np.int32)
    S = frames.shape[2]
    act_g = np.asarray(records[2]) < 0
    act_r = np.repeat(act_g, n)
    tokens[~act_r] = R.null_action(S, shift)
    new, nnz2, rec2, sc2, ovf2, act2 = R.advance(frames, tokens, n, step, records, scalars, overflow, actions, shift)

    def pick(mask, a, b):
        if a is None:
            return None
        m = mask.reshape((-1,) + (1,) * (np.asarray(a).ndim - 1))
        return np.where(m, a, b).astype(np.asarray(b).dtype)

    out_rec = tuple(pick(act_g, a, b) for a, b in zip(rec2, records))
    if active is not None:
        still = np.repeat(out_rec[2] < 0, n).astype(np.uint8)
        active = pick(act_r, still, np.asarray(active, np.uint8))
    return (pick(act_r, new, frames), pick(act_r, nnz2, nnz), out_rec, pick(act_r, sc2, scalars),
            pick(act_r, ovf2, overflow), pick(act_r, act2, actions), active)


def rollout_masked(policy, states, scalars, n, max_actions, shift=1, check_every=0, first_row=0):
    """The loop of ``sample_rollouts(stop_solved=True, check_every=..., first_row=...)``: policy(frames, scalars, rows,
    step) -> tokens int8 (B,3S) is asked for all rows."""
    states = np.asarray(states, np.int8)
    G, T, S = states.shape[:3]
    frames = np.repeat(states, n, axis=0)
    scal = np.repeat(np.asarray(scalars, np.float32), n, axis=0)
    B = G * n
    rows = np.arange(first_row, first_row + B, dtype=np.int64)
    rec = R.fresh_records(G, S)
    overflow, nnz, active = np.zeros(B, np.uint8), np.zeros(B, np.int32), np.ones(B, np.uint8)
    actions = np.zeros((B, max_actions, 3 * S), np.int8)
    r = R.Result()
    r.steps_run = max_actions if B else 0
    for step in range(max_actions if B else 0):
        tokens = np.asarray(policy(frames, scal, rows, step), np.int8)
        frames, nnz, rec, scal, overflow, actions, active = advance_masked(frames, tokens, n, step, rec, nnz, scal,
                                                                           overflow, actions, active, shift)
        if check_every and (step + 1) % check_every == 0 and not (rec[2] < 0).any():
            r.steps_run = step + 1
            break
    r.n_samples, r.max_actions, r.shift = n, max_actions, shift
    r.best_nnz, r.hits, r.solved_step, r.solved_sample = rec
    r.frames, r.scalars, r.nnz, r.overflow, r.actions, r.active = frames, scal, nnz, overflow, actions, active
    r.lowest_rank = int(r.best_nnz.min()) if G else S ** 3
    r.num_hits = int(r.hits.sum())
    r.num_solved = int((r.solved_step >= 0).sum())
    return r


def plain_trace(policy, states, scalars, n, max_actions, shift=1):
    """``rollout_ref.rollout`` that also keeps the frames as they are after every step: ``.after[k]``."""
    after = []

    def spy(frames, scal, rows, step):
        if step:
            after.append(frames.copy())
        return policy(frames, scal, rows, step)

    r = R.rollout(spy, states, scalars, n, max_actions, shift)
    after.append(r.frames.copy())
    r.after = after
    return r


def check_property(masked, plain, after=None, get=np.asarray):
    """The relation between a masked run and the plain run of the same inputs, for a policy whose action depends only
    on the row and on (row, step).  ``masked`` / ``plain`` have the fields of RolloutResult (``get`` turns one into a
    numpy array); ``after`` (``plain_trace(...).after``) also checks the frozen frames of the solved groups.  Returns
    (number of solved groups, number of unsolved groups)."""
    n, K = plain.n_samples, plain.max_actions
    sstep = get(plain.solved_step)
    solved = sstep >= 0
    rows_u = np.repeat(~solved, n)
    for name in RECORDS:  # solved_step, solved_sample and best_nnz are equal for every group
        if name != "hits":
            assert np.array_equal(get(getattr(masked, name)), get(getattr(plain, name))), name
    hits = get(masked.hits)
    assert np.array_equal(hits[~solved], get(plain.hits)[~solved]) and not hits[~solved].any()
    assert (hits[solved] == 1).all()
    for name in ROWS:  # unsolved groups: bit for bit
        assert np.array_equal(get(getattr(masked, name))[rows_u], get(getattr(plain, name))[rows_u]), name
    m_act, p_act, m_sc = get(masked.actions), get(plain.actions), get(masked.scalars)
    m_frames, p_scal0 = get(masked.frames), get(plain.scalars) - np.float32(K)
    m_nnz, m_sample = get(masked.nnz), get(masked.solved_sample)
    for g in np.nonzero(solved)[0]:
        rows, L = slice(g * n, (g + 1) * n), int(sstep[g]) + 1
        assert np.array_equal(m_act[rows, :L], p_act[rows, :L]) and not m_act[rows, L:].any(), g
        assert np.array_equal(m_sc[rows], p_scal0[rows] + np.float32(L)), g     # scalars + 1 per step that ran
        assert not m_frames[g * n + int(m_sample[g]), 0].any(), g  # the winning row's head is zero
        if after is not None:
            assert np.array_equal(m_frames[rows], after[L - 1][rows]), g
            head_nnz = (after[L - 1][rows, 0] != 0).reshape(n, -1).sum(1)
            assert np.array_equal(m_nnz[rows], head_nnz), g
    if getattr(masked, "active", None) is not None:
        assert np.array_equal(get(masked.active), rows_u.astype(np.uint8))
    return int(solved.sum()), int((~solved).sum())
