"""Sampled policy rollouts: the solution search of the reference's SyntheticDemoTrainingApp (training.py:325-352).

Every start state is copied ``n_samples`` times, the network samples ONE action per copy, the copies are stepped
(``_take_action``, training.py:249-268), and this repeats ``max_actions`` times while the lowest non-zero count and the
steps at which a copy reached the zero tensor are tracked.  Here a step is the policy's launches plus ONE more
(``tg_rollout_advance``, include/tensor_game_rollout.h): the int8 frames are stepped in place and are the next torso
input as they stand, the statistics stay on the device, and the played tokens are recorded, so a solved group can be
turned back into the factorisation that was found.  Nothing in the loop synchronises with the host.

    res = sample_rollouts(net.rollout_policy(seed=0), states, scalars, n_samples=8, max_actions=7)
    res.num_solved.item(), res.lowest_rank.item()       # the first host syncs
    groups, tokens, lengths = res.solutions()             # action lists that replay the start states to zero

Two deliberate differences from training.py.  Its ``fwd_infer(..., n_samples=1)`` call (:252) does not run as written
(fwd_infer takes no such argument); the policy here draws one action per row.  Its ``repeat(n_samples, ...)`` (:332)
followed by ``view(-1, n_samples, ...)`` (:259) groups copies of DIFFERENT states; here a group is the n samples of one
state (rows are group-major: row g*n + s is sample s of state g).  ``shift`` defaults to 1, the live path's
vocabulary; the reference hard-codes ``- 2`` (:253, the Strassen vocabulary): pass ``shift=2`` for that.

``stop_solved=True`` stops a group at the step that solves it (``tg_rollout_advance_masked``): its rows are not stepped
again and a policy with ``takes_active = True`` (``FusedAlphaTensor.rollout_policy(seed, masked=True)``) does not
evaluate them, ``check_every=m`` leaves the loop once no group is left, and ``solve_states`` runs a whole dataset that
way, chunk by chunk (the dataset loop of training.py:331-346).

``solve_stream`` runs the same dataset through ``slots`` resident groups that are refilled from a device-side queue
(include/tensor_game_rollout_slots.h): a group that is solved or out of steps is flushed and takes the next start state
in the same tick, so every policy call stays full until the queue is drained and the host reads one word now and then.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import TensorGameError

__all__ = ["sample_rollouts", "RolloutResult", "model_policy", "RolloutPolicy", "solve_states", "SolveResult",
           "solve_stream"]

# (frames int8 (B,T,S,S,S), scalars float32 (B,dim_s), rows int64 (B,), step) -> tokens int8 (B,3S)
RolloutPolicy = Callable[[torch.Tensor, torch.Tensor, torch.Tensor, int], torch.Tensor]


@dataclass
class RolloutResult:
    """What ``sample_rollouts`` leaves on the device.  Per group (int32 (G,)): ``best_nnz`` the lowest non-zero count
    any sample reached at any step, ``hits`` the number of steps at which some sample was at zero, ``solved_step`` the
    first such step (-1: never) and ``solved_sample`` the lowest sample index at zero at that step.  ``frames`` int8
    (B,T,S,S,S) and ``scalars`` are the final rows, ``nnz`` int32 (B,) the last step's counts, ``overflow`` uint8 (B,)
    is set where an entry ever left int8, ``actions`` int8 (B,max_actions,3S) the played tokens (None unless
    recorded).  ``lowest_rank`` (the reference's lowest_rank, :343), ``num_hits`` (its num_solutions_found, :346) and
    ``num_solved`` (groups with a solution) are 0-d device tensors.

    After ``stop_solved=True``: ``hits`` is 0 or 1; ``frames``, ``scalars`` and ``nnz`` of a solved group are those right
    after its solving step (the winning row's head is zero) and its ``actions`` beyond ``solved_step`` are zero;
    ``active`` uint8 (B,) is 1 on the rows of the unsolved groups (None otherwise).  ``steps_run`` is the number of
    steps the loop made (``max_actions`` unless ``check_every`` ended it early)."""

    n_samples: int
    max_actions: int
    shift: int
    best_nnz: torch.Tensor
    hits: torch.Tensor
    solved_step: torch.Tensor
    solved_sample: torch.Tensor
    frames: torch.Tensor
    scalars: torch.Tensor
    nnz: torch.Tensor
    overflow: torch.Tensor
    actions: Optional[torch.Tensor]
    lowest_rank: torch.Tensor
    num_hits: torch.Tensor
    num_solved: torch.Tensor
    graph: Optional[torch.cuda.CUDAGraph] = None  # the captured loop (graph=True): kept alive with its results
    active: Optional[torch.Tensor] = None
    steps_run: int = 0

    def solutions(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """For every solved group, gathered on the device: (groups int64 (M,), tokens int8 (M,max_actions,3S),
        lengths int64 (M,)).  tokens[m, :lengths[m]] are the winning sample's actions 0 .. solved_step, which replay
        start state groups[m] to zero; the rows beyond the length are zero."""
        if self.actions is None:
            raise TensorGameError("solutions", -1, "the rollout did not record its actions (record_actions=False)")
        groups = torch.nonzero(self.solved_step >= 0).flatten()
        rows = groups * self.n_samples + self.solved_sample[groups].to(torch.int64)
        lengths = self.solved_step[groups].to(torch.int64) + 1
        tokens = self.actions[rows]
        keep = torch.arange(self.max_actions, device=tokens.device)[None, :] < lengths[:, None]
        return groups, tokens * keep[:, :, None].to(torch.int8), lengths


def model_policy(model) -> RolloutPolicy:
    """Wrap an ``AlphaTensor``-like torch model (``fwd_infer(states, scalars) -> (tokens (B,k,3S), probs, q)``,
    model.py:347-356): the first of its samples is the row's action.  Not capturable (``ops.as_tokens`` checks the
    token range on the host)."""

    @torch.no_grad()
    def policy(frames, scalars, rows, step):
        aa = model.fwd_infer(frames.float(), scalars)[0]
        B = frames.shape[0]
        return ops.as_tokens(aa.reshape(B, -1, aa.shape[-1])[:, 0], frames.device)

    return policy


def sample_rollouts(policy: RolloutPolicy, states: torch.Tensor, scalars: torch.Tensor, n_samples: int,
                    max_actions: int, shift: int = 1, record_actions: bool = True, graph: bool = False,
                    stop_solved: bool = False, check_every: int = 0, first_row: int = 0) -> RolloutResult:
    """Roll every start state out ``n_samples`` times for ``max_actions`` steps of ``policy -> advance``.

    states int8 (G,T,S,S,S) (newest frame first), scalars float32 (G,dim_s); neither is modified.  ``policy`` sees the
    B = G*n_samples rows (group-major) and their global row indices, so that the samples of one state draw
    differently.  ``graph=True`` captures the whole loop once (a linear chain of launches) and replays it: only for
    policies that can be captured (``FusedAlphaTensor.rollout_policy`` can); the results equal the eager loop bit for
    bit.

    ``stop_solved``: a group is stepped up to the step that solves it and left alone from then on (see
    ``RolloutResult``); a policy with ``takes_active = True`` is called as ``policy(frames, scalars, rows, step,
    active=..., out=tokens)`` with the row mask and one persistent int8 (B,3S) token buffer, any other policy on all
    rows as without it.  For a policy whose action depends only on the row and on (row, step), the records of the
    unsolved groups, and ``solved_step``, ``solved_sample``, ``best_nnz`` and ``solutions()`` of the solved ones, equal
    those without ``stop_solved``.  ``check_every = m > 0`` (with ``stop_solved``, eager only) reads
    ``(solved_step < 0).any()`` on the host after every m-th step and leaves the loop when no group is active; the
    results do not depend on m.  ``graph=True`` still captures all ``max_actions`` steps: the mask is read when the
    kernels run.  ``first_row`` is added to the row indices that key the policy's stream (``solve_states``)."""
    if not states.is_cuda:
        raise TensorGameError("sample_rollouts", -1, f"states must live on a ROCm device (got {states.device}); there "
                              "is no CPU path")
    if states.dtype != torch.int8 or states.dim() != 5 or not (states.shape[2] == states.shape[3] == states.shape[4]):
        raise TensorGameError("sample_rollouts", -1, f"states must be int8 (G,T,S,S,S), got {states.dtype} "
                              f"{tuple(states.shape)}")
    G, T, S = states.shape[0], states.shape[1], states.shape[2]
    dev = states.device
    if scalars.dim() != 2 or scalars.shape[0] != G or scalars.dtype != torch.float32 or scalars.device != dev:
        raise TensorGameError("sample_rollouts", -1, f"scalars must be float32 ({G},dim_s) on {dev}, got "
                              f"{scalars.dtype} {tuple(scalars.shape)} on {scalars.device}")
    n, K, m = int(n_samples), int(max_actions), int(check_every)
    if K < 1:
        raise TensorGameError("sample_rollouts", -1, f"max_actions={max_actions} < 1")
    if m < 0:
        raise TensorGameError("sample_rollouts", -1, f"check_every={check_every} < 0")
    if m and graph:
        raise TensorGameError("sample_rollouts", -1, f"check_every={m} reads the records on the host between steps: "
                              "not with graph=True (a captured loop runs all max_actions steps)")
    if m and not stop_solved:
        raise TensorGameError("sample_rollouts", -1, f"check_every={m} needs stop_solved=True: without it every step "
                              "changes the results of the solved groups")
    if int(first_row) < 0:
        raise TensorGameError("sample_rollouts", -1, f"first_row={first_row} < 0")
    B = G * max(n, 0)
    ops.rollout_check(B, n, S, T, scalars.shape[1], 0, K, record_actions)
    frames = states.repeat_interleave(n, dim=0).contiguous()
    scal = scalars.repeat_interleave(n, dim=0).contiguous()
    rows = torch.arange(int(first_row), int(first_row) + B, device=dev, dtype=torch.int64)
    records = ops.rollout_records(G, S, dev)
    nnz = torch.zeros((B,), dtype=torch.int32, device=dev)
    overflow = torch.zeros((B,), dtype=torch.uint8, device=dev)
    actions = torch.zeros((B, K, 3 * S), dtype=torch.int8, device=dev) if record_actions else None

    active = torch.ones((B,), dtype=torch.uint8, device=dev) if stop_solved else None
    takes_active = stop_solved and bool(getattr(policy, "takes_active", False))
    token_buf = torch.zeros((B, 3 * S), dtype=torch.int8, device=dev) if takes_active else None

    def one(step: int) -> None:
        if takes_active:
            tokens = policy(frames, scal, rows, step, active=active, out=token_buf)
            if tokens is not token_buf:
                raise TensorGameError("policy", -1, "a policy with takes_active returns the token buffer `out`")
        else:
            tokens = policy(frames, scal, rows, step)
        ops.rollout_advance(frames, tokens, n, step, records, scalars=scal, nnz=nnz, overflow=overflow,
                            actions=actions, shift=shift, active=active, stop_solved=stop_solved)

    g = None
    steps_run = K if B else 0
    if graph and B:
        # one warm-up step outside the capture (lazy initialisation of the policy's launches), then undone
        keep = (frames.clone(), scal.clone())
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            one(0)
            frames.copy_(keep[0])
            scal.copy_(keep[1])
            for r, fresh in zip(records, ops.rollout_records(G, S, dev)):
                r.copy_(fresh)
            overflow.zero_()
            if stop_solved:
                active.fill_(1)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for step in range(K):
                one(step)
        g.replay()
    elif B:
        for step in range(K):
            one(step)
            if m and (step + 1) % m == 0 and not bool((records[2] < 0).any()):
                steps_run = step + 1
                break
    best_nnz, hits, solved_step, solved_sample = records
    return RolloutResult(n, K, int(shift), best_nnz, hits, solved_step, solved_sample, frames, scal, nnz, overflow,
                         actions, best_nnz.min() if G else torch.tensor(S ** 3, dtype=torch.int32, device=dev),
                         hits.sum(), (solved_step >= 0).sum(), g, active, steps_run)


@dataclass
class SolveResult:
    """What ``solve_states`` leaves on the device: the per-group records of ``RolloutResult`` for all G states (int32
    (G,) each) and ``solutions()`` of all chunks -- ``groups`` int64 (M,) indexes ``states``, ``tokens`` int8
    (M,max_actions,3S), ``lengths`` int64 (M,).  ``steps_run`` has one entry per chunk and is the only field that
    depends on the chunking.  ``solve_stream`` also fills ``overflow`` uint8 (G,) (1 where an entry of some row of the
    state left int8) and ``ticks`` (the policy calls it made; ``steps_run`` = (ticks,))."""

    best_nnz: torch.Tensor
    hits: torch.Tensor
    solved_step: torch.Tensor
    solved_sample: torch.Tensor
    groups: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    steps_run: Sequence[int]
    overflow: Optional[torch.Tensor] = None
    ticks: int = 0


def solve_states(policy: RolloutPolicy, states: torch.Tensor, scalars: torch.Tensor, n_samples: int, max_actions: int,
                 chunk_groups: int, check_every: int = 1, shift: int = 1) -> SolveResult:
    """The solution search over a dataset of start states (the loop of training.py:331-346): the states go through
    ``sample_rollouts(stop_solved=True, check_every=check_every)`` in chunks of ``chunk_groups``, every chunk with
    ``first_row`` = its first state's index * n_samples, so a row draws the same actions whatever the chunking; the
    records and the solutions are concatenated on the device.  The results do not depend on ``chunk_groups`` for a
    policy that decides from the row, its state and the step alone."""
    c = int(chunk_groups)
    if c < 1:
        raise TensorGameError("solve_states", -1, f"chunk_groups={chunk_groups} < 1")
    n = int(n_samples)
    G = states.shape[0] if states.dim() else 0
    parts = [sample_rollouts(policy, states[g0:g0 + c], scalars[g0:g0 + c], n, max_actions, shift=shift,
                             stop_solved=True, check_every=check_every, first_row=g0 * n) for g0 in range(0, G, c)]
    if not parts:  # no states: one empty rollout has the right shapes and checks the arguments
        parts = [sample_rollouts(policy, states, scalars, n, max_actions, shift=shift, stop_solved=True)]
    sols = [p.solutions() for p in parts]
    cat = lambda xs: torch.cat(list(xs))  # noqa: E731
    return SolveResult(cat(p.best_nnz for p in parts), cat(p.hits for p in parts), cat(p.solved_step for p in parts),
                       cat(p.solved_sample for p in parts),
                       cat(s[0] + i * c for i, s in enumerate(sols)), cat(s[1] for s in sols),
                       cat(s[2] for s in sols), tuple(p.steps_run for p in parts))


def solve_stream(policy, states: torch.Tensor, scalars: torch.Tensor, n_samples: int, max_actions: int, slots: int,
                 check_every: int = 8, shift: int = 1, graph: bool = False, first_state: int = 0) -> SolveResult:
    """``solve_states`` with continuous refill: ``slots`` groups of ``n_samples`` rows stay resident; after every step
    the finished ones (solved, or ``max_actions`` steps old) are flushed to per-state outputs and take the next start
    states in slot order (``ops.rollout_refill``), so a tick is ``policy -> advance_slots -> refill`` on full launches
    until the dataset is drained.  Every ``check_every`` ticks (0: never before the bound) the host reads the number of
    occupied slots and leaves when it is 0; after ``max_actions * (N // slots + 1)`` ticks, the makespan bound of
    handing states out greedily, the loop ends either way and raises if a slot is still occupied.

    A row's stream is keyed by ``(first_state + state index) * n_samples + sample`` and by the row's OWN step, so for
    a policy that decides from the row key, the row's state and that step, every field but ``steps_run`` / ``ticks``
    equals ``solve_states`` bit for bit, for every ``slots`` >= 1.

    ``policy`` with ``takes_slots = True`` (``FusedAlphaTensor.slot_policy(seed)``; it exposes ``seed``) is called as
    ``policy(frames, scalars, rows, steps, active=..., uniforms=..., out=...)``: ``steps`` int32 (B,) is each row's own
    step, ``uniforms`` float32 (B,1,3S) the row's draws for that step, ``out`` the persistent int8 (B,3S) token buffer
    it returns.  Any other policy is called as ``policy(frames, scalars, rows, steps)`` and no uniforms are generated.
    ``graph=True`` captures ONE tick (a linear chain: nothing in it depends on a host step number) and replays it,
    reading the occupied count between blocks of ``check_every`` replays; the results equal the eager loop."""
    if not states.is_cuda:
        raise TensorGameError("solve_stream", -1, f"states must live on a ROCm device (got {states.device}); there is "
                              "no CPU path")
    if states.dtype != torch.int8 or states.dim() != 5 or not (states.shape[2] == states.shape[3] == states.shape[4]):
        raise TensorGameError("solve_stream", -1, f"states must be int8 (N,T,S,S,S), got {states.dtype} "
                              f"{tuple(states.shape)}")
    N, T, S = states.shape[0], states.shape[1], states.shape[2]
    dev = states.device
    if scalars.dim() != 2 or scalars.shape[0] != N or scalars.dtype != torch.float32 or scalars.device != dev:
        raise TensorGameError("solve_stream", -1, f"scalars must be float32 ({N},dim_s) on {dev}, got "
                              f"{scalars.dtype} {tuple(scalars.shape)} on {scalars.device}")
    n, K, R, m = int(n_samples), int(max_actions), int(slots), int(check_every)
    if K < 1:
        raise TensorGameError("solve_stream", -1, f"max_actions={max_actions} < 1")
    if R < 1:
        raise TensorGameError("solve_stream", -1, f"slots={slots} < 1")
    if m < 0:
        raise TensorGameError("solve_stream", -1, f"check_every={check_every} < 0")
    if int(first_state) < 0:
        raise TensorGameError("solve_stream", -1, f"first_state={first_state} < 0")
    dim_s = scalars.shape[1]
    sl = ops.rollout_slots(R, n, S, T, dim_s, K, dev)
    states, scalars = states.contiguous(), scalars.contiguous()
    kw = dict(dtype=torch.int32, device=dev)
    # a state the queue never hands out (there is none unless the loop fails) reads as unsolved
    out = (torch.full((N,), S ** 3, **kw), torch.zeros((N,), **kw), torch.full((N,), -1, **kw),
           torch.full((N,), -1, **kw), torch.zeros((N,), dtype=torch.uint8, device=dev),
           torch.zeros((N, K, 3 * S), dtype=torch.int8, device=dev))
    takes_slots = bool(getattr(policy, "takes_slots", False))
    seed = int(policy.seed) if takes_slots else 0
    steps = torch.zeros((R * n,), dtype=torch.int32, device=dev)

    def refill() -> None:
        ops.rollout_refill(sl, states, scalars, out, seed=seed, first_state=first_state, uniforms=takes_slots)

    def tick() -> None:
        steps.view(R, n).copy_(sl.slot_step.view(R, 1).expand(R, n))
        if takes_slots:
            tokens = policy(sl.frames, sl.scalars, sl.rows, steps, active=sl.active, uniforms=sl.uniforms,
                            out=sl.tokens)
            if tokens is not sl.tokens:
                raise TensorGameError("policy", -1, "a policy with takes_slots returns the token buffer `out`")
        else:
            tokens = policy(sl.frames, sl.scalars, sl.rows, steps)
        ops.rollout_advance_slots(sl, tokens, shift=shift)
        refill()

    bound = K * (N // R + 1)
    ticks, live, g = 0, 0, None
    if N:
        refill()
        if graph:
            # one warm-up tick on a side stream (lazy initialisation of the policy's launches); it is a real tick
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                tick()
            torch.cuda.current_stream(dev).wait_stream(side)
            ticks = 1
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                tick()
            run = g.replay
        else:
            run = tick
        live = -1
        if m and ticks and ticks % m == 0:
            live = int(sl.live.item())
        while live != 0 and ticks < bound:
            run()
            ticks += 1
            if m and ticks % m == 0:
                live = int(sl.live.item())
        if live != 0:
            live = int(sl.live.item())
        if live != 0:
            raise TensorGameError("solve_stream", -1, f"{live} slots are still occupied after {ticks} ticks, the bound "
                                  f"max_actions * (N // slots + 1) = {bound}: the refill does not drain the queue")
    best_nnz, hits, solved_step, solved_sample, overflow, tokens = out
    groups = torch.nonzero(solved_step >= 0).flatten()
    return SolveResult(best_nnz, hits, solved_step, solved_sample, groups, tokens[groups],
                       solved_step[groups].to(torch.int64) + 1, (ticks,), overflow, ticks)
