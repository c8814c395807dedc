"""Batched self-play search: a forest of B Monte Carlo search trees resident in HBM (include/tensor_game_search.h).

The reference plays one game at a time (``actor_prediction`` -> ``mc_ts`` -> ``extend_tree``, act.py:8-301) with the
tree in Python dicts and a ``.item()`` round trip per descent step.  Here every game has its own tree in device memory
and each simulation is two launches for all games -- ``select`` (descent to a leaf, model input out) and ``commit``
(expansion with the model's candidates, backup) -- with the policy network called in between.  The semantics, the two
deliberate deviations (a terminal leaf inside the horizon is worth 0 instead of raising; a runaway descent is cut at
``max_depth``) and the layout are those of the header.

    forest = SearchForest(B, S, T, k=8, max_actions=8, device="cuda")
    states, policy, rewards, lengths = actor_prediction(model_policy(model), start, 8, n_sim=16, n_bar=100, n_logits=3)

``policy(frames, scalars, games)`` is any callable returning ``(tokens int8 (b,k,3S), prior float32 (b,k) or None,
q float32 (b,))`` for the rows ``games`` (int64 game indices) of the model input.  The first call of a simulation
covers all B games (rows of games that need no expansion are ignored), so that no host sync is needed to find the
games that do; games whose candidates were all dropped are asked again, alone, with ``forest.attempt`` counting.

A policy with the attribute ``takes_flags = True`` (``FusedAlphaTensor.policy(seed, masked=True)``) is called as
``policy(frames, scalars, games, flags=forest.flags, need=bits, out=(tokens, q))`` instead, always on all B rows with
``games = arange(B)``: it evaluates the rows whose flags hold every bit of ``need`` (EXPAND | PENDING on the first call
of a simulation, RETRY on a retry), writes their rows of ``out`` (int8 (B,k,3S), float32 (B,)) in place and returns
``(tokens, None, q)`` with those two buffers.  The mask is applied on the device, so the rows nobody reads (finished
games, games out of simulations, terminal leaves, leaves past the horizon) cost nothing.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from . import ops
from ._lib import (TG_SEARCH_EXPAND, TG_SEARCH_HORIZON, TG_SEARCH_MAX_ACTIONS, TG_SEARCH_MAX_DEPTH, TG_SEARCH_MAX_K,
                   TG_SEARCH_MAX_T, TG_SEARCH_PENDING, TG_SEARCH_RETRY, TG_SEARCH_TERMINAL, SearchForestDesc,
                   TensorGameError)

__all__ = ["SearchForest", "actor_prediction", "model_policy", "keyed_policy", "EXPAND", "TERMINAL", "HORIZON", "RETRY",
           "PENDING"]

EXPAND, TERMINAL, HORIZON, RETRY, PENDING = (TG_SEARCH_EXPAND, TG_SEARCH_TERMINAL, TG_SEARCH_HORIZON, TG_SEARCH_RETRY,
                                             TG_SEARCH_PENDING)

Policy = Callable[[torch.Tensor, torch.Tensor, torch.Tensor], Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]]


def frame_bytes(S: int) -> int:
    return (S ** 3 + 15) // 16 * 16


class SearchForest:
    """B search trees of ``max_nodes`` nodes each, plus the per-game root, move counter and trajectory.

    ``max_nodes`` defaults to ``n_sim * max_actions + 1`` when ``n_sim`` is given (a simulation creates at most one
    node); the index gets the next power of two >= 2 * max_nodes slots.  ``prior=True`` keeps a prior per child and
    selects by PUCT (``commit(..., prior=...)``)."""

    def __init__(self, B: int, S: int, T: int = 1, k: int = 8, max_actions: int = 8, max_nodes: Optional[int] = None,
                 n_sim: Optional[int] = None, horizon: int = 5, max_depth: Optional[int] = None,
                 index_capacity: Optional[int] = None, prior: bool = False, shift: int = 1, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TensorGameError("SearchForest", -1, "a ROCm device is required; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not (1 <= k <= TG_SEARCH_MAX_K and 1 <= T <= TG_SEARCH_MAX_T and 1 <= max_actions <= TG_SEARCH_MAX_ACTIONS):
            raise TensorGameError("SearchForest", -1, f"need 1 <= k <= {TG_SEARCH_MAX_K}, 1 <= T <= {TG_SEARCH_MAX_T}, "
                                  f"1 <= max_actions <= {TG_SEARCH_MAX_ACTIONS}")
        if max_nodes is None:
            if n_sim is None:
                raise TensorGameError("SearchForest", -1, "give max_nodes or n_sim")
            max_nodes = n_sim * max_actions + 1
        if max_depth is None:
            max_depth = min(TG_SEARCH_MAX_DEPTH, max(64, max_nodes + 1))
        if index_capacity is None:
            index_capacity = 1 << max(6, (2 * max_nodes - 1).bit_length())
        self.B, self.S, self.T, self.k, self.M = B, S, T, k, max_nodes
        self.max_actions, self.horizon, self.max_depth, self.shift = max_actions, horizon, max_depth, shift
        FB = frame_bytes(S)
        dev, i8, i32, i64, f32, u8 = self.device, torch.int8, torch.int32, torch.int64, torch.float32, torch.uint8
        M = max_nodes

        def z(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=dev)

        self.node_key = z((B, M), i64)
        self.node_frames = z((B, M, T, FB), i8)
        self.node_nchild = z((B, M), i32)
        self.child_tokens = z((B, M, k, 3 * S), i8)
        self.child_key = z((B, M, k), i64)
        self.child_n = z((B, M, k), f32)
        self.child_q = z((B, M, k), f32)
        self.child_prior = z((B, M, k), f32) if prior else None
        self.index_key = z((B, index_capacity), i64)
        self.index_node = z((B, index_capacity), i32)
        self.node_count = z((B,), i32)
        self.root_frames = z((B, T, FB), i8)
        self.root_key = z((B,), i64)
        self.move = z((B,), i32)
        self.done = z((B,), u8)
        self.sims_left = z((B,), i32)
        self.status = z((B,), i32)
        self.overflow = z((B,), u8)
        self.leaf_frames = z((B, T, FB), i8)
        self.leaf_key = z((B,), i64)
        self.path_node = z((B, max_depth), i32)
        self.path_slot = z((B, max_depth), i32)
        self.depth = z((B,), i32)
        self.flags = z((B,), u8)
        self.attempt = z((B,), i32)
        self.traj_frames = z((B, max_actions, T, FB), i8)
        self.traj_node = torch.full((B, max_actions), -1, dtype=i32, device=dev)
        self.traj_choice = torch.full((B, max_actions), -1, dtype=i32, device=dev)
        # model-input buffers of select, reused (rows of games not selected keep their old, finite values)
        self._model_in = {}
        self.scalars = z((B, 1), f32)
        self.desc = SearchForestDesc(B=B, S=S, T=T, k=k, M=M, index_capacity=index_capacity, max_actions=max_actions,
                                     horizon=horizon, max_depth=max_depth, shift=shift)
        for name, _ in SearchForestDesc._fields_[10:]:
            t = getattr(self, name)
            setattr(self.desc, name, None if t is None else t.data_ptr())

    @property
    def index_capacity(self) -> int:
        return self.index_key.shape[1]

    # ---- the four calls ------------------------------------------------------------------------------------------
    def reset(self, states: torch.Tensor, n_sim: int) -> None:
        """Roots <- states (int8 (B,T,S,S,S), frame 0 = head); every tree emptied; n_sim simulations for move 0."""
        ops.search_reset(self, states, n_sim)

    def select(self, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
        """One descent per active game.  Returns the model input (B,T,S,S,S) of ``dtype`` and scalars (B,1) (views of
        buffers the next ``select`` overwrites); ``flags``, ``leaf_key``, ``depth``, ``path_*`` are updated."""
        if dtype not in self._model_in:
            self._model_in[dtype] = torch.zeros((self.B, self.T, self.S, self.S, self.S), dtype=dtype, device=self.device)
        ops.search_select(self, self._model_in[dtype], self.scalars)
        return self._model_in[dtype], self.scalars

    def commit(self, tokens, q, prior=None, mask=None) -> None:
        """Expansion + backup of the selected games (tokens int8 (B,k,3S), q float32 (B,), prior float32 (B,k))."""
        ops.search_commit(self, tokens, q, prior, mask)

    def advance(self, n_sim: int) -> None:
        """End the move: the root's argmax-Q child becomes the root."""
        ops.search_advance(self, n_sim)

    def policy(self, n_logits: int, n_bar: int) -> torch.Tensor:
        """Improved policy float32 (B, max_actions, 3S, n_logits) of every move played (zero rows elsewhere)."""
        return ops.search_policy(self, n_logits, n_bar)

    # ---- the driver ----------------------------------------------------------------------------------------------
    def play(self, policy: Policy, states: torch.Tensor, n_sim: int, dtype=torch.float32, max_retries: int = 256) -> None:
        """Play every game to the end (``actor_prediction``'s loop, act.py:34-52, for B games at once).  One host sync per
        simulation (retry count and whether any game still has simulations left) and one per move."""
        self.reset(states, n_sim)
        B, k, S = self.B, self.k, self.S
        games = torch.arange(B, device=self.device)
        tokens_all = torch.zeros((B, k, 3 * S), dtype=torch.int8, device=self.device)
        q_all = torch.zeros((B,), dtype=torch.float32, device=self.device)
        prior_all = torch.zeros((B, k), dtype=torch.float32, device=self.device) if self.child_prior is not None else None
        masked = bool(getattr(policy, "takes_flags", False))

        def ask(need):  # the masked policy writes the rows it evaluates straight into tokens_all / q_all
            tokens, _, q = policy(frames, scalars, games, flags=self.flags, need=need, out=(tokens_all, q_all))
            if tokens is not tokens_all or q is not q_all:
                raise TensorGameError("policy", -1, "a policy with takes_flags returns the tokens and q buffers of `out`")

        for _ in range(self.max_actions):
            for _ in range(n_sim):
                frames, scalars = self.select(dtype)
                if masked:
                    ask(EXPAND | PENDING)
                    self.commit(tokens_all, q_all, prior_all)
                else:
                    tokens, prior, q = policy(frames, scalars, games)
                    self.commit(*self._full(tokens, prior, q, games, tokens_all, prior_all, q_all))
                for attempt in range(max_retries + 1):
                    retry = (self.flags & RETRY) != 0
                    n_retry, n_active = torch.stack([retry.sum(), ((self.sims_left > 0) & (self.done == 0)).sum()]).tolist()
                    if n_retry == 0:
                        break
                    if attempt == max_retries:
                        raise TensorGameError("SearchForest.play", -1, f"{n_retry} games found no surviving candidate "
                                              f"after {max_retries} retries")
                    if masked:
                        ask(RETRY)
                        self.commit(tokens_all, q_all, prior_all, mask=retry.to(torch.uint8))
                        continue
                    sel = retry.nonzero()[:, 0]
                    tokens, prior, q = policy(frames[sel], scalars[sel], sel)
                    self.commit(*self._full(tokens, prior, q, sel, tokens_all, prior_all, q_all),
                                mask=retry.to(torch.uint8))
                if n_active == 0:
                    break
            self.advance(n_sim)
            if bool(self.done.all()):
                break

    def _full(self, tokens, prior, q, rows, tokens_all, prior_all, q_all):
        b = rows.shape[0]
        tokens = torch.as_tensor(tokens, device=self.device)
        if tokens.dtype != torch.int8:
            tokens = tokens.to(torch.int8)
        if tuple(tokens.shape) != (b, self.k, 3 * self.S):
            raise TensorGameError("policy", -1, f"tokens must be (b,k,3S) = {(b, self.k, 3 * self.S)}, got {tuple(tokens.shape)}")
        q = torch.as_tensor(q, device=self.device).to(torch.float32).reshape(b)
        if b == self.B:
            tokens_all.copy_(tokens)
            q_all.copy_(q)
        else:
            tokens_all[rows] = tokens
            q_all[rows] = q
        if prior_all is not None:
            if prior is None:
                prior_all[rows] = 0.0
            else:
                prior_all[rows] = torch.as_tensor(prior, device=self.device).to(torch.float32).reshape(b, self.k)
        return tokens_all, q_all, prior_all

    # ---- results -------------------------------------------------------------------------------------------------
    def lengths(self) -> torch.Tensor:
        """int64 (B,): moves played per game."""
        return self.move.to(torch.int64)

    def states(self) -> torch.Tensor:
        """int8 (B, max_actions, T, S, S, S): the root at the start of each move played, zero after the last."""
        N = self.S ** 3
        st = self.traj_frames[..., :N].reshape(self.B, self.max_actions, self.T, self.S, self.S, self.S)
        played = torch.arange(self.max_actions, device=self.device)[None, :] < self.move[:, None]
        return st * played[:, :, None, None, None, None].to(torch.int8)

    def final_heads(self) -> torch.Tensor:
        """int8 (B,S,S,S): the head of the state after the last move (the root now)."""
        return self.root_frames[:, 0, :self.S ** 3].reshape(self.B, self.S, self.S, self.S).contiguous()

    def root_stats(self):
        """(N, Q float32 (B, max_actions, k), n_children int32 (B, max_actions), choice int32 (B, max_actions)): the root
        node's visit counts and Q values of every move played (NaN-free zeros beyond n_children / the last move)."""
        node = self.traj_node.clamp(min=0).to(torch.int64)
        played = self.traj_node >= 0
        gi = torch.arange(self.B, device=self.device)[:, None]
        n = self.child_n[gi, node] * played[..., None]
        q = self.child_q[gi, node] * played[..., None]
        nc = self.node_nchild[gi, node] * played
        slot = torch.arange(self.k, device=self.device)
        live = slot[None, None, :] < nc[..., None]
        return n * live, q * live, nc, self.traj_choice


def rewards_of(lengths: torch.Tensor, final_rank: torch.Tensor, max_actions: int) -> torch.Tensor:
    """int64 (B, max_actions): cumsum([-1]*(L-1) + [-1 - rank(final)]) per game (act.py:53-57), zero past L."""
    m = torch.arange(max_actions, device=lengths.device)[None, :]
    L = lengths[:, None]
    r = -(m + 1) - torch.where(m == L - 1, final_rank[:, None].to(torch.int64), torch.zeros_like(m))
    return torch.where(m < L, r, torch.zeros_like(r))


def actor_prediction(policy: Policy, initial_states: torch.Tensor, max_actions: int, n_sim: int, n_bar: int,
                     n_logits: int, horizon: int = 5, k: int = 8, max_nodes: Optional[int] = None, prior: bool = False,
                     dtype=torch.float32, max_retries: int = 256, forest: Optional[SearchForest] = None):
    """B self-play games at once: ``actor_prediction`` (act.py:8-64) with the tree of each game on the device.

    initial_states: int8 (B,T,S,S,S) on the device (frame 0 = head).  Returns
    ``states`` int8 (B,L,T,S,S,S), ``policy`` float32 (B,L,3S,n_logits), ``rewards`` int64 (B,L) and ``lengths``
    int64 (B,), L = max_actions; entries past a game's length are zero.  ``forest`` (optional) is used instead of a
    new one (it must match the shapes)."""
    if initial_states.dim() != 5:
        raise TensorGameError("actor_prediction", -1, "initial_states must be int8 (B,T,S,S,S)")
    B, T, S = initial_states.shape[0], initial_states.shape[1], initial_states.shape[2]
    if forest is None:
        forest = SearchForest(B, S, T, k=k, max_actions=max_actions, max_nodes=max_nodes, n_sim=n_sim, horizon=horizon,
                              prior=prior, device=initial_states.device)
    forest.play(policy, initial_states, n_sim, dtype=dtype, max_retries=max_retries)
    pol = forest.policy(n_logits, n_bar)
    lengths = forest.lengths()
    rank = ops.slice_rank(forest.final_heads())
    return forest.states(), pol, rewards_of(lengths, rank, max_actions), lengths


def model_policy(model) -> Policy:
    """Wrap an ``AlphaTensor``-like model (``fwd_infer(states, scalars) -> (tokens, probs, q)``, model.py:347-356): its
    ``n_samples`` candidate actions are the k of the search."""

    @torch.no_grad()
    def policy(frames, scalars, games):
        aa, _, qq = model.fwd_infer(frames, scalars)
        return aa.to(torch.int8), None, qq.reshape(frames.shape[0], -1)[:, 0].float()

    return policy


# ---- a deterministic stand-in for the network (tests, benchmarks) -------------------------------------------------
_M64 = (1 << 64) - 1


def _s64(x: int) -> int:
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


_C1, _C2, _C3, _C4 = (_s64(c) for c in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93))


def _lsr(x: torch.Tensor, s: int) -> torch.Tensor:
    return (x >> s) & ((1 << (64 - s)) - 1)


def _mix(x: torch.Tensor) -> torch.Tensor:
    """splitmix64's finaliser on int64 tensors (wrapping arithmetic, logical shifts)."""
    x = (x ^ _lsr(x, 30)) * _C2
    x = (x ^ _lsr(x, 27)) * _C3
    return x ^ _lsr(x, 31)


def keyed_policy(forest: SearchForest, pool: torch.Tensor, seed: int = 0, p_pool: float = 0.75) -> Policy:
    """A network stand-in computed on the device: the candidates and q of a leaf are a function of (leaf key, attempt,
    seed) only.  Candidate j is a row of ``pool`` (int8 (P,3S) tokens, shift 1) with probability ``p_pool`` on the first
    attempt, otherwise uniform tokens in {0,1,2}; q is uniform in [-1,1) on a 2^-23 grid.  tests/search_ref.py restates
    it on the host."""
    pool = pool.to(forest.device, torch.int8)
    P, L = pool.shape[0], 3 * forest.S
    thr = int(p_pool * (1 << 24))
    j = torch.arange(forest.k, device=forest.device, dtype=torch.int64)
    t = torch.arange(L, device=forest.device, dtype=torch.int64)

    def policy(frames, scalars, games):
        key = forest.leaf_key[games]
        att = forest.attempt[games].to(torch.int64)
        h = _mix(key ^ _mix(att * _C1 + seed))                                      # (b,)
        hj = _mix(h[:, None] + (j[None, :] + 1) * _C4)                              # (b,k)
        from_pool = (_lsr(hj, 40) < thr) & (att[:, None] == 0)
        pick = _lsr(_mix(hj + _C1), 33) % P
        rand = (_lsr(_mix(hj[:, :, None] + (t[None, None, :] + 1) * _C2), 40) % 3).to(torch.int8)
        tokens = torch.where(from_pool[:, :, None], pool[pick], rand)
        q = _lsr(_mix(h + _C3), 40).to(torch.float32) * (2.0 ** -23) - 1.0
        return tokens, None, q

    return policy
