"""Fused eval-mode inference of the AlphaTensor network (include/tensor_game_net.h).

The reference's ``AlphaTensor.fwd_infer`` (model.py:347-356) runs about 4 000 small torch ops per call: the torso, then
a policy head that reruns the whole prefix at each of the n_steps token steps, then the value head.  Here the same
eval-mode forward is two launches -- ``tg_net_torso`` and ``tg_net_sample`` (decoder with a cache, sampling and value
head) -- from one packed float32 weight blob.

    net = FusedAlphaTensor.from_model(model)              # or from_state_dict(sd, n_samples)
    aa, pp, qq = net.fwd_infer(xx, ss, seed=0)              # int64 (B,k,n_steps), float32 (B,k), float32 (B,)
    oo, zz0 = net.logits(xx, ss, g_action)                  # teacher-forced, PolicyHead.fwd_train's forward
    states, policy, rewards, lengths = search.actor_prediction(net.policy(seed=0), start, 8, n_sim=16, ...)

Supported: dim_3d <= 5, or exactly 9 (3x3 matmul) or 16 (4x4 matmul, n_steps <= 48: the torso then runs one
workgroup per (game, slice) instead of one per game, and training goes through ``train.SlicedTrainer``), inside the TG_NET_MAX_* bounds and the LDS plans of the
header; ``check_config`` names the bound otherwise.  The 5x5 matmul tensor, dim_3d = 25 (n_steps <= 75), has a class
of its own, ``FusedAlphaTensor25``, on the entries of include/tensor_game_net_s25.h (the decoder keeps one normalised
copy of the torso output for all policy blocks there); it takes that size only, and training there goes through
``train.SlicedTrainer25``.

The draws follow the header's sampling rule (Philox keyed by seed, counter (game, call, sample, step block)), not
torch's generator: the distribution is the reference's, the individual draws are not.  There is no CPU path.
"""
from __future__ import annotations

import re
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import TG_NET_MAX_SAMPLES, NetConfig, TensorGameError

__all__ = ["FusedAlphaTensor", "FusedAlphaTensor25", "infer_config", "check_config", "pack_weights", "CONFIG_FIELDS"]

CONFIG_FIELDS = tuple(name for name, _ in NetConfig._fields_)

_P = "policy_head.predict_action_logits."


def _np64(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().to("cpu", torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def _count(sd: Mapping, pattern: str) -> int:
    rx = re.compile(pattern)
    return len({m.group(1) for k in sd for m in [rx.fullmatch(k)] if m})


def infer_config(sd: Mapping) -> Dict[str, int]:
    """The dimensions of the network a reference ``AlphaTensor`` state_dict holds (shapes and block counts)."""
    try:
        S2, dim_s = sd["torso.li1.0.weight"].shape
        c, cin = sd["torso.li2.0.weight"].shape
        S = int(round(S2 ** 0.5))
        if S * S != S2 or (cin - 1) % S:
            raise TensorGameError("infer_config", -1, f"torso shapes {S2}x{dim_s}, {c}x{cin} are not a dim_3d grid")
        torso_d = sd["torso.blocks.0.mha.heads.0.query.weight"].shape[0]
        nl1, W = sd[_P + "emb1.weight"].shape
        n_steps = sd[_P + "pos_enc"].shape[0]
        d = sd[_P + "blocks.0.att1.heads.0.query.weight"].shape[0]
        cfg = dict(
            S=S, T=(cin - 1) // S, dim_s=dim_s, c=c,
            torso_layers=_count(sd, r"torso\.blocks\.(\d+)\.mha\.ln1\.weight"),
            torso_heads=_count(sd, r"torso\.blocks\.0\.mha\.heads\.(\d+)\.query\.weight"), torso_d=torso_d,
            torso_ff=sd["torso.blocks.0.mha.li2.weight"].shape[0],
            W=W, heads=_count(sd, re.escape(_P) + r"blocks\.0\.att1\.heads\.(\d+)\.query\.weight"), d=d,
            ff=sd[_P + "blocks.0.att1.li2.weight"].shape[0],
            blocks=_count(sd, re.escape(_P) + r"blocks\.(\d+)\.ln1\.weight"),
            n_steps=n_steps, n_logits=nl1 - 1, n_hidden=sd["value_head.mlp.0.weight"].shape[0],
            n_quantile=sd["value_head.mlp.6.weight"].shape[0])
    except KeyError as e:
        raise TensorGameError("infer_config", -1, f"not an AlphaTensor state_dict: missing {e}") from None
    cfg = {k: int(v) for k, v in cfg.items()}
    heads2 = _count(sd, re.escape(_P) + r"blocks\.0\.att2\.heads\.(\d+)\.query\.weight")
    if heads2 != cfg["heads"] or sd[_P + "blocks.0.att2.li2.weight"].shape[0] != cfg["ff"]:
        raise TensorGameError("infer_config", -1, "the cross-attention's heads or MLP width differ from the "
                              "self-attention's")
    return cfg


def check_config(cfg: Mapping[str, int], check=ops.net_check) -> NetConfig:
    """The C struct of ``cfg``; raises TensorGameError naming the bound unless tg_net_check (or the ``check`` of another
    header's family) accepts it."""
    c = NetConfig(**{k: int(cfg[k]) for k in CONFIG_FIELDS})
    check(c)
    return c


def _mha(sd: Mapping, p: str, H: int, out: list) -> None:
    """One MultiHeadAttention in the blob's order (Linear weights transposed; keys as torch holds them)."""
    g = lambda n: _np64(sd[p + n])  # noqa: E731
    out += [g("ln1.weight"), g("ln1.bias"), g("ln2.weight"), g("ln2.bias")]
    out.append(np.concatenate([g(f"heads.{h}.query.weight") for h in range(H)], axis=0).T)
    out.append(np.concatenate([g(f"heads.{h}.key.weight") for h in range(H)], axis=0))
    out.append(np.concatenate([g(f"heads.{h}.value.weight") for h in range(H)], axis=0).T)
    out += [g("li1.weight").T, g("li1.bias"), g("ln3.weight"), g("ln3.bias"), g("li2.weight").T, g("li2.bias"),
            g("li3.weight").T, g("li3.bias")]


def pack_weights(sd: Mapping, cfg: Mapping[str, int], fold_pos: bool = True) -> np.ndarray:
    """The float32 weight blob of include/tensor_game_net.h.  The one folding (pos_enc + pos_enc_fix) is done in
    float64 and rounded once.  ``fold_pos=False`` packs the training parameter vector of include/tensor_game_train.h
    instead, whose pos slot holds pos_enc alone."""
    g = lambda n: _np64(sd[n])  # noqa: E731
    parts: list = []
    for i in range(3):
        parts += [g(f"torso.li1.{i}.weight").T, g(f"torso.li1.{i}.bias")]
    for i in range(3):
        parts += [g(f"torso.li2.{i}.weight").T, g(f"torso.li2.{i}.bias")]
    for l in range(cfg["torso_layers"]):
        _mha(sd, f"torso.blocks.{l}.mha.", cfg["torso_heads"], parts)
    parts += [g(_P + "emb1.weight"), g(_P + "pos_enc") + g(_P + "pos_enc_fix") if fold_pos else g(_P + "pos_enc")]
    for b in range(cfg["blocks"]):
        p = f"{_P}blocks.{b}."
        parts += [g(p + "ln1.weight"), g(p + "ln1.bias")]
        _mha(sd, p + "att1.", cfg["heads"], parts)
        parts += [g(p + "ln2.weight"), g(p + "ln2.bias")]
        _mha(sd, p + "att2.", cfg["heads"], parts)
    parts += [g(_P + "li1.weight").T, g(_P + "li1.bias")]
    for i in (0, 2, 4, 6):
        parts += [g(f"value_head.mlp.{i}.weight").T, g(f"value_head.mlp.{i}.bias")]
    return np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in parts]).astype(np.float32)


class FusedAlphaTensor:
    """Eval-mode inference of a reference ``AlphaTensor`` from its weights, packed once on the device."""

    # the library entries (include/tensor_game_net.h); a subclass names another header's
    _check = staticmethod(ops.net_check)
    _weights_size = staticmethod(ops.net_weights_size)
    _torso = staticmethod(ops.net_torso)
    _sample = staticmethod(ops.net_sample)
    _logits = staticmethod(ops.net_logits)

    def __init__(self, cfg: Mapping[str, int], blob: torch.Tensor, n_samples: int):
        if not 1 <= n_samples <= TG_NET_MAX_SAMPLES:
            raise TensorGameError("FusedAlphaTensor", -1, f"n_samples={n_samples} outside [1, {TG_NET_MAX_SAMPLES}]")
        self.config = {k: int(cfg[k]) for k in CONFIG_FIELDS}
        self.c = check_config(self.config, self._check)
        if blob.numel() != self._weights_size(self.c):
            raise TensorGameError("FusedAlphaTensor", -1, f"blob of {blob.numel()} floats, the configuration needs "
                                  f"{self._weights_size(self.c)}")
        self.w = blob
        self.device = blob.device
        self.n_samples = int(n_samples)
        self.n_steps, self.n_logits = self.config["n_steps"], self.config["n_logits"]
        self.calls = 0  # the `call` counter of the random stream; advanced by every sampling call

    @classmethod
    def from_state_dict(cls, sd: Mapping, n_samples: int, device="cuda") -> "FusedAlphaTensor":
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError("FusedAlphaTensor", -1, "a ROCm device is required; there is no CPU path")
        cfg = infer_config(sd)
        check_config(cfg, cls._check)
        return cls(cfg, torch.from_numpy(pack_weights(sd, cfg)).to(dev), n_samples)

    @classmethod
    def from_model(cls, model, device=None) -> "FusedAlphaTensor":
        if device is None:
            device = model.device if model.device.type == "cuda" else "cuda"
        return cls.from_state_dict(model.state_dict(), model.n_samples, device)

    # ---- forward pieces -------------------------------------------------------------------------------------------
    def torso(self, xx: torch.Tensor, ss: torch.Tensor, out: Optional[torch.Tensor] = None,
              flags: Optional[torch.Tensor] = None, need: int = 0) -> torch.Tensor:
        """Torso.forward: xx (B,T,S,S,S) float32 or int8, ss float32 (B,dim_s) -> ee float32 (B,3S^2,c).  One launch at
        every supported S (by slices at S = 16 and 25).  ``flags`` uint8 (B,) / ``need``: only the rows with
        ``(flags & need) == need`` are computed; the others of ``out`` are left as they are (zeros without ``out``)."""
        return self._torso(self.c, self.w, xx, ss.to(torch.float32), out=out, flags=flags, need=need)

    def sample(self, ee: torch.Tensor, rows: Optional[torch.Tensor] = None, seed: int = 0, call: Optional[int] = None,
               uniforms: Optional[torch.Tensor] = None, k: Optional[int] = None, tokens: Optional[torch.Tensor] = None,
               probs: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None,
               flags: Optional[torch.Tensor] = None, need: int = 0):
        """The policy and value heads of fwd_infer on ee: tokens int8 (B,k,n_steps), pp float32 (B,k), qq float32 (B,).
        ``rows`` (default 0..B-1) key the random stream; ``call`` defaults to the instance's counter, which every call
        advances.  ``tokens`` / ``probs`` / ``q`` are output buffers; ``flags`` / ``need`` as in ``torso``."""
        B = ee.shape[0]
        if rows is None:
            rows = torch.arange(B, device=self.device, dtype=torch.int64)
        if call is None:
            call = self.calls
        self.calls += 1
        return self._sample(self.c, self.w, ee.contiguous(), rows.to(self.device, torch.int64).contiguous(),
                            k or self.n_samples, seed, call, uniforms=uniforms, tokens=tokens, probs=probs, q=q,
                            flags=flags, need=need)

    @torch.no_grad()
    def fwd_infer(self, xx: torch.Tensor, ss: torch.Tensor, seed: int = 0, call: Optional[int] = None,
                  rows: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """AlphaTensor.fwd_infer in eval mode: aa int64 (B,k,n_steps), pp float32 (B,k), qq float32 (B,)."""
        tokens, pp, qq = self.sample(self.torso(xx, ss), rows, seed, call, uniforms)
        return tokens.to(torch.int64), pp, qq

    @torch.no_grad()
    def logits(self, xx: torch.Tensor, ss: torch.Tensor, g_action: torch.Tensor, with_q: bool = False):
        """The forward of PolicyHead.fwd_train: (oo float32 (B,n_steps,n_logits), zz0 float32 (B,W)), and the value
        head's quantiles q float32 (B,n_quantile) on zz0 when ``with_q``."""
        oo, zz0, q = self._logits(self.c, self.w, self.torso(xx, ss), g_action.to(self.device))
        return (oo, zz0, q) if with_q else (oo, zz0)

    def policy(self, seed: int = 0, masked: bool = False):
        """A ``search.Policy``: candidates (tokens int8 (b,k,3S), None, q (b,)) drawn with the random stream keyed by the
        ``games`` argument.  The policy keeps its own call counter, from 0, and advances it on every call, so a retried
        game draws new candidates and two policies of the same seed replay the same games.

        ``masked=True`` gives a policy with ``takes_flags = True`` instead, which the search driver calls on all B rows
        as ``policy(frames, scalars, games, flags=..., need=..., out=(tokens, q))``: only the rows whose flags hold the
        ``need`` bits are evaluated, their tokens and q written into ``out`` (the other rows of ``out`` keep what they
        held).  Same stream and counter rule, so both kinds of policy play the same games."""
        calls = [0]
        if masked:
            ee = [None]

            @torch.no_grad()
            def masked_policy(frames, scalars, games, flags, need, out):
                B = frames.shape[0]
                if ee[0] is None or ee[0].shape[0] != B:
                    S = self.config["S"]
                    ee[0] = torch.zeros((B, 3 * S * S, self.config["c"]), dtype=torch.float32, device=self.device)
                tokens, q = out
                self.torso(frames, scalars, out=ee[0], flags=flags, need=need)
                self.sample(ee[0], games, seed, call=calls[0], tokens=tokens, q=q, flags=flags, need=need)
                calls[0] += 1
                return tokens, None, q

            masked_policy.takes_flags = True
            return masked_policy

        @torch.no_grad()
        def policy(frames, scalars, games):
            tokens, _, q = self.sample(self.torso(frames, scalars), games, seed, call=calls[0])
            calls[0] += 1
            return tokens, None, q

        return policy

    def rollout_policy(self, seed: int = 0, masked: bool = False):
        """A ``rollout.RolloutPolicy``: ONE action per row (torso on the int8 frames, then ``sample`` with k = 1), drawn
        with the random stream keyed by the global row index -- so the samples of one start state draw differently --
        and ``call`` = the step, so two rollouts of the same seed play the same games.  Two launches, capturable.

        ``masked=True`` gives a policy with ``takes_active = True`` instead, which ``sample_rollouts(stop_solved=True)``
        calls as ``policy(frames, scalars, rows, step, active=..., out=tokens)``: only the rows whose ``active`` byte
        is set are evaluated (``flags=active, need=1`` in both launches) and their tokens written into ``out`` int8
        (B,3S); the other rows of ``out`` keep what they held.  Same stream rule, so an active row draws what the plain
        policy draws for it."""
        if self.n_steps != 3 * self.config["S"]:
            raise TensorGameError("rollout_policy", -1, f"n_steps={self.n_steps} is not 3*dim_3d: the sampled tokens "
                                  "are not one action")
        if masked:
            ee = [None]

            @torch.no_grad()
            def masked_policy(frames, scalars, rows, step, active, out):
                B = frames.shape[0]
                if ee[0] is None or ee[0].shape[0] != B:
                    S = self.config["S"]
                    ee[0] = torch.zeros((B, 3 * S * S, self.config["c"]), dtype=torch.float32, device=self.device)
                self.torso(frames, scalars, out=ee[0], flags=active, need=1)
                self.sample(ee[0], rows, seed, call=step, k=1, tokens=out.view(B, 1, self.n_steps), flags=active, need=1)
                return out

            masked_policy.takes_active = True
            return masked_policy

        @torch.no_grad()
        def policy(frames, scalars, rows, step):
            tokens, _, _ = self.sample(self.torso(frames, scalars), rows, seed, call=step, k=1)
            return tokens.view(frames.shape[0], self.n_steps)

        return policy

    def slot_policy(self, seed: int = 0):
        """The policy of ``rollout.solve_stream`` (``takes_slots = True``, ``seed``): called as ``policy(frames, scalars,
        rows, steps, active=..., uniforms=..., out=tokens)``, it evaluates the rows whose ``active`` byte is set (torso
        and ``sample`` with k = 1, ``flags=active, need=1``) with the given ``uniforms`` float32 (B,1,n_steps) -- which
        ``ops.rollout_refill`` fills by the sampling rule at (row key, call = the row's own step) under ``seed`` -- and
        writes their tokens into ``out`` int8 (B,3S); the other rows of ``out`` keep what they held.  A row so draws
        what ``rollout_policy(seed)`` draws for the row of the same key at the same step.  Two launches, capturable."""
        if self.n_steps != 3 * self.config["S"]:
            raise TensorGameError("slot_policy", -1, f"n_steps={self.n_steps} is not 3*dim_3d: the sampled tokens "
                                  "are not one action")
        ee = [None]

        @torch.no_grad()
        def policy(frames, scalars, rows, steps, active, uniforms, out):
            B = frames.shape[0]
            if ee[0] is None or ee[0].shape[0] != B:
                S = self.config["S"]
                ee[0] = torch.zeros((B, 3 * S * S, self.config["c"]), dtype=torch.float32, device=self.device)
            self.torso(frames, scalars, out=ee[0], flags=active, need=1)
            self.sample(ee[0], rows, seed, call=0, k=1, uniforms=uniforms, tokens=out.view(B, 1, self.n_steps),
                        flags=active, need=1)
            return out

        policy.takes_slots = True
        policy.seed = seed
        return policy


class FusedAlphaTensor25(FusedAlphaTensor):
    """``FusedAlphaTensor`` at the 5x5 matmul tensor, dim_3d = 25 exactly (n_steps <= 75): the same constructor,
    classmethods and methods on include/tensor_game_net_s25.h's entries.  The torso runs one workgroup per (game, slice);
    the decoder keeps one normalised copy of the game's 1875 torso rows for every policy block, which is what lets the
    training app's configuration fit (one sample per workgroup).  Inference only."""

    _check = staticmethod(ops.net_s25_check)
    _weights_size = staticmethod(ops.net_s25_weights_size)
    _torso = staticmethod(ops.net_s25_torso)
    _sample = staticmethod(ops.net_s25_sample)
    _logits = staticmethod(ops.net_s25_logits)
