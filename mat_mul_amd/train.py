"""Training of the AlphaTensor network on the device (include/tensor_game_train.h).

The reference's ``train_step`` (training.py:419-445) runs ``model.fwd_train`` in train mode, ``loss.backward()`` and
``AdamW.step()`` on its own copy of the weights, several thousand small kernels per batch; the search then needs those
weights re-packed.  Here the loss and its gradient are four launches (``tg_net_loss_grad``) on one flat parameter
vector in the blob layout, so any torch optimizer updates it in place and the inference blob is refreshed from it by one
add into the pos slot:

    tr = FusedTrainer.from_model(model)                          # or from_state_dict(sd, dropout_p=...)
    opt = torch.optim.AdamW([tr.params], lr=1e-4)
    for batch in data.batches(256):                              # TensorGameData: (state, scalar, action, reward)
        l_pol, l_val = tr.train_step(batch, opt)                 # device tensors, no host sync
    states, policy, rewards, lengths = search.actor_prediction(tr.net().policy(seed), start, ...)
    model.load_state_dict(tr.state_dict())                       # reference-format weights

Dropout follows the header's keep rule (Philox keyed by the trainer's seed, counter (row, call, block, position)), not
torch's generator: the distribution is the reference's, the individual masks are not.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import TensorGameError
from .net import _P, CONFIG_FIELDS, FusedAlphaTensor, FusedAlphaTensor25, check_config, infer_config, pack_weights

__all__ = ["FusedTrainer", "SlicedTrainer", "SlicedTrainer25", "unpack_weights", "blob_layout"]


def _mha_layout(p: str, c1: int, c2: int, H: int, d: int, ff: int, out: list) -> None:
    hd = H * d
    out += [(p + "ln1.weight", (c1,), "id"), (p + "ln1.bias", (c1,), "id"), (p + "ln2.weight", (c2,), "id"),
            (p + "ln2.bias", (c2,), "id"), (p + "heads.{h}.query.weight", (c1, hd), "headsT"),
            (p + "heads.{h}.key.weight", (hd, c2), "heads"), (p + "heads.{h}.value.weight", (c2, hd), "headsT"),
            (p + "li1.weight", (hd, c1), "T"), (p + "li1.bias", (c1,), "id"), (p + "ln3.weight", (c1,), "id"),
            (p + "ln3.bias", (c1,), "id"), (p + "li2.weight", (c1, ff), "T"), (p + "li2.bias", (ff,), "id"),
            (p + "li3.weight", (ff, c1), "T"), (p + "li3.bias", (c1,), "id")]


def blob_layout(cfg: Mapping[str, int]) -> List[Tuple[str, Tuple[int, ...], str, int]]:
    """(state_dict name, stored shape, kind, float offset) of every slot of the blob, in order.  kind: "id" (as torch
    holds it), "T" (a Linear weight, transposed), "heads" (the heads' weights stacked on rows; ``{h}`` in the name),
    "headsT" (stacked, then transposed), "pos" (pos_enc, plus pos_enc_fix in the inference blob)."""
    c = cfg
    S2, cin = c["S"] * c["S"], c["S"] * c["T"] + 1
    items: list = []
    for i in range(3):
        items += [(f"torso.li1.{i}.weight", (c["dim_s"], S2), "T"), (f"torso.li1.{i}.bias", (S2,), "id")]
    for i in range(3):
        items += [(f"torso.li2.{i}.weight", (cin, c["c"]), "T"), (f"torso.li2.{i}.bias", (c["c"],), "id")]
    for l in range(c["torso_layers"]):
        _mha_layout(f"torso.blocks.{l}.mha.", c["c"], c["c"], c["torso_heads"], c["torso_d"], c["torso_ff"], items)
    W = c["W"]
    items += [(_P + "emb1.weight", (c["n_logits"] + 1, W), "id"), (_P + "pos_enc", (c["n_steps"], W), "pos")]
    for b in range(c["blocks"]):
        p = f"{_P}blocks.{b}."
        items += [(p + "ln1.weight", (W,), "id"), (p + "ln1.bias", (W,), "id")]
        _mha_layout(p + "att1.", W, W, c["heads"], c["d"], c["ff"], items)
        items += [(p + "ln2.weight", (W,), "id"), (p + "ln2.bias", (W,), "id")]
        _mha_layout(p + "att2.", W, c["c"], c["heads"], c["d"], c["ff"], items)
    items += [(_P + "li1.weight", (W, c["n_logits"]), "T"), (_P + "li1.bias", (c["n_logits"],), "id")]
    fin = W
    for i, fout in ((0, c["n_hidden"]), (2, c["n_hidden"]), (4, c["n_hidden"]), (6, c["n_quantile"])):
        items += [(f"value_head.mlp.{i}.weight", (fin, fout), "T"), (f"value_head.mlp.{i}.bias", (fout,), "id")]
        fin = fout
    out, off = [], 0
    for name, shape, kind in items:
        out.append((name, shape, kind, off))
        off += int(np.prod(shape))
    return out


def unpack_weights(blob, cfg: Mapping[str, int], pos_fix, folded: bool = False) -> Dict[str, torch.Tensor]:
    """The inverse of ``pack_weights``: a reference-format state_dict (float32 CPU tensors) that a reference
    ``AlphaTensor`` of ``cfg`` loads with ``load_state_dict(strict=True)``.  ``blob`` is the training parameter vector
    (pos slot = pos_enc; exact inverse of ``pack_weights(sd, cfg, fold_pos=False)``), or with ``folded`` the inference
    blob (pos_enc = slot - pos_fix, rounded once).  ``pos_fix`` becomes pos_enc_fix."""
    if isinstance(blob, torch.Tensor):
        blob = blob.detach().to("cpu")
    v = np.asarray(blob, dtype=np.float32).reshape(-1)
    fix = np.asarray(pos_fix.detach().cpu() if isinstance(pos_fix, torch.Tensor) else pos_fix, np.float32)
    lay = blob_layout(cfg)
    name, shape, kind, off = lay[-1]
    if v.size != off + int(np.prod(shape)):
        raise TensorGameError("unpack_weights", -1, f"blob of {v.size} floats, the configuration needs "
                              f"{off + int(np.prod(shape))}")
    sd: Dict[str, np.ndarray] = {}
    for name, shape, kind, off in lay:
        a = v[off:off + int(np.prod(shape))].reshape(shape)
        if kind == "T":
            sd[name] = a.T
        elif kind == "pos":
            sd[name] = (a.astype(np.float64) - fix.astype(np.float64)).astype(np.float32) if folded else a
            sd[_P + "pos_enc_fix"] = fix.reshape(shape)
        elif kind in ("heads", "headsT"):
            rows = a.T if kind == "headsT" else a
            H = cfg["torso_heads"] if name.startswith("torso.") else cfg["heads"]
            d = rows.shape[0] // H
            for h in range(H):
                sd[name.format(h=h)] = rows[h * d:(h + 1) * d]
        else:
            sd[name] = a
    return {k: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for k, x in sd.items()}


class FusedTrainer:
    """The training step of a reference ``AlphaTensor`` on one flat float32 parameter vector on the device."""

    # the library entries a trainer calls (a subclass names others): the family check, the workspace size, the loss
    _check = staticmethod(ops.net_train_check)
    _workspace_size = staticmethod(ops.net_train_workspace_size)
    _loss_grad = staticmethod(ops.net_loss_grad)
    # the inference family's check, the blob's size and the inference class of net()
    _net_check = staticmethod(ops.net_check)
    _weights_size = staticmethod(ops.net_weights_size)
    _net = FusedAlphaTensor

    def __init__(self, cfg: Mapping[str, int], theta: torch.Tensor, pos_fix: torch.Tensor, dropout_p: float = 0.5,
                 weight_pol: float = 1.0, weight_val: float = 1000.0, n_samples: int = 4, seed: int = 0):
        self.config = {k: int(cfg[k]) for k in CONFIG_FIELDS}
        self.c = check_config(self.config, self._net_check)
        self._check(self.c)
        n = self._weights_size(self.c)
        if theta.numel() != n or theta.dtype != torch.float32 or not theta.is_cuda:
            raise TensorGameError("FusedTrainer", -1, f"theta must be {n} float32 on a ROCm device, got {theta.dtype} "
                                  f"{tuple(theta.shape)} on {theta.device}")
        if not 0.0 <= float(dropout_p) < 1.0:
            raise TensorGameError("FusedTrainer", -1, f"dropout_p={dropout_p} outside [0, 1)")
        self.device = theta.device
        self.params = torch.nn.Parameter(theta.detach().clone().reshape(-1))
        self.params.grad = torch.zeros_like(self.params)
        self.pos_fix = pos_fix.to(self.device, torch.float32).reshape(self.config["n_steps"], self.config["W"]).contiguous()
        self.dropout_p, self.weight_pol, self.weight_val = float(dropout_p), float(weight_pol), float(weight_val)
        self.n_samples, self.seed = int(n_samples), int(seed)
        self.calls = 0  # the `call` counter of the keep rule; advanced by every train-mode call
        pos = next(e for e in blob_layout(self.config) if e[2] == "pos")
        self._pos = slice(pos[3], pos[3] + self.pos_fix.numel())
        self._blob = torch.empty_like(self.params.detach())
        self._ws: Dict[int, torch.Tensor] = {}
        self._losses = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.refresh()

    @classmethod
    def from_state_dict(cls, sd: Mapping, dropout_p: float = 0.5, weight_pol: float = 1.0, weight_val: float = 1000.0,
                        n_samples: int = 4, seed: int = 0, device="cuda") -> "FusedTrainer":
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError("FusedTrainer", -1, "a ROCm device is required; there is no CPU path")
        cfg = infer_config(sd)
        check_config(cfg, cls._net_check)
        theta = torch.from_numpy(pack_weights(sd, cfg, fold_pos=False)).to(dev)
        fix = torch.as_tensor(np.asarray(sd[_P + "pos_enc_fix"].detach().cpu() if isinstance(
            sd[_P + "pos_enc_fix"], torch.Tensor) else sd[_P + "pos_enc_fix"], np.float32))
        return cls(cfg, theta, fix, dropout_p, weight_pol, weight_val, n_samples, seed)

    @classmethod
    def from_model(cls, model, weight_pol: float = 1.0, weight_val: float = 1000.0, seed: int = 0,
                   device=None) -> "FusedTrainer":
        """Weights, n_samples and the PredictBlock dropout of a reference ``AlphaTensor``."""
        if device is None:
            device = model.device if model.device.type == "cuda" else "cuda"
        p = model.policy_head.predict_action_logits.blocks[0].dropout1.p
        return cls.from_state_dict(model.state_dict(), p, weight_pol, weight_val, model.n_samples, seed, device)

    # ---- the loss -------------------------------------------------------------------------------------------------
    def workspace(self, B: int) -> torch.Tensor:
        ws = self._ws.get(B)
        if ws is None:
            self._ws = {B: torch.empty(self._workspace_size(self.c, B), dtype=torch.uint8, device=self.device)}
            ws = self._ws[B]
        return ws

    def _inputs(self, state, scalar, action, reward):
        dev = self.device
        state = state.to(dev)
        if state.dtype not in (torch.int8, torch.float32):
            state = state.to(torch.float32)
        B = state.shape[0]
        return (state.contiguous(), scalar.to(dev, torch.float32).reshape(B, -1).contiguous(),
                action.to(dev).to(torch.int8).contiguous(), reward.to(dev, torch.float32).reshape(B, 1).contiguous())

    def _call(self, grad, dropout_p, state, scalar, action, reward, keep_in=None, keep_out=None):
        state, scalar, action, reward = self._inputs(state, scalar, action, reward)
        call = self.calls
        if dropout_p > 0 or keep_in is not None:
            self.calls += 1
        losses = torch.empty(2, dtype=torch.float32, device=self.device)
        self._loss_grad(self.c, self.params.detach(), self.pos_fix, state, scalar, action, reward,
                        self.workspace(state.shape[0]), grad=grad, losses=losses, status=self.status,
                        weight_pol=self.weight_pol, weight_val=self.weight_val, dropout_p=dropout_p, seed=self.seed,
                        call_idx=call, keep_in=keep_in, keep_out=keep_out)
        return losses[0], losses[1]

    def loss_and_grad(self, state, scalar, action, reward, keep_in=None, keep_out=None):
        """``model.fwd_train`` in train mode and the backward of weight_pol * l_pol + weight_val * l_val: writes
        ``params.grad`` and returns (l_pol, l_val) as device scalars.  No host sync."""
        if self.params.grad is None:
            self.params.grad = torch.zeros_like(self.params)
        return self._call(self.params.grad, self.dropout_p, state, scalar, action, reward, keep_in, keep_out)

    @torch.no_grad()
    def losses(self, state, scalar, action, reward):
        """(l_pol, l_val) in eval mode, no gradient: the body of the reference's ``val_step``."""
        return self._call(None, 0.0, state, scalar, action, reward)

    def train_step(self, batch, optimizer):
        """One batch of the reference's ``train_step``: the loss and gradient, ``optimizer.step()``, then the inference
        blob refresh.  Returns (l_pol, l_val) as device scalars."""
        state, scalar, action, reward = batch
        l_pol, l_val = self.loss_and_grad(state, scalar, action, reward)
        optimizer.step()
        self.refresh()
        return l_pol, l_val

    # ---- the weights ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self) -> None:
        """The inference blob := params with pos_enc_fix added into the pos slot (on the device)."""
        self._blob.copy_(self.params.detach())
        self._blob[self._pos] += self.pos_fix.reshape(-1)

    def net(self, n_samples: Optional[int] = None) -> FusedAlphaTensor:
        """A ``FusedAlphaTensor`` on the trainer's inference blob (shared: every train_step updates it)."""
        return self._net(self.config, self._blob, n_samples or self.n_samples)

    def checkpoint(self) -> dict:
        """Everything a resumed trainer needs, as host tensors and plain scalars (``torch.save`` it; it loads with
        ``weights_only=True``): the configuration, ``params`` (the training vector, bit for bit), ``pos_fix``, the
        dropout probability, both loss weights, ``n_samples``, the dropout ``seed`` and the ``calls`` counter that keys
        the next mask.  A host copy."""
        return {"config": dict(self.config), "params": self.params.detach().cpu(), "pos_fix": self.pos_fix.cpu(),
                "dropout_p": self.dropout_p, "weight_pol": self.weight_pol, "weight_val": self.weight_val,
                "n_samples": self.n_samples, "seed": self.seed, "calls": self.calls}

    @classmethod
    def from_checkpoint(cls, d: Mapping, device="cuda") -> "FusedTrainer":
        """The trainer ``checkpoint`` described, on ``device``: its next ``train_step`` is the one the saved trainer
        would have made."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise TensorGameError("FusedTrainer", -1, "a ROCm device is required; there is no CPU path")
        tr = cls(d["config"], d["params"].to(dev), d["pos_fix"], d["dropout_p"], d["weight_pol"], d["weight_val"],
                 d["n_samples"], d["seed"])
        tr.calls = int(d["calls"])
        return tr

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference-format weights (float32 CPU tensors; a host copy)."""
        return unpack_weights(self.params.detach(), self.config, self.pos_fix)


class SlicedTrainer(FusedTrainer):
    """``FusedTrainer`` at the 4x4 matmul tensor (dim_3d = 16), the size ``FusedTrainer`` refuses: the same constructor,
    classmethods and methods on include/tensor_game_train_sliced.h's entries (``tg_net_loss_grad_sliced``), which cut
    the torso by slices and the decoder's cross-attention by chunks of positions.  Every other size is refused here."""

    _check = staticmethod(ops.net_train_sliced_check)
    _workspace_size = staticmethod(ops.net_train_sliced_workspace_size)
    _loss_grad = staticmethod(ops.net_loss_grad_sliced)

    def checkpoint(self) -> dict:
        """``FusedTrainer.checkpoint`` with ``"kind": "sliced"``, by which ``replay_io.load_run`` builds this class."""
        return dict(super().checkpoint(), kind="sliced")


class SlicedTrainer25(FusedTrainer):
    """``FusedTrainer`` at the 5x5 matmul tensor (dim_3d = 25), the size ``FusedTrainer`` and ``SlicedTrainer`` refuse:
    the same constructor, classmethods and methods on include/tensor_game_train_s25.h's entries
    (``tg_net_loss_grad_s25``), which cut the torso by slices and both attention blocks of the decoder by chunks of
    positions.  ``net()`` is a ``FusedAlphaTensor25``.  Every other size is refused here."""

    _check = staticmethod(ops.net_train_s25_check)
    _workspace_size = staticmethod(ops.net_train_s25_workspace_size)
    _loss_grad = staticmethod(ops.net_loss_grad_s25)
    _net_check = staticmethod(ops.net_s25_check)
    _weights_size = staticmethod(ops.net_s25_weights_size)
    _net = FusedAlphaTensor25

    def checkpoint(self) -> dict:
        """``FusedTrainer.checkpoint`` with ``"kind": "sliced25"``, by which ``replay_io.load_run`` builds this class."""
        return dict(super().checkpoint(), kind="sliced25")
