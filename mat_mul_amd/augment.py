"""Symmetry augmentation of training batches (include/tensor_game_symmetry.h).

``Augment`` draws one element of the symmetry group per item -- a permutation of the three modes and a signed
permutation of each mode -- and applies it to the item's frames and action.  The group maps valid items to valid items
with tokens inside the vocabulary, exactly and invertibly, so an augmented batch trains like any other.  The reference
has no counterpart.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import TG_SYM_MODES, TG_SYM_PERMS, TG_SYM_SIGNS, TensorGameError

__all__ = ["Augment"]


class Augment:
    """``aug(state_i8, action_i8, dtype)`` -> (state of ``dtype``, action int8): item n of the call gets the group
    element of the global id ``next_id + n`` under ``seed``, and ``next_id`` advances by the batch, so a run is
    reproducible from ``state_dict()`` whatever its batch sizes.  Two launches (sample, apply), no host sync.

    A sign flip turns a token ``tok`` into ``2*shift - tok``: with ``signs=True`` the vocabulary must be symmetric about
    ``shift``.  Pass the network's ``n_logits`` to have that checked (``n_logits == 2*shift + 1``)."""

    def __init__(self, seed: int, modes: bool = True, perms: bool = True, signs: bool = True, shift: int = 1,
                 n_logits: Optional[int] = None):
        self.seed, self.shift, self.next_id = int(seed), int(shift), 0
        self._S, self._device = None, None
        self.flags = (TG_SYM_MODES if modes else 0) | (TG_SYM_PERMS if perms else 0) | (TG_SYM_SIGNS if signs else 0)
        if signs and n_logits is not None and int(n_logits) != 2 * self.shift + 1:
            raise TensorGameError("Augment", -1, f"signs=True needs n_logits == 2*shift + 1 = {2 * self.shift + 1}, got "
                                  f"{n_logits}: a negated token would leave the vocabulary")

    def sym_for(self, N: int, S: Optional[int] = None, device=None) -> torch.Tensor:
        """The uint8 (N,3S+1) rows the next call on N items would use, ids ``next_id .. next_id + N - 1`` (``next_id``
        stays).  ``S`` and ``device`` default to those of the last call."""
        from . import ops

        S = self._S if S is None else int(S)
        device = self._device if device is None else device
        if S is None or device is None:
            raise TensorGameError("sym_for", -1, "pass S and device before the first call")
        return ops.symmetry_sample(N, S, device, seed=self.seed, item_offset=self.next_id,
                                   modes=bool(self.flags & TG_SYM_MODES), perms=bool(self.flags & TG_SYM_PERMS),
                                   signs=bool(self.flags & TG_SYM_SIGNS))

    def __call__(self, state_i8, action_i8, dtype=torch.float32, overflow=None, status=None):
        from . import ops

        N = state_i8.shape[0]
        self._S, self._device = state_i8.shape[-1], state_i8.device
        sym = self.sym_for(N)
        out = ops.symmetry_apply(state_i8, action_i8, sym, dtype=dtype, shift=self.shift, overflow=overflow, status=status)
        self.next_id += N
        return out

    def state_dict(self) -> dict:
        return {"seed": self.seed, "flags": self.flags, "next_id": self.next_id, "shift": self.shift}

    def load_state_dict(self, d: dict) -> None:
        self.seed, self.flags, self.next_id, self.shift = (int(d[k]) for k in ("seed", "flags", "next_id", "shift"))
