"""Host side of the training tests (include/tensor_game_train.h, mat_mul_amd.train):

* ``TrainRef``: ``net_ref.Ref`` with explicit dropout masks on att1's and att2's outputs, the two losses of
  ``AlphaTensor.fwd_train`` (the policy cross entropy summed, the quantile loss averaged) and their gradient by torch
  autograd, in float64 (or float32 for the eager stand-in of tools/train_bench.py);
* ``keep_mask``: the header's dropout keep rule restated on the host (Philox from oracle.tensor_game);
* ``make_batch``: states, scalars, actions and rewards for a configuration.
"""
import numpy as np
import torch

from net_ref import P, Ref, dims
from oracle import tensor_game as O


class TrainRef(Ref):
    """The train-mode loss of a reference AlphaTensor, written from the network's math (``cfg`` in either form of
    net_ref.dims).  ``w`` holds leaf tensors that require grad (every state_dict entry but the buffer pos_enc_fix)."""

    def __init__(self, sd, cfg, device="cpu", dtype=torch.float64):
        super().__init__(sd, cfg, device, dtype)
        for k, v in self.w.items():
            if k != P + "pos_enc_fix":
                v.requires_grad_(True)

    def decode_masked(self, ee, tokens_in, masks=None):
        """Ref.decode with dropout multipliers masks (N, blocks, 2, n, W) (keep / (1 - p), or 0) on the blocks."""
        m = self.m
        n = tokens_in.shape[1]
        x = self.w[P + "emb1.weight"][tokens_in] + self.w[P + "pos_enc"][:n] + self.w[P + "pos_enc_fix"][:n]
        for b in range(m["blocks"]):
            p = f"{P}blocks.{b}."
            xb = self._ln(x, p + "ln1")
            c1 = self._attn(p + "att1.", xb, xb, m["heads"], causal=True)
            x = xb + (c1 if masks is None else c1 * masks[:, b, 0])
            xb = self._ln(x, p + "ln2")
            c2 = self._attn(p + "att2.", xb, ee, m["heads"], causal=False)
            x = xb + (c2 if masks is None else c2 * masks[:, b, 1])
        return self._lin(torch.relu(x), P + "li1"), x

    def losses(self, xx, ss, g_action, g_value, masks=None):
        """(l_pol, l_val) of AlphaTensor.fwd_train for g_action int (B,n_steps), g_value (B,1)."""
        g = torch.as_tensor(g_action, device=self.device).long()
        gv = torch.as_tensor(g_value, device=self.device).to(self.dtype).reshape(-1, 1)
        if masks is not None:
            masks = torch.as_tensor(masks, device=self.device).to(self.dtype)
        ee = self.torso(xx, ss)
        start = torch.full((g.shape[0], 1), self.m["n_logits"], dtype=torch.long, device=self.device)
        oo, x = self.decode_masked(ee, torch.cat([start, g[:, :-1]], 1), masks)
        l_pol = torch.nn.functional.cross_entropy(oo.reshape(-1, self.m["n_logits"]), g.reshape(-1), reduction="sum")
        q = self.value(x[:, 0])
        n = q.shape[-1]
        # the quantile levels and their weights in float32, as the reference's quantile_loss forms them (exact when n
        # is a power of two)
        tau = (torch.arange(n, dtype=torch.float32, device=self.device) + 0.5) / n
        dd = gv - q
        ad = dd.abs()
        hh = torch.where(ad < 1.0, 0.5 * dd * dd, ad - 0.5)
        kk = (tau - (dd > 0).float()).abs().to(self.dtype)
        return l_pol, (hh * kk).mean()

    def loss_grad(self, xx, ss, g_action, g_value, masks=None, weight_pol=1.0, weight_val=1000.0):
        """(l_pol, l_val, {name: gradient of weight_pol * l_pol + weight_val * l_val}) as float64 numpy values."""
        for v in self.w.values():
            v.grad = None
        l_pol, l_val = self.losses(xx, ss, g_action, g_value, masks)
        (weight_pol * l_pol + weight_val * l_val).backward()
        grads = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in self.w.items() if v.requires_grad}
        return l_pol.item(), l_val.item(), grads


def keep_mask(seed, call, B, cfg, p):
    """uint8 (B, blocks, 2, n_steps, W) of the header's keep rule: element (r, blk, which, t, i) is kept iff
    (w >> 8) * 2^-24 >= p, w = word i % 4 of philox4x32_10((r, call, blk*2 + which, t*ceil(W/4) + i//4), seed)."""
    m = dims(cfg)
    NB, N, W = m["blocks"], m["n_steps"], m["W"]
    nw4 = (W + 3) // 4
    ctr = np.zeros((B, NB * 2, N, nw4, 4), np.uint32)
    ctr[..., 0] = (np.arange(B, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)[:, None, None, None]
    ctr[..., 1] = np.uint32(call & 0xFFFFFFFF)
    ctr[..., 2] = np.arange(NB * 2, dtype=np.uint32)[None, :, None, None]
    ctr[..., 3] = (np.arange(N, dtype=np.uint32)[:, None] * nw4 + np.arange(nw4, dtype=np.uint32)[None, :])[None, None]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    w = O.philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    w = w.reshape(B, NB * 2, N, nw4 * 4)[..., :W]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8).reshape(B, NB, 2, N, W)


def multipliers(keep, p):
    """The float64 dropout multipliers of a keep mask: keep * float32(1 / (1 - p))."""
    return keep.astype(np.float64) * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def make_batch(cfg, B, seed):
    """int8 states (B,T,S,S,S) in {-2..2}, float32 scalars (B,dim_s), int8 actions (B,n_steps) in [0, n_logits) and
    float32 rewards (B,1) in [-12, 0], for ``cfg`` in either form of net_ref.dims."""
    rng = np.random.default_rng(seed)
    m = dims(cfg)
    S, T = m["S"], m["T"]
    xx = rng.integers(-2, 3, size=(B, T, S, S, S)).astype(np.int8)
    ss = rng.integers(0, 12, size=(B, m["dim_s"])).astype(np.float32)
    aa = rng.integers(0, m["n_logits"], size=(B, m["n_steps"])).astype(np.int8)
    rr = -rng.integers(0, 13, size=(B, 1)).astype(np.float32)
    return xx, ss, aa, rr


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


__all__ = ["TrainRef", "keep_mask", "multipliers", "make_batch", "rel_err"]
