"""Host side of the training tests (include/tensor_game_train.h, mat_mul_amd.train):

* ``TrainRef``: ``net_ref.Ref`` with explicit dropout masks on att1's and att2's outputs, the two losses of
  ``AlphaTensor.fwd_train`` (the policy cross entropy summed, the quantile loss averaged) and their gradient by torch
  autograd, in float64 (or float32 for the eager stand-in of tools/train_bench.py);
* ``keep_mask``: the header's dropout keep rule restated on the host (Philox from oracle.tensor_game);
* ``make_batch``: states, scalars, actions and rewards for a configuration; ``two_sided_rewards`` and
  ``two_sided_batch``: rewards on both sides of the random networks' quantiles, inside and outside the Huber kink;
  ``bad_tokens``: a batch's actions with out-of-range entries and the rows that hold them;
* ``value_branches``: how a batch's (game, quantile) pairs fall on the quantile loss's four branches;
* ``err`` and ``within``: the suite's per-tensor bound; ``compare_grads``: losses and every gradient tensor under it;
* ``GuardedCall``: a trainer's loss entry with the workspace and every output between guard bytes.
"""
import numpy as np
import torch

import guarded_buffers as G
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

    def forward(self, xx, ss, g_action, masks=None):
        """(logits (B,n_steps,n_logits), value quantiles (B,n_quantile)) of the teacher-forced decoder on START followed
        by g_action shifted by one; an input token outside [0, n_logits) reads as START."""
        g = torch.as_tensor(g_action, device=self.device).long()
        if masks is not None:
            masks = torch.as_tensor(masks, device=self.device).to(self.dtype)
        ee = self.torso(xx, ss)
        NL = self.m["n_logits"]
        start = torch.full((g.shape[0], 1), NL, dtype=torch.long, device=self.device)
        tin = torch.cat([start, g[:, :-1]], 1)
        tin = torch.where((tin >= 0) & (tin <= NL), tin, torch.full_like(tin, NL))
        oo, x = self.decode_masked(ee, tin, masks)
        return oo, self.value(x[:, 0])

    def losses(self, xx, ss, g_action, g_value, masks=None, skip_rows=None):
        """(l_pol, l_val) of AlphaTensor.fwd_train for g_action int (B,n_steps), g_value (B,1).  The rows of skip_rows
        (bool (B,), the header's rows with a token outside [0, n_logits)) add nothing to l_pol and count in l_val."""
        g = torch.as_tensor(g_action, device=self.device).long()
        gv = torch.as_tensor(g_value, device=self.device).to(self.dtype).reshape(-1, 1)
        oo, q = self.forward(xx, ss, g_action, masks)
        NL = self.m["n_logits"]
        if skip_rows is None:
            l_pol = torch.nn.functional.cross_entropy(oo.reshape(-1, NL), g.reshape(-1), reduction="sum")
        else:
            skip = torch.as_tensor(np.asarray(skip_rows, bool), device=self.device)
            tgt = torch.where(skip[:, None], torch.zeros_like(g), g)  # a skipped row's targets are never used
            ce = torch.nn.functional.cross_entropy(oo.reshape(-1, NL), tgt.reshape(-1), reduction="none")
            l_pol = (ce.reshape(g.shape) * (~skip)[:, None].to(self.dtype)).sum()
        return l_pol, self.quantile_loss(q, gv)

    def quantile_loss(self, q, gv):
        """The reference's quantile_loss of quantiles q (B,n_quantile) against gv (B,1): the mean of huber(gv - q_j) *
        |tau_j - 1[gv - q_j > 0]|."""
        n = q.shape[-1]
        # the quantile levels and their weights in float32, as the reference's quantile_loss forms them (exact when n
        # is a power of two)
        tau = (torch.arange(n, dtype=torch.float32, device=self.device) + 0.5) / n
        dd = gv - q
        ad = dd.abs()
        hh = torch.where(ad < 1.0, 0.5 * dd * dd, ad - 0.5)
        kk = (tau - (dd > 0).float()).abs().to(self.dtype)
        return (hh * kk).mean()

    def loss_grad(self, xx, ss, g_action, g_value, masks=None, weight_pol=1.0, weight_val=1000.0, skip_rows=None):
        """(l_pol, l_val, {name: gradient of weight_pol * l_pol + weight_val * l_val}) as float64 numpy values."""
        for v in self.w.values():
            v.grad = None
        l_pol, l_val = self.losses(xx, ss, g_action, g_value, masks, skip_rows)
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


def two_sided_rewards(B, seed):
    """float32 rewards (B,1) uniform in [-1.5, 1.5]: on both sides of the random networks' quantiles (about +-0.2), and
    on both sides of the Huber kink |g_value - q| = 1."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, size=(B, 1)).astype(np.float32)


def two_sided_batch(cfg, B, seed):
    """make_batch(cfg, B, seed) with two_sided_rewards(B, seed) in place of its integer rewards."""
    xx, ss, aa, _ = make_batch(cfg, B, seed)
    return xx, ss, aa, two_sided_rewards(B, seed)


def bad_tokens(aa, n_logits):
    """(actions, skip_rows) for int8 actions aa (B >= 300, n_steps): n_logits at position 0 of row 5, 127 at the last
    position of row 6 (never a decoder input; rows 5 and 6 share a partial slab at B = 300), -128 mid-row in row 200
    and -1 in row 299."""
    bad = aa.copy()
    n = aa.shape[1]
    bad[5, 0] = n_logits
    bad[6, n - 1] = 127
    bad[200, n // 2] = -128
    bad[299, min(1, n - 1)] = -1
    skip = np.zeros(aa.shape[0], bool)
    skip[[5, 6, 200, 299]] = True
    return bad, skip


def value_branches(ref, xx, ss, g_action, g_value):
    """Of d = g_value - q over the B * n_quantile pairs of ``ref`` (a float64 TrainRef): the shares of the four classes
    {quadratic |d| < 1, linear} x {d > 0, d <= 0} as a dict, and the distance of the nearest pair to a branch change,
    min(min |d|, min ||d| - 1|)."""
    with torch.no_grad():
        _, q = ref.forward(xx, ss, g_action)
    d = (torch.as_tensor(g_value, device=q.device).to(q.dtype).reshape(-1, 1) - q).cpu().numpy()
    quad, pos = np.abs(d) < 1.0, d > 0
    shares = {("quad", "pos"): float((quad & pos).mean()), ("quad", "neg"): float((quad & ~pos).mean()),
              ("lin", "pos"): float((~quad & pos).mean()), ("lin", "neg"): float((~quad & ~pos).mean())}
    return shares, float(min(np.abs(d).min(), np.abs(np.abs(d) - 1.0).min()))


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))


def err(got, ref):
    """max |got - ref|."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    return float(np.abs(got - ref).max())


def bound(tol, ref):
    """The suite's bound of a tensor: tol * max(1, max |ref|)."""
    return tol * max(1.0, float(np.abs(ref).max()))


def within(e, tol, ref, f32_err, what):
    """e <= tol * max(1, max |ref|), or, where the eager float32 restatement's error f32_err() misses that bound too,
    e <= twice that error."""
    b = bound(tol, ref)
    if e <= b:
        return True
    e32 = f32_err()
    if e32 < b:
        return False
    print(f"FAMILY-F32-BOUND {what}: error {e:.3g}, eager float32 {e32:.3g} >= {b:.3g}")
    return e <= 2.0 * e32


def compare_grads(tag, what, got, ref, ref32, tol):
    """got = (l_pol, l_val, {name: gradient}) of the fused kernels against ref, the same of a float64 TrainRef, under the
    suite's bound (``within``, with ref32, the same of a float32 TrainRef, as the eager float32 restatement).  Prints
    ``tag what fused .. eager32 ..``: the worst error of a tensor over that tensor's own max |ref| (no floor of 1)."""
    assert sorted(ref[2]) == sorted(got[2])
    pairs = [("l_pol", got[0], ref[0], ref32[0]), ("l_val", got[1], ref[1], ref32[1])]
    pairs += [(k, got[2][k], g, ref32[2][k]) for k, g in ref[2].items()]
    bad, own, own32 = {}, 0.0, 0.0
    for key, value, want, want32 in pairs:
        e, e32 = err(value, want), err(want32, want)
        top = float(np.abs(want).max())
        if top > 0.0:
            own, own32 = max(own, e / top), max(own32, e32 / top)
        if not within(e, tol, want, lambda: e32, f"{what} {key}"):
            bad[key] = e
    print(f"{tag} {what} fused {own:.3g} eager32 {own32:.3g}")
    assert not bad, bad


class GuardedCall:
    """The loss entry of a trainer (FusedTrainer: ops.net_loss_grad, SlicedTrainer: ops.net_loss_grad_sliced) on the
    trainer's weights with the workspace, grad, losses, status and keep_out each between guard bytes (guarded_buffers);
    the workspace defaults to exactly the entry's workspace size for the batch, filled with ``fill`` bytes.  Dropout
    0.5 with the internal keep rule (seed 3, call 4)."""

    def __init__(self, tr, batch, ws=None, fill=0):
        self.tr, self.batch, m = tr, batch, tr.config
        b = batch[0].shape[0]
        self.bufs = {}
        if ws is None:
            ws = self.guarded("workspace", (tr._workspace_size(tr.c, b),), torch.uint8)
            ws.fill_(fill)
        self.ws = ws
        self.grad = self.guarded("grad", tuple(tr.params.shape), torch.float32)
        self.losses = self.guarded("losses", (2,), torch.float32)
        self.status = self.guarded("status", (1,), torch.int32)
        self.keep = self.guarded("keep_out", (b, m["blocks"], 2, m["n_steps"], m["W"]), torch.uint8)

    def guarded(self, what, shape, dtype):
        self.bufs[what], t = G.guarded(shape, dtype)
        return t

    def run(self, grad=True):
        """(grad or None, losses) of one call; the outputs start as NaN."""
        self.grad.fill_(float("nan"))
        self.losses.fill_(float("nan"))
        tr = self.tr
        tr._loss_grad(tr.c, tr.params.detach(), tr.pos_fix, *self.batch, self.ws, grad=self.grad if grad else None,
                      losses=self.losses, status=self.status, dropout_p=0.5, seed=3, call_idx=4, keep_out=self.keep)
        torch.cuda.synchronize()
        for what, buf in self.bufs.items():
            G.check_flat(buf, what)
        assert int(self.status[0]) == 0 and torch.isfinite(self.losses).all()
        assert not grad or torch.isfinite(self.grad).all()
        return self.grad.clone() if grad else None, self.losses.clone()


__all__ = ["TrainRef", "keep_mask", "multipliers", "make_batch", "two_sided_rewards", "two_sided_batch", "bad_tokens",
           "value_branches", "rel_err", "err", "bound", "within", "compare_grads", "GuardedCall"]
