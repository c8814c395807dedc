"""Host side of the fused network tests (include/tensor_game_net.h, mat_mul_amd.net):

* ``CONFIGS`` and ``make_weights(config, seed)``: every state_dict entry of a reference ``AlphaTensor`` of that
  configuration, drawn from ``numpy.random.default_rng(seed)`` (weights uniform +-1/sqrt(fan_in), non-zero biases,
  LayerNorm weights 1 +- noise, ``pos_enc_fix`` random too so that its packing is checked);
* a float64 torch restatement of the eval-mode forward, written from the network's math (``ee``, teacher-forced
  logits, ``zz0``, value quantiles, the risk-managed value);
* the host sampling rule of the header (Philox uniforms from oracle.tensor_game, cumulative sums, the running product).
"""
import math

import numpy as np
import torch

from oracle import tensor_game as O

# reference constructor arguments; n_layers (when given) is shared by the torso and the policy head, as the reference
# passes its kwargs to both
CONFIGS = {
    "a": dict(dim_3d=4, dim_t=2, dim_s=1, dim_c=8, n_steps=12, n_logits=3, n_samples=8, n_feats=8, n_heads=4,
              n_hidden=128),
    "b": dict(dim_3d=3, dim_t=1, dim_s=1, dim_c=16, n_steps=9, n_logits=3, n_samples=4, n_feats=16, n_heads=2,
              n_hidden=64, n_layers=3),
    "c": dict(dim_3d=5, dim_t=1, dim_s=1, dim_c=16, n_steps=15, n_logits=3, n_samples=8, n_feats=16, n_heads=4,
              n_hidden=64),
}
D_HEAD, MLP_W, N_QUANTILE = 32, 4, 8  # the reference's MultiHeadAttention / ValueHead defaults
P = "policy_head.predict_action_logits."


FIELDS = ("S", "T", "dim_s", "c", "torso_layers", "torso_heads", "torso_d", "torso_ff", "W", "heads", "d", "ff",
          "blocks", "n_steps", "n_logits", "n_hidden", "n_quantile")  # tg_net_config's, in its order


def dims(cfg):
    """The fused configuration (include/tensor_game_net.h field names) of a configuration: reference constructor kwargs
    (``d``, ``w`` and ``n_quantile`` optional: the first two reach the torso's attention only, as in the reference; the
    policy keeps D_HEAD and MLP_W), or the fused dims themselves (every field of FIELDS)."""
    if "S" in cfg:
        return {k: int(cfg[k]) for k in FIELDS}
    W = cfg["n_feats"] * cfg["n_heads"]
    return dict(S=cfg["dim_3d"], T=cfg["dim_t"], dim_s=cfg["dim_s"], c=cfg["dim_c"],
                torso_layers=cfg.get("n_layers", 8), torso_heads=cfg["n_heads"], torso_d=cfg.get("d", D_HEAD),
                torso_ff=cfg.get("w", MLP_W) * cfg["dim_c"], W=W, heads=cfg["n_heads"], d=D_HEAD, ff=MLP_W * W,
                blocks=cfg.get("n_layers", 2), n_steps=cfg["n_steps"], n_logits=cfg["n_logits"],
                n_hidden=cfg["n_hidden"], n_quantile=cfg.get("n_quantile", N_QUANTILE))


def make_weights(cfg, seed):
    """state_dict (name -> float32 numpy array) of a reference AlphaTensor with configuration ``cfg`` (either form of
    ``dims``)."""
    rng = np.random.default_rng(seed)
    m = dims(cfg)
    sd = {}

    def lin(name, fin, fout, bias=True):
        a = 1.0 / math.sqrt(fin)
        sd[name + ".weight"] = rng.uniform(-a, a, (fout, fin))
        if bias:
            sd[name + ".bias"] = rng.uniform(-a, a, fout)

    def ln(name, n):
        sd[name + ".weight"] = 1.0 + rng.uniform(-0.2, 0.2, n)
        sd[name + ".bias"] = rng.uniform(-0.2, 0.2, n)

    def mha(p, c1, c2, H, d, ff):
        ln(p + "ln1", c1)
        ln(p + "ln2", c2)
        for h in range(H):
            lin(f"{p}heads.{h}.query", c1, d, bias=False)
            lin(f"{p}heads.{h}.key", c2, d, bias=False)
            lin(f"{p}heads.{h}.value", c2, d, bias=False)
        lin(p + "li1", H * d, c1)
        ln(p + "ln3", c1)
        lin(p + "li2", c1, ff)
        lin(p + "li3", ff, c1)

    S, T, c, W = m["S"], m["T"], m["c"], m["W"]
    for i in range(3):
        lin(f"torso.li1.{i}", m["dim_s"], S * S)
    for i in range(3):
        lin(f"torso.li2.{i}", S * T + 1, c)
    for l in range(m["torso_layers"]):
        mha(f"torso.blocks.{l}.mha.", c, c, m["torso_heads"], m["torso_d"], m["torso_ff"])
    sd[P + "emb1.weight"] = rng.normal(0.0, 1.0, (m["n_logits"] + 1, W))
    sd[P + "pos_enc"] = rng.uniform(0.0, 1.0, (m["n_steps"], W))
    sd[P + "pos_enc_fix"] = rng.uniform(-1.0, 1.0, (m["n_steps"], W))
    for b in range(m["blocks"]):
        p = f"{P}blocks.{b}."
        ln(p + "ln1", W)
        mha(p + "att1.", W, W, m["heads"], m["d"], m["ff"])
        ln(p + "ln2", W)
        mha(p + "att2.", W, c, m["heads"], m["d"], m["ff"])
    lin(P + "li1", W, m["n_logits"])
    nh = m["n_hidden"]
    lin("value_head.mlp.0", W, nh)
    lin("value_head.mlp.2", nh, nh)
    lin("value_head.mlp.4", nh, nh)
    lin("value_head.mlp.6", nh, m["n_quantile"])
    return {k: v.astype(np.float32) for k, v in sd.items()}


def make_inputs(cfg, n, seed):
    """n states with entries in {-2..2} (int8 (n,T,S,S,S)) and their scalars float32 (n,dim_s)."""
    rng = np.random.default_rng(seed)
    m = dims(cfg)
    S, T = m["S"], m["T"]
    xx = rng.integers(-2, 3, size=(n, T, S, S, S)).astype(np.int8)
    ss = rng.integers(0, 12, size=(n, m["dim_s"])).astype(np.float32)
    return xx, ss


# ---- float64 restatement ---------------------------------------------------------------------------------------------
class Ref:
    """The eval-mode forward in float64 torch on ``device``, from a state_dict (numpy or torch values) and its
    configuration in either form of ``dims``.  ``dtype`` float32 gives the eager stand-in of tools/net_bench.py."""

    def __init__(self, sd, cfg, device="cpu", dtype=torch.float64):
        self.w = {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in sd.items()}
        self.m = dims(cfg)
        self.device, self.dtype = device, dtype

    def _ln(self, x, p):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-5) * self.w[p + ".weight"] + self.w[p + ".bias"]

    def _lin(self, x, p):
        y = x @ self.w[p + ".weight"].T
        return y + self.w[p + ".bias"] if p + ".bias" in self.w else y

    def _attn(self, p, x, y, H, causal):
        """Pre-LN attention block: x + li1(heads) then + li3(gelu(li2(ln3(.))))."""
        xn, yn = self._ln(x, p + "ln1"), self._ln(y, p + "ln2")
        outs = []
        for h in range(H):
            q = xn @ self.w[f"{p}heads.{h}.query.weight"].T
            k = yn @ self.w[f"{p}heads.{h}.key.weight"].T
            v = yn @ self.w[f"{p}heads.{h}.value.weight"].T
            s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
            if causal:
                n = s.shape[-1]
                s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
            outs.append(torch.softmax(s, -1) @ v)
        h1 = x + self._lin(torch.cat(outs, -1), p + "li1")
        f = self._lin(self._ln(h1, p + "ln3"), p + "li2")
        return h1 + self._lin(0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0))), p + "li3")

    def torso(self, xx, ss):
        """ee float64 (B,3S^2,c): row i*3S + m*S + j holds grid m at (i, j)."""
        m = self.m
        S, T = m["S"], m["T"]
        x = torch.as_tensor(xx, device=self.device).to(self.dtype)   # [b][t][a0][a1][a2]
        s = torch.as_tensor(ss, device=self.device).to(self.dtype)
        B = x.shape[0]
        # grid m, row (p, q), channel c3*T + t: (a0,a1,a2) = (p,q,c3), (q,c3,p), (c3,p,q)
        src = [x.permute(0, 2, 3, 4, 1), x.permute(0, 4, 2, 3, 1), x.permute(0, 3, 4, 2, 1)]
        g = []
        for i in range(3):
            proj = self._lin(s, f"torso.li1.{i}").reshape(B, S, S, 1)
            inp = torch.cat([src[i].reshape(B, S, S, S * T), proj], -1)
            g.append(self._lin(inp, f"torso.li2.{i}"))
        for l in range(m["torso_layers"]):
            for m1, m2 in ((0, 1), (1, 2), (2, 0)):
                y = self._attn(f"torso.blocks.{l}.mha.", *(2 * [torch.cat([g[m1], g[m2]], 2)]),
                               H=m["torso_heads"], causal=False)
                g[m1], g[m2] = y[:, :, :S], y[:, :, S:]
        return torch.stack(g, 2).reshape(B, 3 * S * S, m["c"])

    def decode(self, ee, tokens_in):
        """(logits (N,n,n_logits), xx (N,n,W)) for input token rows tokens_in int (N,n) (START = n_logits first)."""
        m = self.m
        n = tokens_in.shape[1]
        x = self.w[P + "emb1.weight"][tokens_in] + self.w[P + "pos_enc"][:n] + self.w[P + "pos_enc_fix"][:n]
        for b in range(m["blocks"]):
            p = f"{P}blocks.{b}."
            xb = self._ln(x, p + "ln1")
            x = xb + self._attn(p + "att1.", xb, xb, m["heads"], causal=True)
            xb = self._ln(x, p + "ln2")
            x = xb + self._attn(p + "att2.", xb, ee, m["heads"], causal=False)
        return self._lin(torch.relu(x), P + "li1"), x

    def value(self, z):
        h = z
        for i in (0, 2, 4):
            h = torch.relu(self._lin(h, f"value_head.mlp.{i}"))
        return self._lin(h, "value_head.mlp.6")

    @staticmethod
    def risk(q):
        jj = math.ceil(0.75 * q.shape[-1]) - 1
        return q[:, jj:].mean(-1)

    def fwd_infer(self, xx, ss, k):
        """AlphaTensor.fwd_infer's op structure (the whole prefix rerun at every step, torch's Categorical draws):
        aa (B,k,n_steps), pp (B,k), qq (B,)."""
        m = self.m
        ee = self.torso(xx, ss)
        B = ee.shape[0]
        ee = ee.unsqueeze(1).repeat(1, k, 1, 1).reshape(B * k, *ee.shape[1:])
        aa = torch.full((B * k, m["n_steps"] + 1), m["n_logits"], dtype=torch.long, device=self.device)
        pp = torch.ones(B * k, dtype=self.dtype, device=self.device)
        for i in range(m["n_steps"]):
            oo, xo = self.decode(ee, aa[:, :i + 1])
            dist = torch.distributions.Categorical(logits=oo[:, i])
            aa[:, i + 1] = dist.sample()
            pp = pp * dist.probs.gather(1, aa[:, i + 1:i + 2])[:, 0]
        qq = self.risk(self.value(xo[:, 0].reshape(B, k, -1).mean(1)))
        return aa[:, 1:].reshape(B, k, -1), pp.reshape(B, k), qq

    def teacher(self, ee, g_action):
        """(oo, zz0, q): PolicyHead.fwd_train's forward on g_action (B,n_steps) and the value head on zz0."""
        g = torch.as_tensor(np.asarray(g_action), device=self.device).long()
        start = torch.full((g.shape[0], 1), self.m["n_logits"], dtype=torch.long, device=self.device)
        oo, xx = self.decode(ee, torch.cat([start, g[:, :-1]], 1))
        return oo, xx[:, 0], self.value(xx[:, 0])


# ---- the sampling rule -------------------------------------------------------------------------------------------------
def philox_uniforms(seed, rows, call, k, n_steps):
    """float64 (B,k,n_steps) uniforms of the header's rule: word t%4 of philox4x32_10((row, call, s, t//4), seed)."""
    rows = np.asarray(rows, np.int64)
    B, nb = rows.shape[0], (n_steps + 3) // 4
    ctr = np.zeros((B, k, nb, 4), np.uint32)
    ctr[..., 0] = (rows & 0xFFFFFFFF).astype(np.uint32)[:, None, None]
    ctr[..., 1] = np.uint32(call & 0xFFFFFFFF)
    ctr[..., 2] = np.arange(k, dtype=np.uint32)[None, :, None]
    ctr[..., 3] = np.arange(nb, dtype=np.uint32)[None, None, :]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    w = O.philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    w = w.reshape(B, k, nb * 4)[:, :, :n_steps]
    return (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def pick(u, probs):
    """Token of the rule for uniforms u (...,) and probabilities (..., n_logits), and the distance of u to the nearest
    cumulative boundary."""
    c = np.cumsum(np.asarray(probs, np.float64), -1)
    below = u[..., None] < c
    tok = np.where(below.any(-1), below.argmax(-1), probs.shape[-1] - 1)
    dist = np.abs(u[..., None] - c[..., :-1]).min(-1) if probs.shape[-1] > 1 else np.full(u.shape, np.inf)
    return tok, dist
