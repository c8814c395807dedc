#!/usr/bin/env python3
"""Golden fixture of the training loss and gradient (include/tensor_game_train.h, mat_mul_amd.train), recorded by
RUNNING THE REFERENCE's own ``AlphaTensor`` (/root/reference/model.py) in train mode with dropout_p = 0, in float64,
with the weights of tests/net_ref.make_weights.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train.py      (build container only)

Per configuration <c> of net_ref.CONFIGS, for B_CASE states with actions and rewards (train_ref.make_batch(cfg, B_CASE,
<c>_seed + 300)):
  <c>_seed int64: make_weights' seed;  <c>_keys bytes (n,): the state_dict's names in the model's order;
  <c>_l_pol, <c>_l_val float64: AlphaTensor.fwd_train's two losses;
  <c>_gnorm (n,), <c>_gdot (n,2) float64: per state_dict tensor, the gradient of 1 * l_pol + 1000 * l_val: its norm and
      its dot products with two +-1 vectors (signs(seed, key index) below; buffers have no gradient: 0);
  <c>_g_<name> float64: the full gradient of the small tensors (FULL below);
  <c>_adam_loss float64 (3,): the combined loss before each of three torch.optim.AdamW(lr=1e-3) steps on the batch;
  <c>_pnorm (n,), <c>_pdot (n,2) float64: the parameters after the three steps, projected the same way;
  <c>_p_<name> float64: the small tensors after the three steps.
The archive is written deterministically (write_npz of make_golden_net.py).  Nothing of the reference is copied.
"""
import copy
import sys
from pathlib import Path

import numpy as np

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
OUT = HERE / "train_cases.npz"
SEEDS = {"a": 21, "b": 22, "c": 23}
B_CASE = 4
LR = 1e-3
P = "policy_head.predict_action_logits."
FULL = ["value_head.mlp.6.weight", "value_head.mlp.6.bias", P + "li1.weight", P + "li1.bias", P + "emb1.weight",
        P + "pos_enc"] + [f"torso.li1.{i}.{w}" for i in range(3) for w in ("weight", "bias")]


def signs(seed, index, shape):
    """Two +-1 arrays of ``shape`` for state_dict entry ``index``."""
    rng = np.random.default_rng([seed, index])
    return rng.integers(0, 2, size=(2,) + tuple(shape)).astype(np.float64) * 2.0 - 1.0


def project(seed, keys, values):
    norm = np.zeros(len(keys))
    dot = np.zeros((len(keys), 2))
    for i, k in enumerate(keys):
        v = values.get(k)
        if v is None:
            continue
        v = np.asarray(v, np.float64)
        s = signs(seed, i, v.shape)
        norm[i] = np.sqrt((v * v).sum())
        dot[i] = [(s[0] * v).sum(), (s[1] * v).sum()]
    return norm, dot


def record(torch, model_mod, name, cfg):
    import net_ref
    import train_ref

    seed = SEEDS[name]
    sd = net_ref.make_weights(cfg, seed)
    model = model_mod.AlphaTensor(**cfg, dropout_p=0.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = copy.deepcopy(model).double()
    model.train()
    keys = list(model.state_dict().keys())
    xx, ss, aa, rr = train_ref.make_batch(cfg, B_CASE, seed + 300)
    x, s = torch.from_numpy(xx).double(), torch.from_numpy(ss).double()
    a, r = torch.from_numpy(aa).long(), torch.from_numpy(rr).double()
    out = {f"{name}_seed": np.int64(seed), f"{name}_keys": np.array(keys, dtype=bytes)}
    l_pol, l_val = model.fwd_train(x, s, a, r)
    model.zero_grad()
    (1.0 * l_pol + 1000.0 * l_val).backward()
    grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    out[f"{name}_l_pol"] = np.float64(l_pol.item())
    out[f"{name}_l_val"] = np.float64(l_val.item())
    out[f"{name}_gnorm"], out[f"{name}_gdot"] = project(seed, keys, grads)
    for k in FULL:
        out[f"{name}_g_{k}"] = grads[k]
    opt = torch.optim.AdamW(model.parameters(), lr=LR)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        l_pol, l_val = model.fwd_train(x, s, a, r)
        loss = 1.0 * l_pol + 1000.0 * l_val
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out[f"{name}_adam_loss"] = np.array(losses)
    params = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out[f"{name}_pnorm"], out[f"{name}_pdot"] = project(seed, keys, params)
    for k in FULL:
        out[f"{name}_p_{k}"] = params[k]
    return out


def main(out_path=OUT):
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    sys.path.insert(0, REF)
    import torch

    import model as model_mod  # noqa: E402  (reference)
    import net_ref
    from make_golden_net import write_npz

    torch.set_num_threads(1)  # a fixed summation order
    arrays = {}
    for name, cfg in net_ref.CONFIGS.items():
        arrays.update(record(torch, model_mod, name, cfg))
    write_npz(out_path, arrays)
    print(f"wrote {out_path} ({Path(out_path).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
