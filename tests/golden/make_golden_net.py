#!/usr/bin/env python3
"""Golden fixture of the fused network (include/tensor_game_net.h, mat_mul_amd.net), recorded by RUNNING THE
REFERENCE's own ``AlphaTensor`` (/root/reference/model.py) in eval mode with the weights of tests/net_ref.make_weights.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net.py      (build container only)

Per configuration <c> of net_ref.CONFIGS (a: the training app's defaults, b, c), the weights are regenerated from
``seed`` (<c>_seed), so only inputs and outputs are stored.  To keep the archive small, the outputs are recorded for the
first N_OUT of the 64 states and the torso output for the first N_EE; tests/net_ref.py's float64 restatement, which
reproduces every recorded output, stands in for the reference on the other states:
  <c>_keys bytes (n,), <c>_shapes int64 (n,4) (zero-padded): the state_dict's names and shapes, in the model's order;
  <c>_xx int8 (64,T,S,S,S) entries in {-2..2}, <c>_ss float32 (64,dim_s), <c>_g_action int8 (64,n_steps);
  <c>_ee{32,64} (N_EE,3S^2,c): the torso output, from the model in float32 and from copy.deepcopy(model).double();
  <c>_oo{32,64}, <c>_zz0{32,64}, <c>_q{32,64} (N_OUT,...): teacher-forced logits and zz[:, 0] (PolicyHead.fwd_train's
      forward on g_action) and the value head's quantiles on zz0, in float32 and float64;
  <c>_qq{32,64} (N_OUT,): the value output of fwd_infer (deterministic: it does not depend on the draws).
The archive is written deterministically (fixed member order and time stamps), so a rerun reproduces it byte for byte.
Nothing of the reference is copied.
"""
import copy
import io
import sys
import zipfile
from pathlib import Path

import numpy as np

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
OUT = HERE / "net_cases.npz"
SEEDS = {"a": 11, "b": 12, "c": 13}
N = 64      # input states
N_OUT = 8   # states whose oo, zz0, q and qq are recorded
N_EE = 1    # states whose torso output is recorded


def write_npz(path, arrays):
    """np.savez_compressed with fixed member order and time stamps: reruns are byte-identical."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, member.getvalue())
    Path(path).write_bytes(buf.getvalue())


def record(torch, model_mod, name, cfg):
    import net_ref

    seed = SEEDS[name]
    sd = net_ref.make_weights(cfg, seed)
    model = model_mod.AlphaTensor(**cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.eval()
    keys = list(model.state_dict().keys())
    shapes = np.zeros((len(keys), 4), np.int64)
    for i, k in enumerate(keys):
        s = model.state_dict()[k].shape
        shapes[i, :len(s)] = s
    xx, ss = net_ref.make_inputs(cfg, N, seed + 100)
    rng = np.random.default_rng(seed + 200)
    g_action = rng.integers(0, cfg["n_logits"], size=(N, cfg["n_steps"])).astype(np.int8)
    out = {f"{name}_seed": np.int64(seed), f"{name}_keys": np.array(keys, dtype=bytes), f"{name}_shapes": shapes,
           f"{name}_xx": xx, f"{name}_ss": ss, f"{name}_g_action": g_action}
    for tag, m, dt in (("32", model, torch.float32), ("64", copy.deepcopy(model).double(), torch.float64)):
        x = torch.from_numpy(xx[:N_OUT]).to(dt)
        s = torch.from_numpy(ss[:N_OUT]).to(dt)
        with torch.no_grad():
            ee = m.torso(x, s)
            oo, zz0 = m.policy_head.fwd_train(ee, torch.from_numpy(g_action[:N_OUT]).long())
            q = m.value_head(zz0)
            torch.manual_seed(0)
            _, _, qq = m.fwd_infer(x, s)
        out[f"{name}_ee{tag}"] = ee[:N_EE].numpy()
        out[f"{name}_oo{tag}"] = oo.numpy()
        out[f"{name}_zz0{tag}"] = zz0.numpy()
        out[f"{name}_q{tag}"] = q.numpy()
        out[f"{name}_qq{tag}"] = qq.numpy()
    return out


def main(out_path=OUT):
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    sys.path.insert(0, REF)
    import torch

    import model as model_mod  # noqa: E402  (reference)
    import net_ref

    torch.set_num_threads(1)  # a fixed summation order
    arrays = {}
    for name, cfg in net_ref.CONFIGS.items():
        arrays.update(record(torch, model_mod, name, cfg))
    write_npz(out_path, arrays)
    print(f"wrote {out_path} ({Path(out_path).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
