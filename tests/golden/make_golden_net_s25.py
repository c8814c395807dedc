#!/usr/bin/env python3
"""Golden fixture of the network at S = 25 (tests/net_s25_ref.CONFIGS: a25, b25), recorded by RUNNING THE REFERENCE's
own ``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the recorder of make_golden_net.py (eval-mode
outputs, in float32 and in float64), unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_s25.py      (build container only)

writes net_s25_cases.npz (N = 4 input states; outputs of the first 2) with the members that script describes under the
names a25_* and b25_*.  One difference: the torso output of the first state would be 180 KB per configuration, so only
its slices i = 0, 12 and 24 are kept, <c>_ee{32,64} (1,3,75,c) = rows i*75 .. i*75 + 74 of ee[0] for i in <c>_ee_slices;
the float64 restatement is checked on those and stands in for the rest.  c25 has no recorded fixture.  Deterministic
(write_npz).  Nothing of the reference is copied.  There is no training archive: training at S = 25 is not built.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
N = 4  # input states per configuration


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    import make_golden_net as mgn

    sys.path.insert(0, mgn.REF)
    import numpy as np
    import torch

    import model as model_mod  # noqa: E402  (reference)
    import net_s25_ref

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = N, 2, 1  # the archive stays small at S = 25
    mgn.SEEDS.update(net_s25_ref.SEEDS_NET)
    arrays = {}
    for cfg_name in net_s25_ref.RECORDED:
        cfg = net_s25_ref.CONFIGS[cfg_name]
        rec = mgn.record(torch, model_mod, cfg_name, cfg)
        for tag in ("32", "64"):
            ee = rec[f"{cfg_name}_ee{tag}"]
            assert ee.shape == (1, 3 * 25 * 25, cfg["dim_c"])
            rec[f"{cfg_name}_ee{tag}"] = ee.reshape(1, 25, 75, -1)[:, list(net_s25_ref.EE_SLICES)]
        rec[f"{cfg_name}_ee_slices"] = np.array(net_s25_ref.EE_SLICES, np.int64)
        arrays.update(rec)
    out = HERE / "net_s25_cases.npz"
    mgn.write_npz(out, arrays)
    print(f"wrote {out} ({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
