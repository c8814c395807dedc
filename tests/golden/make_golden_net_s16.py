#!/usr/bin/env python3
"""Golden fixture of the network at S = 16 (tests/net_s16_ref.CONFIGS: a16, b16), recorded by RUNNING THE REFERENCE's
own ``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the recorder of make_golden_net.py (eval-mode
outputs), unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_s16.py      (build container only)

writes net_s16_cases.npz (N input states; outputs of the first 4, the torso output of the first 1) with the members
that script describes under the names a16_* and b16_*.  Deterministic (write_npz).  Nothing of the reference is copied.
There is no training archive: training at S = 16 is not built.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
N = 6  # input states per configuration


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    import make_golden_net as mgn

    sys.path.insert(0, mgn.REF)
    import torch

    import model as model_mod  # noqa: E402  (reference)
    import net_s16_ref

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = N, 4, 1  # the archive stays small at S = 16
    mgn.SEEDS.update(net_s16_ref.SEEDS_NET)
    arrays = {}
    for cfg_name, cfg in net_s16_ref.CONFIGS.items():
        arrays.update(mgn.record(torch, model_mod, cfg_name, cfg))
    out = HERE / "net_s16_cases.npz"
    mgn.write_npz(out, arrays)
    print(f"wrote {out} ({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
