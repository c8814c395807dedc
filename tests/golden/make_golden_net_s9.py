#!/usr/bin/env python3
"""Golden fixtures of the network at S = 9 (tests/net_s9_ref.CONFIGS: a9, b9), recorded by RUNNING THE REFERENCE's own
``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the recorders of make_golden_net.py (eval-mode
outputs) and make_golden_train.py (train-mode losses, gradients and AdamW steps), unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_s9.py      (build container only)

writes net_s9_cases.npz (16 input states; outputs of the first 4, the torso output of the first 1) and
train_s9_cases.npz (4 states), with the members those scripts describe under the names a9_* and b9_*.  Deterministic
(write_npz).  Nothing of the reference is copied.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    import make_golden_net as mgn

    sys.path.insert(0, mgn.REF)
    import torch

    import make_golden_train as mgt
    import model as model_mod  # noqa: E402  (reference)
    import net_s9_ref

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = 16, 4, 1  # the archives stay small at S = 9
    mgn.SEEDS.update(net_s9_ref.SEEDS_NET)
    mgt.SEEDS.update(net_s9_ref.SEEDS_TRAIN)
    for recorder, name in ((mgn, "net_s9_cases.npz"), (mgt, "train_s9_cases.npz")):
        arrays = {}
        for cfg_name, cfg in net_s9_ref.CONFIGS.items():
            arrays.update(recorder.record(torch, model_mod, cfg_name, cfg))
        mgn.write_npz(HERE / name, arrays)
        print(f"wrote {HERE / name} ({(HERE / name).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
