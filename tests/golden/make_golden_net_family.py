#!/usr/bin/env python3
"""Golden fixtures of the network family's reference-reachable rows (tests/net_family.REFERENCE_ROWS: e, f, g), recorded
by RUNNING THE REFERENCE's own ``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the recorders of
make_golden_net.py (eval-mode outputs) and make_golden_train.py (train-mode losses, gradients and AdamW steps),
unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_family.py      (build container only)

writes net_family_cases.npz (e, f, g: 16 input states; outputs of the first 4, the torso output of the first 1) and
train_family_cases.npz (the training rows e and g: 4 states), with the members those scripts describe under the names
e_*, f_* and g_*.  At g the full tensors recorded are FULL without the value head's 512 x 16 output weight, which its
projections still cover, so that the archive stays small.  Deterministic (write_npz).  Nothing of the reference is
copied.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
SEEDS_NET = {"e": 61, "f": 62, "g": 63}
SEEDS_TRAIN = {"e": 71, "g": 72}


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
    from net_family import FAMILY, REFERENCE_ROWS

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = 16, 4, 1
    mgn.SEEDS.update(SEEDS_NET)
    mgt.SEEDS.update(SEEDS_TRAIN)
    full = list(mgt.FULL)
    small = {"g": [k for k in full if k != "value_head.mlp.6.weight"]}
    for recorder, name, rows in ((mgn, "net_family_cases.npz", REFERENCE_ROWS),
                                 (mgt, "train_family_cases.npz", [r for r in REFERENCE_ROWS if FAMILY[r].train])):
        arrays = {}
        for row in rows:
            mgt.FULL = small.get(row, full)
            arrays.update(recorder.record(torch, model_mod, row, FAMILY[row].cfg))
        mgt.FULL = full
        mgn.write_npz(HERE / name, arrays)
        print(f"wrote {HERE / name} ({(HERE / name).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
