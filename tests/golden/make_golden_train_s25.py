#!/usr/bin/env python3
"""Golden fixture of the training loss and gradient at S = 25 (tests/net_s25_ref.CONFIGS: a25, b25;
include/tensor_game_train_s25.h), recorded by RUNNING THE REFERENCE's own ``AlphaTensor`` (its model.py, where
make_golden_net.REF points) in train mode with the recorder of make_golden_train.py, unchanged but for B_CASE = 2:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_s25.py      (build container only)

writes train_s25_cases.npz (2 states per configuration, train_ref.make_batch(cfg, 2, seed + 300)), with the members
that script describes under the names a25_* and b25_*.  Deterministic (write_npz).  Nothing of the reference is copied.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "train_s25_cases.npz"
SEEDS_TRAIN = {"a25": 71, "b25": 72}
B_CASE = 2


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
    import net_s25_ref

    torch.set_num_threads(1)  # a fixed summation order
    mgt.SEEDS.update(SEEDS_TRAIN)
    mgt.B_CASE = B_CASE
    arrays = {}
    for name in net_s25_ref.RECORDED:
        arrays.update(mgt.record(torch, model_mod, name, net_s25_ref.CONFIGS[name]))
    mgn.write_npz(OUT, arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
