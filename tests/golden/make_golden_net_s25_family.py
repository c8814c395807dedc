#!/usr/bin/env python3
"""Golden fixture of the S = 25 network family's reference-reachable rows (tests/net_s25_family.REFERENCE_ROWS: e25,
f25), recorded by RUNNING THE REFERENCE's own ``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the
recorder of make_golden_net.py (eval-mode outputs, in float32 and in float64), unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_s25_family.py      (build container only)

writes net_s25_family_cases.npz (N input states and their outputs) with the members that script describes under the
names e25_* and f25_*.  As in make_golden_net_s25.py, of the torso output of the first state only the slices i = 0, 12
and 24 are kept, <row>_ee{32,64} (1,3,75,c) = rows i*75 .. i*75 + 74 of ee[0] for i in <row>_ee_slices; the float64
restatement is checked on those and stands in for the rest, and for the reference at every other state.  N = 2 keeps the
archive no larger than the largest of the others (train_s25_cases.npz, 255 337 bytes): the int8 frames of e25 at T = 8
are 122 KiB a state before compression.  Deterministic (write_npz).  Nothing of the reference is copied.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
N = 2  # input states per row
LARGEST = 255337  # bytes of the largest fixture beside this one


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
    import net_s25_family as F25
    from net_s25_ref import EE_SLICES

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = N, N, 1
    mgn.SEEDS.update(F25.SEEDS_NET)
    arrays = {}
    for row in F25.REFERENCE_ROWS:
        cfg = F25.FAMILY25[row].cfg
        rec = mgn.record(torch, model_mod, row, cfg)
        for tag in ("32", "64"):
            ee = rec[f"{row}_ee{tag}"]
            assert ee.shape == (1, 3 * 25 * 25, cfg["dim_c"])
            rec[f"{row}_ee{tag}"] = ee.reshape(1, 25, 75, -1)[:, list(EE_SLICES)]
        rec[f"{row}_ee_slices"] = np.array(EE_SLICES, np.int64)
        arrays.update(rec)
    out = HERE / "net_s25_family_cases.npz"
    mgn.write_npz(out, arrays)
    size = out.stat().st_size
    print(f"wrote {out} ({size} bytes)")
    assert size <= LARGEST, size


if __name__ == "__main__":
    main()
