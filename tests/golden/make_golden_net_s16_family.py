#!/usr/bin/env python3
"""Golden fixture of the S = 16 network family's reference-reachable rows (tests/net_s16_family.REFERENCE_ROWS: e16,
f16), recorded by RUNNING THE REFERENCE's own ``AlphaTensor`` (its model.py, where make_golden_net.REF points) with the
recorder of make_golden_net.py (eval-mode outputs), unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_s16_family.py      (build container only)

writes net_s16_family_cases.npz (N input states and their outputs, at most 2 of them; the torso output of the first 1)
with the members that script describes under the names e16_* and f16_*.  N = 1 keeps the archive (175 146 bytes) no
larger than the largest of the others (net_s16_cases.npz, 192 080 bytes): N = 3 gives 208 234 bytes and N = 2 192 940,
since ee of e16 alone is 768 x 12 values in two precisions and int8 frames at T = 8 are 32 KiB a state.  The float64
restatement, which reproduces what is recorded, stands in for the reference at every other state.  Deterministic
(write_npz).  Nothing of the reference is copied.  There is no training archive: training at S = 16 is not built.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
N = 1  # input states per row


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    sys.path.insert(0, str(HERE.parent))
    sys.path.insert(0, str(HERE.parent.parent))
    import make_golden_net as mgn

    sys.path.insert(0, mgn.REF)
    import torch

    import model as model_mod  # noqa: E402  (reference)
    import net_s16_family as F16

    torch.set_num_threads(1)  # a fixed summation order
    mgn.N, mgn.N_OUT, mgn.N_EE = N, 2, 1
    mgn.SEEDS.update(F16.SEEDS_NET)
    arrays = {}
    for row in F16.REFERENCE_ROWS:
        arrays.update(mgn.record(torch, model_mod, row, F16.FAMILY16[row].cfg))
    out = HERE / "net_s16_family_cases.npz"
    mgn.write_npz(out, arrays)
    print(f"wrote {out} ({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
