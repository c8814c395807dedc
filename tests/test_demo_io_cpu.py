"""N4: packed demo files and the reference's on-disk layout.  CPU only."""
import numpy as np
import pytest
import torch

from mat_mul_amd import demo_io
from oracle import tensor_game as O


def _demos(B=5, S=4, R=6, seed=3):
    thr = O.categorical_thresholds((0.15, 0.7, 0.15))
    tok, tgt, _ = O.gen_demos_i8(B, S, R, thr, (-1, 0, 1), 1, seed=seed)
    return torch.from_numpy(tok), torch.from_numpy(tgt)


def test_packed_roundtrip(tmp_path):
    tok, tgt = _demos()
    f = tmp_path / "demos.tgd"
    demo_io.save_packed(f, tok, tgt, shift=1, seed=3, game_id_offset=10)
    assert f.stat().st_size == 64 + tok.numel() + tgt.numel()
    for mmap in (True, False):
        tok2, tgt2, meta = demo_io.load_packed(f, mmap=mmap)
        assert torch.equal(tok2, tok) and torch.equal(tgt2, tgt)
        assert meta == {"B": 5, "R": 6, "S": 4, "shift": 1, "seed": 3, "game_id_offset": 10}
    f.write_bytes(f.read_bytes()[:-1])
    with pytest.raises(ValueError, match="truncated"):
        demo_io.load_packed(f)


def test_reference_layout_roundtrip(tmp_path):
    tok, tgt = _demos(B=4, S=9, R=5)
    assert demo_io.export_reference_layout(tmp_path, tok, tgt) == 4
    seq = torch.load(tmp_path / "action_seq_2.pt")
    assert isinstance(seq, list) and len(seq) == 5 and seq[0].dtype == torch.int64 and seq[0].shape == (27,)
    t = torch.load(tmp_path / "target_tensor_2.pt")
    assert t.dtype == torch.float32 and t.shape == (9, 9, 9)
    tok2, tgt2 = demo_io.import_reference_layout(tmp_path, 4)
    assert torch.equal(tok2, tok) and torch.equal(tgt2, tgt)


def test_reference_dataset_reads_our_files(tmp_path, golden):
    """The reference's own SyntheticDemoDataset(overwrite=False) consumed the exported files of these demos, and what
    its __getitem__ (datasets.py:78-122) returned is recorded (tests/golden/reference_dataset_getitem.npz,
    make_golden_reference_runs.py).  The files written today carry the same demos in the reference's layout, read the
    way the dataset reads them (datasets.py:55, 86-89), and the oracle predicts the recorded items from them."""
    g = golden("reference_dataset_getitem")
    tok, tgt = _demos(B=3, S=4, R=7, seed=11)
    assert np.array_equal(tok.numpy(), g["tokens"]) and np.array_equal(tgt.numpy(), g["target"])
    demo_io.export_reference_layout(tmp_path / "d", tok, tgt)
    assert len(list((tmp_path / "d").glob("target_tensor_*.pt"))) == 3
    for i in range(21):
        d, ia = divmod(i, 7)
        seq = torch.load(tmp_path / "d" / f"action_seq_{d}.pt")
        target = torch.load(tmp_path / "d" / f"target_tensor_{d}.pt")
        assert isinstance(seq, list) and all(a.dtype == torch.int64 for a in seq) and target.dtype == torch.float32
        f, sc, a, rw = O.demo_getitem([s.numpy() for s in seq], target.numpy(), ia, 2)
        assert np.array_equal(g["frames"][i], f) and g["meta"][i].tolist() == [sc, rw]
        assert np.array_equal(g["action"][i], a)
        # and from the tokens as generated, without the files
        f2, sc2, a2, rw2 = O.demo_getitem(list(tok[d].numpy()), tgt[d].numpy(), ia, 2)
        assert np.array_equal(f2, f) and [sc2, rw2] == [sc, rw] and np.array_equal(a2, a)
