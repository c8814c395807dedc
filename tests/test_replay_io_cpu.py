"""CPU checks of the replay buffers' dense form and of the files of mat_mul_amd.replay_io
(include/tensor_game_replay_io.h): the header is plain C and both libraries export exactly its symbols; both entries
refuse bad arguments in their documented order before any device work; the host restatement (tests/replay_io_ref.py)
of pack and add_packed reproduces the reference's ring (tests/golden/replay_cases.npz); the buffer file round-trips and
refuses a wrong magic and a wrong size; the reference's three-files-per-game layout round-trips and reads back as the
reference's own PlayedGamesDataset reads it; a run refuses a CPU device."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import replay_io_ref as IO
import replay_ref as RR
from mat_mul_amd import _lib, build, replay_io

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "tensor_game_replay_io.h"
RINGS = ["S4_T2", "S16_T1"]
SYMS = ["tg_replay_add_packed", "tg_replay_pack"]


# ---- the header ---------------------------------------------------------------------------------------------------------
def test_replay_io_header_is_plain_c():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    res = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wpedantic", "-Werror",
                          "-I", str(ROOT / "include"), str(HDR)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_replay_io_header_symbols_exported_by_both_libraries():
    syms = sorted(set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", HDR.read_text(), flags=re.M)))
    assert syms == SYMS
    assert sorted(_lib.REPLAY_IO_SIGNATURES) == syms
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "REPLAY_IO_SIGNATURES"]
    assert len(others) >= 9 and not any(set(syms) & set(t) for t in others)
    for path in (_lib.LIB_PATH, build.lib_path(ab=True)):
        lib = C.CDLL(str(path))
        for s in syms:
            assert hasattr(lib, s), (path, s)
    text = HDR.read_text()
    assert int(re.search(r"#define TG_REPLAY_IO_BAD_LENGTH (\d+)u", text).group(1)) == _lib.TG_REPLAY_IO_BAD_LENGTH
    assert int(re.search(r"#define TG_REPLAY_IO_TRUNCATED (\d+)u", text).group(1)) == _lib.TG_REPLAY_IO_TRUNCATED


# ---- the host checks, in their order --------------------------------------------------------------------------------------
ONE = 64  # a pointer that is never dereferenced: validation fails first


def _desc(**over):
    d = _lib.ReplayBufferDesc(C=8, L=4, T=2, S=4)
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        setattr(d, name, ONE)
    for key, val in over.items():
        setattr(d, key, val)
    return d


def _pack(d, **over):
    kw = dict(max_moves=5, lengths=ONE, move_offset=ONE, counts=ONE, rewards=ONE, tokens=ONE, frames=ONE, status=ONE)
    kw.update(over)
    p = lambda k: C.c_void_p(kw[k])
    return _lib.lib.tg_replay_pack(None if d is None else C.byref(d), kw["max_moves"], p("lengths"), p("move_offset"),
                                   p("counts"), p("rewards"), p("tokens"), p("frames"), p("status"), None)


def _unpack(d, **over):
    kw = dict(frames=ONE, tokens=ONE, rewards=ONE, lengths=ONE, G=2, M=5, first_slot=-1, games_added=-1, status=ONE)
    kw.update(over)
    p = lambda k: C.c_void_p(kw[k])
    return _lib.lib.tg_replay_add_packed(None if d is None else C.byref(d), p("frames"), p("tokens"), p("rewards"),
                                         p("lengths"), kw["G"], kw["M"], kw["first_slot"], kw["games_added"],
                                         p("status"), None)


def refused(call, fn, words, d, **over):
    err = _lib.lib.tg_last_error
    assert call(d, **over) == -1 and fn in err() and words in err(), (over, err())


SIZES = [(dict(C=0), b"C=0"), (dict(C=65537), b"C=65537"), (dict(L=0), b"L=0"), (dict(L=4097), b"L=4097"),
         (dict(T=0), b"T=0"), (dict(T=17), b"T=17"), (dict(S=0), b"S=0"), (dict(S=33), b"S=33")]


def test_pack_validation_without_gpu_in_order():
    fn = b"tg_replay_pack"
    refused(_pack, fn, b"null buffer", None)
    for over, words in SIZES:
        # a bad size wins over everything after it: a negative max_moves, null and misaligned pointers
        refused(_pack, fn, words, _desc(frames=None, offset=ONE + 4, **over), max_moves=-1, lengths=None)
    refused(_pack, fn, b"max_moves=-1", _desc(frames=None), max_moves=-1, lengths=None)
    for name in ("frames", "tokens", "rewards", "length", "offset", "ring"):
        refused(_pack, fn, b"null buffer array", _desc(**{name: None, "offset" if name != "offset" else "ring": ONE + 4}),
                lengths=None)
    for name, at in (("rewards", ONE + 2), ("length", ONE + 2), ("offset", ONE + 4), ("ring", ONE + 4)):
        refused(_pack, fn, b"buffer arrays not aligned", _desc(**{name: at}), lengths=None)
    for name in ("lengths", "move_offset", "counts"):
        refused(_pack, fn, b"null lengths_out", _desc(), **{name: None, "rewards": ONE + 2})
    for name in ("rewards", "tokens", "frames"):
        refused(_pack, fn, b"null rewards_out", _desc(), **{name: None, "counts": ONE + 4})
    for name, at in (("lengths", ONE + 2), ("move_offset", ONE + 4), ("counts", ONE + 4), ("rewards", ONE + 2),
                     ("status", ONE + 2)):
        refused(_pack, fn, b"not aligned", _desc(), **{name: at})


def test_add_packed_validation_without_gpu_in_order():
    fn = b"tg_replay_add_packed"
    refused(_unpack, fn, b"null buffer", None)
    for over, words in SIZES:
        refused(_unpack, fn, words, _desc(frames=None, **over), M=-1, G=-1, first_slot=8, lengths=None)
    refused(_unpack, fn, b"M=-1", _desc(frames=None), M=-1, G=-1, first_slot=8)
    refused(_unpack, fn, b"G=-1", _desc(frames=None), G=-1, first_slot=8)
    refused(_unpack, fn, b"G=2147483649", _desc(frames=None), G=2 ** 31 + 1, first_slot=8)
    refused(_unpack, fn, b"first_slot=8", _desc(frames=None), first_slot=8, games_added=-2)
    refused(_unpack, fn, b"first_slot=-2", _desc(frames=None), first_slot=-2)
    refused(_unpack, fn, b"games_added=-2", _desc(frames=None), games_added=-2)
    refused(_unpack, fn, b"null buffer array", _desc(ring=None), lengths=None)
    refused(_unpack, fn, b"buffer arrays not aligned", _desc(offset=ONE + 4), lengths=None)
    assert _unpack(_desc(), G=0, frames=None, tokens=None, rewards=None, lengths=None) == 0  # no games: a no-op
    refused(_unpack, fn, b"null lengths", _desc(), lengths=None, frames=None)
    for name in ("frames", "tokens", "rewards"):
        refused(_unpack, fn, b"null frames", _desc(), **{name: None, "lengths": ONE + 2})
    for name, at in (("lengths", ONE + 2), ("rewards", ONE + 2), ("status", ONE + 1)):
        refused(_unpack, fn, b"not aligned", _desc(), **{name: at})


# ---- the restatement against the reference's ring ----------------------------------------------------------------------
def ring_games(g, name):
    return [g[f"ring_{name}_{k}"] for k in ("states", "policy", "rewards", "lengths")]


def check_snapshot(g, name, a, ring):
    items = [ring.getitem(i) for i in range(len(ring))]
    assert np.array_equal(np.stack([it[0] for it in items]), g[f"ring_{name}_snap{a}_frames"])
    assert np.array_equal(np.array([it[1] for it in items]), g[f"ring_{name}_snap{a}_scalar"])
    assert np.array_equal(np.stack([it[2] for it in items]), g[f"ring_{name}_snap{a}_action"])
    assert np.array_equal(np.array([it[3] for it in items]), g[f"ring_{name}_snap{a}_reward"])


@pytest.mark.parametrize("name", RINGS)
def test_restated_pack_then_add_packed_reproduces_the_reference_ring(golden, name):
    g = golden("replay_cases")
    states, policy, rewards, lengths = ring_games(g, name)
    L, T, S = states.shape[1], states.shape[2], states.shape[3]
    ring = RR.Ring(3, L)
    for a in range(len(lengths)):
        ring.add(states[a:a + 1], policy[a:a + 1], rewards[a:a + 1], lengths[a:a + 1])
        p = IO.pack(ring, T, S)
        G = len(p["lengths"])
        assert p["status"] == 0 and p["written"] == p["counts"][1] == len(ring) and G == min(a + 1, 3)
        # oldest first: the last game of the dense form is the one just added
        n = int(lengths[a])
        assert p["lengths"][-1] == n and np.array_equal(p["frames"][-n:], states[a, :n])
        # into the slots it had: the same ring, the same items
        back = RR.Ring(3, L)
        assert IO.add_packed(back, p["frames"], p["tokens"], p["rewards"], p["lengths"],
                             first_slot=(ring.pointer - G) % 3, games_added=ring.added) == 0
        assert IO.rings_equal(back, ring)
        check_snapshot(g, name, a, back)
        # into an empty ring from its start: the games oldest first; the same slots until the ring has wrapped
        fresh = RR.Ring(3, L)
        assert IO.add_packed(fresh, p["frames"], p["tokens"], p["rewards"], p["lengths"]) == 0
        assert fresh.added == G and len(fresh) == len(ring)
        if a < 3:
            check_snapshot(g, name, a, fresh)
        # the defining property: equal to replay_ref's add of the same games, padded, with one-hot policies
        padded = RR.Ring(3, L)
        st, po, rw = np.zeros((G, L) + states.shape[2:], np.int8), np.zeros((G, L, 3 * S, 3), np.float32), \
            np.zeros((G, L), np.float32)
        for r in range(G):
            lo, hi = int(p["move_offset"][r]), int(p["move_offset"][r + 1])
            st[r, :hi - lo], rw[r, :hi - lo] = p["frames"][lo:hi], p["rewards"][lo:hi]
            po[r, :hi - lo] = np.eye(3, dtype=np.float32)[p["tokens"][lo:hi]]
        padded.add(st, po, rw, p["lengths"].astype(np.int64))
        assert IO.rings_equal(padded, fresh)


def test_restated_edges():
    rng = np.random.default_rng(1)
    L, T, S = 3, 1, 2
    ring = RR.Ring(4, L)
    ln = np.array([2, 0, 3, 4, -1, 1, 2], np.int32)
    M = int(np.maximum(ln, 0).sum())
    fr = rng.integers(-2, 3, size=(M, T, S, S, S)).astype(np.int8)
    tk = rng.integers(0, 3, size=(M, 3 * S)).astype(np.int8)
    rw = rng.random(M).astype(np.float32)
    assert IO.add_packed(ring, fr, tk, rw, ln, first_slot=3) == IO.BAD_LENGTH
    assert sorted(ring.slots) == [0, 1, 2, 3] and ring.pointer == 3 and ring.added == 4  # games 0, 2, 5, 6
    assert np.array_equal(ring.slots[3][0], fr[0:2]) and np.array_equal(ring.slots[0][0], fr[2:5])
    assert np.array_equal(ring.slots[1][0], fr[9:10]) and np.array_equal(ring.slots[2][0], fr[10:12])
    cut = RR.Ring(4, L)
    assert IO.add_packed(cut, fr, tk, rw, ln, M=11) == IO.BAD_LENGTH | IO.TRUNCATED
    assert sorted(cut.slots) == [0, 1, 2] and cut.added == 3
    p = IO.pack(ring, T, S, max_moves=4)  # oldest first from slot 3: lengths 2, 3, 1, 2; 4 rows cut the second game
    assert p["lengths"].tolist() == [2, 3, 1, 2] and p["counts"].tolist() == [4, 8] and p["written"] == 2
    assert p["status"] == IO.TRUNCATED and np.array_equal(p["frames"], fr[0:2])
    many = RR.Ring(2, L)
    assert IO.add_packed(many, fr, tk, rw, ln, games_added=9) == IO.BAD_LENGTH  # 4 games into 2 slots: the last two
    assert np.array_equal(many.slots[0][0], fr[9:10]) and np.array_equal(many.slots[1][0], fr[10:12])
    assert many.pointer == 0 and many.added == 9


# ---- the buffer file ------------------------------------------------------------------------------------------------------
def packed_of(ring, T, S):
    p = IO.pack(ring, T, S)
    return replay_io.PackedGames(ring.C, ring.L, T, S, (ring.pointer, ring.added), p["lengths"], p["rewards"],
                                 p["tokens"], p["frames"])


def golden_ring(g, name, adds):
    states, policy, rewards, lengths = ring_games(g, name)
    ring = RR.Ring(3, states.shape[1])
    ring.add(states[:adds], policy[:adds], rewards[:adds], lengths[:adds])
    return ring, states.shape[2], states.shape[3]


def test_file_round_trip_and_refusals(golden, tmp_path):
    g = golden("replay_cases")
    ring, T, S = golden_ring(g, "S4_T2", 4)
    empty = RR.Ring(5, 7)
    for k, p in enumerate((packed_of(ring, T, S), packed_of(empty, 2, 3))):
        path = tmp_path / f"buf{k}.tgr"
        replay_io.save_games(path, p)
        raw = path.read_bytes()
        assert raw == IO.file_bytes(p.C, p.L, p.T, p.S, p.ring, p.lengths, p.rewards, p.tokens, p.frames)
        assert len(raw) == 128 + 4 * p.G + p.M * (4 + 3 * p.S + p.T * p.S ** 3)
        back = replay_io.load_games(path)
        assert back.equals(p) and back.G == p.G and back.M == p.M
        for name, data, words in (("magic", b"TGREPLYX" + raw[8:], "not a packed replay buffer"),
                                  ("short", raw[:-1], "truncated"), ("long", raw + b"\0", "longer")):
            bad = tmp_path / f"{name}{k}.tgr"
            bad.write_bytes(data)
            with pytest.raises(ValueError, match=words):
                replay_io.load_games(bad)
    assert packed_of(empty, 2, 3).G == 0 and packed_of(ring, T, S).G == 3
    with pytest.raises(ValueError, match="truncated"):
        (tmp_path / "head.tgr").write_bytes(b"TGREPLY1" + b"\0" * 50)
        replay_io.load_games(tmp_path / "head.tgr")


def test_dataset_file_round_trip_and_refusals(golden, tmp_path):
    g = golden("replay_cases")
    ring, T, S = golden_ring(g, "S4_T2", 4)
    rng = np.random.default_rng(2)
    R, n_demos, L = 5, 6, ring.L
    d = dict(len_data=20, dim_t=T, shift=1, R=R, S=S, n_demos=n_demos, fract_synth=0.7, fract_best=0.1,
             targets_hash=-(2 ** 62) - 12345, is_synth=rng.random(20) < 0.7, index_synth=rng.integers(0, 30, size=14),
             index_played=np.zeros(0, np.int64), index_best=None, generator=rng.integers(0, 256, size=16).astype(np.uint8),
             played=packed_of(ring, T, S), best=packed_of(RR.Ring(2, L), T, S),
             tokens=rng.integers(0, 3, size=(n_demos, R, 3 * S)).astype(np.int8),
             targets=rng.integers(-2, 3, size=(n_demos, S, S, S)).astype(np.int8))
    for demos in (True, False):
        path = tmp_path / f"data{int(demos)}.tgd"
        replay_io.save_dataset(path, d if demos else dict(d, tokens=None, targets=None))
        back = replay_io.load_dataset(path)
        for key, val in d.items():
            if key in ("played", "best"):
                assert back[key].equals(val), key
            elif key in ("tokens", "targets") and not demos:
                assert back[key] is None
            elif val is None or np.isscalar(val):
                assert back[key] == val and type(back[key]) is type(val), key
            else:
                assert np.array_equal(back[key], val) and back[key].dtype == np.asarray(val).dtype, key
        raw = path.read_bytes()
        for name, data, words in (("magic", b"TGDATA0X" + raw[8:], "not a saved TensorGameData"),
                                  ("short", raw[:-1], "truncated"), ("long", raw + b"\0", "longer")):
            (tmp_path / name).write_bytes(data)
            with pytest.raises(ValueError, match=words):
                replay_io.load_dataset(tmp_path / name)
    assert (tmp_path / "data1.tgd").stat().st_size - (tmp_path / "data0.tgd").stat().st_size == n_demos * (R * 3 * S + S ** 3)


# ---- the reference's layout ---------------------------------------------------------------------------------------------
def reference_getitem(save_dir, game_lengths, idx):
    """PlayedGamesDataset.__getitem__ (datasets.py:196-208), restated: walk the slots from 0, load the three files."""
    i = 0
    while idx >= game_lengths[i]:
        idx -= game_lengths[i]
        i += 1
    state_seq = torch.load(Path(save_dir, f"state_seq_{i}.pt"))
    action_seq = torch.load(Path(save_dir, f"action_seq_{i}.pt"))
    reward_seq = torch.load(Path(save_dir, f"reward_seq_{i}.pt"))
    return state_seq[idx], float(idx), action_seq[idx].argmax(dim=-1), reward_seq[idx].reshape(1)


@pytest.mark.parametrize("name", RINGS)
def test_reference_layout_round_trips_and_reads_as_the_reference_does(golden, name, tmp_path):
    g = golden("replay_cases")
    n_logits = g[f"ring_{name}_policy"].shape[-1]
    for a in (1, 4):  # before the ring wraps, and after
        ring, T, S = golden_ring(g, name, a + 1)
        p = packed_of(ring, T, S)
        d = tmp_path / f"games{a}"
        game_lengths, pointer = replay_io.export_reference_games(d, p, n_logits)
        assert pointer == ring.pointer and game_lengths == {s: len(v[2]) for s, v in sorted(ring.slots.items())}
        assert sorted(f.name for f in d.iterdir()) == sorted(
            f"{k}_seq_{s}.pt" for k in ("state", "action", "reward") for s in game_lengths)
        one = torch.load(d / "action_seq_0.pt")
        assert isinstance(one, list) and one[0].dtype == torch.float32 and one[0].shape == (3 * S, n_logits)
        assert torch.equal(one[0].sum(-1), torch.ones(3 * S)) and set(one[0].unique().tolist()) == {0.0, 1.0}
        st = torch.load(d / "state_seq_0.pt")
        assert isinstance(st, list) and st[0].dtype == torch.float32 and st[0].shape == (T, S, S, S)
        back = replay_io.import_reference_games(d, game_lengths, pointer, buffer_size=3, max_actions=ring.L,
                                                games_added=ring.added)
        assert back.equals(p)
        items = [reference_getitem(d, game_lengths, i) for i in range(sum(game_lengths.values()))]
        assert np.array_equal(np.stack([it[0].numpy() for it in items]).astype(np.int8), g[f"ring_{name}_snap{a}_frames"])
        assert np.array_equal(np.array([it[1] for it in items], np.float32), g[f"ring_{name}_snap{a}_scalar"])
        assert np.array_equal(np.stack([it[2].numpy() for it in items]), g[f"ring_{name}_snap{a}_action"])
        assert np.array_equal(np.array([it[3].item() for it in items], np.float32), g[f"ring_{name}_snap{a}_reward"])


def test_reference_import_refuses_what_does_not_fit_int8(golden, tmp_path):
    g = golden("replay_cases")
    ring, T, S = golden_ring(g, "S4_T2", 2)
    p = packed_of(ring, T, S)
    lengths, pointer = replay_io.export_reference_games(tmp_path, p, 3)
    with pytest.raises(ValueError, match="outside"):
        replay_io.export_reference_games(tmp_path / "x", p, 2)  # the fixture's tokens reach 2
    st = torch.load(tmp_path / "state_seq_1.pt")
    st[0][0, 0, 0, 0] = 128.0
    torch.save(st, tmp_path / "state_seq_1.pt")
    with pytest.raises(ValueError, match="int8"):
        replay_io.import_reference_games(tmp_path, lengths, pointer, buffer_size=3)
    st[0][0, 0, 0, 0] = 0.5
    torch.save(st, tmp_path / "state_seq_1.pt")
    with pytest.raises(ValueError, match="int8"):
        replay_io.import_reference_games(tmp_path, lengths, pointer, buffer_size=3)


READER = """
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, sys.argv[1])
import numpy as np
import datasets
games, out, pointer = sys.argv[2], sys.argv[3], int(sys.argv[4])
lengths = {int(k): int(v) for k, v in (kv.split(":") for kv in sys.argv[5].split(","))}
buf = datasets.PlayedGamesDataset(3, "cpu", save_dir=games)
buf.game_lengths, buf.game_pointer = lengths, pointer
items = [buf[i] for i in range(len(buf))]
np.savez(out, frames=np.stack([it[0].numpy() for it in items]), scalar=np.array([it[1].item() for it in items]),
         action=np.stack([it[2].numpy() for it in items]), reward=np.array([it[3].item() for it in items]))
buf.save_dir = buf.save_dir / "nothing"  # its __del__ deletes the games of its save_dir
"""


@pytest.mark.parametrize("name", RINGS)
def test_the_reference_reads_the_exported_games(golden, name, tmp_path):
    spec = importlib.util.spec_from_file_location("make_golden_replay", ROOT / "tests" / "golden" / "make_golden_replay.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not (Path(mod.REF) / "datasets.py").exists():
        pytest.skip("the reference checkout is not present")
    g = golden("replay_cases")
    a = 4
    ring, T, S = golden_ring(g, name, a + 1)
    lengths, pointer = replay_io.export_reference_games(tmp_path / "games", packed_of(ring, T, S),
                                                        g[f"ring_{name}_policy"].shape[-1])
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, "-c", READER, mod.REF, str(tmp_path / "games"), str(tmp_path / "out.npz"),
                          str(pointer), ",".join(f"{k}:{v}" for k, v in lengths.items())],
                         capture_output=True, text=True, env=env, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    assert np.array_equal(out["frames"].astype(np.int8), g[f"ring_{name}_snap{a}_frames"])
    assert np.array_equal(out["scalar"].astype(np.float32), g[f"ring_{name}_snap{a}_scalar"])
    assert np.array_equal(out["action"], g[f"ring_{name}_snap{a}_action"])
    assert np.array_equal(out["reward"].astype(np.float32), g[f"ring_{name}_snap{a}_reward"])


# ---- no CPU path ----------------------------------------------------------------------------------------------------------
def test_a_run_refuses_the_cpu(tmp_path):
    from mat_mul_amd import FusedTrainer, GameBuffer, TensorGameData

    ckpt = {"config": {}, "params": torch.zeros(4), "pos_fix": torch.zeros(4), "dropout_p": 0.0, "weight_pol": 1.0,
            "weight_val": 1.0, "n_samples": 1, "seed": 0, "calls": 0}
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        FusedTrainer.from_checkpoint(ckpt, "cpu")
    assert FusedTrainer.checkpoint.__doc__ and "host" in FusedTrainer.checkpoint.__doc__
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        replay_io.load_run(tmp_path, "cpu")
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        replay_io.save_run(tmp_path / "run", None, None, None, generators={"loader": torch.Generator()})
    assert not (tmp_path / "run").exists()
    replay_io.save_games(tmp_path / "b.tgr", packed_of(RR.Ring(2, 2), 1, 2))
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        GameBuffer.load(tmp_path / "b.tgr", "cpu")
    with pytest.raises(_lib.TensorGameError, match="no CPU path"):
        TensorGameData.load(tmp_path / "b.tgr", "cpu")
