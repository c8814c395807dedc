"""tg_replay_pack / tg_replay_add_packed and what is built on them (ops.replay_pack / replay_add_packed,
GameBuffer.pack / add_packed / save / load, TensorGameData.save / load, FusedTrainer.checkpoint, replay_io.save_run /
load_run) on the MI355X: bit for bit against the host restatement (tests/replay_io_ref.py), every output between guard
bytes with its unused part poisoned; the defining property of add_packed against tg_replay_add with one-hot policies;
the round trip through a file; graph capture; and a run that is saved after its first epoch and resumed in fresh objects
equals the uninterrupted run bit for bit."""
import functools
import itertools

import numpy as np
import pytest
import torch

import replay_io_ref as IO
import replay_ref as RR
import ring_cases as RC
from guarded_buffers import CANARY, check_flat, guarded
from mat_mul_amd import FusedTrainer, GameBuffer, SyntheticDemos, TensorGameData, ops, replay_io, search
from net_ref import CONFIGS, make_weights
from ring_cases import ARRAYS, guarded_buffer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (C, L, T, S): the aligned path; 27-byte frames (every packed row misaligned); misaligned with T = 3; 729-byte frames;
# the smallest buffer; two age positions per scan thread with a ragged last thread; the capacity bound
SHAPES = [(3, 4, 2, 4), (5, 3, 1, 3), (7, 2, 3, 5), (4, 3, 1, 9), (1, 1, 1, 1), (1025, 2, 1, 2), (65536, 1, 1, 1)]


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def random_games(rng, B, L, T, S, n_logits=3):
    st = rng.integers(-3, 4, size=(B, L, T, S, S, S)).astype(np.int8)
    po = rng.random((B, L, 3 * S, n_logits)).astype(np.float32)
    rw = -rng.integers(1, 9, size=(B, L)).astype(np.float32)
    ln = rng.integers(1, L + 1, size=B).astype(np.int64)
    return st, po, rw, ln


def dense_games(rng, lengths, T, S):
    """Dense rows for games of the given lengths (negative and zero lengths own no rows)."""
    M = int(np.maximum(lengths, 0).sum())
    return (rng.integers(-3, 4, size=(M, T, S, S, S)).astype(np.int8), rng.integers(0, 3, size=(M, 3 * S)).astype(np.int8),
            -rng.integers(1, 9, size=M).astype(np.float32))


def mirror(buf, ring):
    """Bring the host image of frames, tokens and rewards up to date after ONE call on the device: the stored moves of
    the ring's games over whatever the slots held before (a shorter game leaves the tail of the one it replaces)."""
    for s, game in ring.slots.items():
        for w, x in zip(buf.shadow, game):
            w[s, :len(x)] = x


def check_buffer(buf, ring, what):
    """The device buffer holds exactly ``ring``: length, offset, ring words, every stored move; everything else in
    frames, tokens and rewards is what it was (poison, or the tail of a replaced game); the guards are intact.  To be
    called, or ``mirror``, after every call that changes the buffer."""
    mirror(buf, ring)
    torch.cuda.synchronize()
    for name in ARRAYS:
        check_flat(buf.guards[name], (what, name))
    length, offset, words = IO.buffer_words(ring)
    assert np.array_equal(buf.length.cpu().numpy(), length), what
    assert np.array_equal(buf.offset.cpu().numpy(), offset), what
    assert np.array_equal(buf.ring.cpu().numpy(), words), what
    for w, name in zip(buf.shadow, ("frames", "tokens", "rewards")):
        got = getattr(buf, name).cpu().numpy()
        assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), (what, name)


def check_pack(buf, ring, what, max_moves=None, extra=2):
    """ops.replay_pack into guarded, poisoned outputs equals the restatement; nothing past what it says is written."""
    want = IO.pack(ring, buf.T, buf.S, max_moves)
    G, M = (int(v) for v in want["counts"])
    rows = M + extra if max_moves is None else max_moves
    shapes = dict(frames=((rows, buf.T, buf.S, buf.S, buf.S), torch.int8), tokens=((rows, 3 * buf.S), torch.int8),
                  rewards=((rows,), torch.float32), lengths=((buf.C,), torch.int32),
                  move_offset=((buf.C + 1,), torch.int64), counts=((2,), torch.int64), status=((1,), torch.uint32))
    out = {k: guarded(*v) for k, v in shapes.items()}
    out["status"][1].zero_()
    before = {n: getattr(buf, n).clone() for n in ARRAYS}
    ops.replay_pack(buf, rows, **{k: v[1] for k, v in out.items()})
    torch.cuda.synchronize()
    for k, (raw, _) in out.items():
        check_flat(raw, (what, k))
    for n in ARRAYS:  # nothing of the buffer is modified
        assert torch.equal(getattr(buf, n).view(torch.uint8), before[n].view(torch.uint8)), (what, n)
    got = {k: v[1].cpu().numpy() for k, v in out.items()}
    assert got["counts"].tolist() == [G, M] and int(got["status"][0]) == want["status"], what
    poison = lambda a: np.frombuffer(bytes([CANARY]) * a.nbytes, np.uint8)
    for k, n, ref in (("lengths", G, want["lengths"]), ("move_offset", G + 1, want["move_offset"]),
                      ("frames", want["written"], want["frames"]), ("tokens", want["written"], want["tokens"]),
                      ("rewards", want["written"], want["rewards"])):
        assert np.array_equal(got[k][:n].view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), (what, k)
        rest = np.ascontiguousarray(got[k][n:])
        assert np.array_equal(rest.view(np.uint8).reshape(-1), poison(rest)), (what, k, "written past its end")
    return want


# ---- pack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C, L, T, S", SHAPES)
def test_pack_follows_the_restatement_in_every_ring_state(C, L, T, S):
    rng = np.random.default_rng(C * 31 + S)
    buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)

    def add(B):
        st, po, rw, ln = random_games(rng, B, L, T, S)
        IO.add_games(ring, st, po, rw, ln)
        buf.add_games(dev(st), dev(po), dev(rw), dev(ln))
        mirror(buf, ring)

    check_pack(buf, ring, "empty")
    if C > 1:
        add(C // 2)
        assert 0 < len(ring.slots) < C
        check_pack(buf, ring, "partly filled")
    add(C - C // 2)
    assert len(ring.slots) == C and ring.pointer == 0
    check_pack(buf, ring, "exactly full")
    add(max(1, C // 3))
    assert ring.pointer != 0 or C == 1
    want = check_pack(buf, ring, "wrapped")
    if C > 1:  # oldest first: the dense form starts with the game at ring[0]
        assert np.array_equal(want["frames"][:want["lengths"][0]], ring.slots[ring.pointer][0])
    add(C + 3)
    check_pack(buf, ring, "one add of more than C games")
    check_buffer(buf, ring, "after the packs")
    assert int(buf.status[0]) == 0


def test_pack_of_the_reference_ring_at_s16(golden):
    g = golden("replay_cases")
    st, po, rw, ln = (g[f"ring_S16_T1_{k}"] for k in ("states", "policy", "rewards", "lengths"))
    L, T, S = st.shape[1], st.shape[2], st.shape[3]
    assert (S, T) == (16, 1)
    buf, ring = guarded_buffer(3, L, T, S), RR.Ring(3, L)
    for a in range(len(ln)):
        ring.add(st[a:a + 1], po[a:a + 1], rw[a:a + 1], ln[a:a + 1])
        buf.add_games(dev(st[a:a + 1]), dev(po[a:a + 1]), dev(rw[a:a + 1]), dev(ln[a:a + 1]))
        check_pack(buf, ring, a)
    frames, tokens, rewards, lengths, words = buf.pack()
    assert frames.data_ptr() % 16 == 0 and buf.frames.data_ptr() % 16 == 0  # the 16-byte path
    want = IO.pack(ring, T, S)
    assert np.array_equal(frames.cpu().numpy(), want["frames"]) and np.array_equal(lengths.cpu().numpy(), want["lengths"])
    assert words.tolist() == [ring.pointer, ring.added]


@pytest.mark.parametrize("C, L, T, S", [(3, 4, 2, 4), (5, 3, 1, 3), (4, 3, 1, 9)])
def test_pack_of_a_best_buffer(C, L, T, S):
    rng = np.random.default_rng(C + S)
    buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)
    for call in range(C + 2):
        st, po, rw, ln = random_games(rng, 6, L, T, S)
        ring.add(st, po, rw, ln, select=True)
        buf.add_best(dev(st), dev(po), dev(rw), dev(ln))
        mirror(buf, ring)
        if call in (0, C - 1, C + 1):
            check_pack(buf, ring, ("best", call))
    assert ring.added == C + 2
    check_buffer(buf, ring, "best")


@pytest.mark.parametrize("C, L, T, S", [(3, 4, 2, 4), (5, 3, 1, 3)])
def test_pack_cut_inside_a_game(C, L, T, S):
    rng = np.random.default_rng(7)
    buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)
    st, po, rw, ln = random_games(rng, C + 1, L, T, S)
    ln[:] = [2 + (i % 2) for i in range(C + 1)]
    IO.add_games(ring, st, po, rw, ln)
    buf.add_games(dev(st), dev(po), dev(rw), dev(ln))
    full = IO.pack(ring, T, S)
    M = int(full["counts"][1])
    cut = int(full["move_offset"][2]) + 1  # one row into the third game
    want = check_pack(buf, ring, "cut", max_moves=cut)
    assert want["status"] == IO.TRUNCATED and want["written"] == full["move_offset"][2] and want["counts"][1] == M
    assert check_pack(buf, ring, "nothing fits", max_moves=1)["written"] == 0
    assert check_pack(buf, ring, "no rows", max_moves=0)["status"] == IO.TRUNCATED
    assert check_pack(buf, ring, "exact", max_moves=M)["status"] == 0


# ---- add_packed ------------------------------------------------------------------------------------------------------------
def both_add_packed(buf, ring, frames, tokens, rewards, lengths, M=None, first_slot=-1, games_added=-1):
    """The call on the device and on the restatement; the status bits agree."""
    rows = len(rewards) if M is None else M
    status = torch.zeros((1,), dtype=torch.uint32, device=DEV)
    ops.replay_add_packed(buf, dev(frames[:rows]), dev(tokens[:rows]), dev(rewards[:rows]),
                          dev(np.asarray(lengths, np.int32)), first_slot, games_added, status=status)
    want = IO.add_packed(ring, frames, tokens, rewards, lengths, M=M, first_slot=first_slot, games_added=games_added)
    assert int(status[0]) == want
    return want


@pytest.mark.parametrize("C, L, T, S", SHAPES)
def test_add_packed_follows_the_restatement(C, L, T, S):
    rng = np.random.default_rng(C * 17 + S)
    combos = list(itertools.product((-1, 0, C - 1), (-1, 7)))
    for first_slot, games_added in combos if C <= 1025 else (combos[0], combos[-1]):  # the bound: the two extremes
        what = (first_slot, games_added)
        buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)
        # a ring that already holds games and whose next slot is not 0 (where the capacity allows)
        ln = rng.integers(1, L + 1, size=C // 2 + 1).astype(np.int32)
        both_add_packed(buf, ring, *dense_games(rng, ln, T, S), ln)
        check_buffer(buf, ring, (what, "first"))
        # good games among lengths 0, L + 1 and negative ones: their rows are skipped
        ln = rng.integers(1, L + 1, size=min(C, 9) + 4).astype(np.int32)
        ln[[1, 3, 4]] = [0, L + 1, -2]
        assert both_add_packed(buf, ring, *dense_games(rng, ln, T, S), ln, first_slot=first_slot,
                               games_added=games_added) == IO.BAD_LENGTH
        check_buffer(buf, ring, (what, "bad lengths"))
        # no games: nothing changes
        both_add_packed(buf, ring, *dense_games(rng, np.zeros(0, np.int32), T, S), np.zeros(0, np.int32),
                        first_slot=first_slot, games_added=games_added)
        check_buffer(buf, ring, (what, "G = 0"))
        # more games than slots: the last C stay
        ln = rng.integers(1, L + 1, size=C + 3).astype(np.int32)
        assert both_add_packed(buf, ring, *dense_games(rng, ln, T, S), ln, first_slot=first_slot,
                               games_added=games_added) == 0
        check_buffer(buf, ring, (what, "G > C"))
    # fewer rows than the lengths claim: the games past M are not stored, nothing at or past row M is read
    buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)
    ln = np.full(min(C, 5) + 1, L, np.int32)
    fr, tk, rw = dense_games(rng, ln, T, S)
    M = len(rw) - 1
    assert both_add_packed(buf, ring, fr, tk, rw, ln, M=M) == IO.TRUNCATED
    assert ring.added == len(ln) - 1
    check_buffer(buf, ring, "M short")


def test_add_packed_bad_lengths_and_short_rows_together():
    C, L, T, S = 5, 3, 1, 3
    rng = np.random.default_rng(3)
    buf, ring = guarded_buffer(C, L, T, S), RR.Ring(C, L)
    ln = np.array([2, 0, 3, L + 1, -1, 1, 2], np.int32)
    fr, tk, rw = dense_games(rng, ln, T, S)
    assert both_add_packed(buf, ring, fr, tk, rw, ln, M=len(rw) - 1, first_slot=3, games_added=11) == 3
    assert sorted(ring.slots) == [0, 3, 4] and ring.pointer == 1 and ring.added == 11
    check_buffer(buf, ring, "both bits")


@pytest.mark.parametrize("C, L, T, S", [(3, 4, 2, 4), (5, 3, 1, 3)])
def test_add_packed_equals_replay_add_with_one_hot_policies(C, L, T, S):
    rng = np.random.default_rng(C)
    n_logits = 3
    a, b = guarded_buffer(C, L, T, S), guarded_buffer(C, L, T, S)
    ring = RR.Ring(C, L)
    for G in (2, C, C + 2):  # partly filled, wrapped, more than C in one call
        ln = rng.integers(1, L + 1, size=G).astype(np.int32)
        ln[0] = L
        fr, tk, rw = dense_games(rng, ln, T, S)
        starts = np.concatenate([[0], np.cumsum(ln)])
        st, po, rp = np.zeros((G, L, T, S, S, S), np.int8), np.zeros((G, L, 3 * S, n_logits), np.float32), \
            np.zeros((G, L), np.float32)
        for g in range(G):
            st[g, :ln[g]], rp[g, :ln[g]] = fr[starts[g]:starts[g + 1]], rw[starts[g]:starts[g + 1]]
            po[g, :ln[g]] = np.eye(n_logits, dtype=np.float32)[tk[starts[g]:starts[g + 1]]]
        ops.replay_add(a, dev(st), dev(po), dev(rp), dev(ln.astype(np.int64)))
        ops.replay_add_packed(b, dev(fr), dev(tk), dev(rw), dev(ln))
        IO.add_packed(ring, fr, tk, rw, ln)
        check_buffer(a, ring, ("replay_add", G))  # every valid byte, length, offset and ring: equal to the restatement,
        check_buffer(b, ring, ("add_packed", G))  # and so to each other


@pytest.mark.parametrize("C", RC.EDGE_C)
@pytest.mark.parametrize("N", RC.EDGE_N)
def test_add_packed_at_the_plan_chunk_and_slot_range_edges(N, C):
    RC.check_edges("add_packed", N, C, DEV)


# ---- GameBuffer: pack, save, load ------------------------------------------------------------------------------------------
def wrapped_buffer(C, L, T, S, games, seed=0):
    rng = np.random.default_rng(seed)
    buf, ring = GameBuffer(C, L, T, S, DEV), RR.Ring(C, L)
    st, po, rw, ln = random_games(rng, games, L, T, S)
    for lo in range(0, games, 2):
        IO.add_games(ring, st[lo:lo + 2], po[lo:lo + 2], rw[lo:lo + 2], ln[lo:lo + 2])
        buf.add_games(dev(st[lo:lo + 2]), dev(po[lo:lo + 2]), dev(rw[lo:lo + 2]), dev(ln[lo:lo + 2]))
    return buf, ring, (st, po, rw, ln)


def valid_region_equal(a, b):
    for name in ("length", "offset", "ring"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    keep = (torch.arange(a.L, device=DEV)[None] < a.length[:, None])
    for name in ("frames", "tokens", "rewards"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x[keep].view(torch.uint8), y[keep].view(torch.uint8)), name


@pytest.mark.parametrize("C, L, T, S, games", [(3, 4, 2, 4, 5), (5, 3, 1, 3, 7), (4, 3, 1, 9, 3), (6, 4, 2, 4, 0)])
def test_buffer_round_trip_through_a_file(tmp_path, C, L, T, S, games):
    buf, ring, _ = wrapped_buffer(C, L, T, S, games)
    frames, tokens, rewards, lengths, words = buf.pack()
    want = IO.pack(ring, T, S)
    M = int(want["counts"][1])
    assert frames.shape == (M, T, S, S, S) and tokens.shape == (M, 3 * S) and rewards.shape == (M,)
    assert np.array_equal(lengths.cpu().numpy(), want["lengths"]) and words.tolist() == [ring.pointer, ring.added]
    path = tmp_path / "buffer.tgr"
    buf.save(path)
    assert path.read_bytes() == IO.file_bytes(C, L, T, S, (ring.pointer, ring.added), want["lengths"], want["rewards"],
                                              want["tokens"], want["frames"])
    back = GameBuffer.load(path, DEV)
    assert (back.C, back.L, back.T, back.S) == (C, L, T, S)
    valid_region_equal(back, buf)
    n = len(buf)
    assert len(back) == n == M and back.games_added() == ring.added
    for x, y in zip(back.items(torch.arange(n, device=DEV)), buf.items(torch.arange(n, device=DEV))):
        assert torch.equal(x, y)
    assert int(back.status[0]) == 0 and int(buf.status[0]) == 0
    if games:
        with pytest.raises(ValueError, match="max_actions"):
            GameBuffer.load(path, DEV, max_actions=int(want["lengths"].max()) - 1)


def test_load_into_a_smaller_capacity_keeps_the_newest_games(tmp_path):
    C, L, T, S = 3, 4, 2, 4
    buf, ring, (st, po, rw, ln) = wrapped_buffer(C, L, T, S, 5)
    assert ring.pointer != 0 and len(ring.slots) == 3
    buf.save(tmp_path / "b.tgr")
    small = GameBuffer.load(tmp_path / "b.tgr", DEV, capacity=2)
    want = GameBuffer(2, L, T, S, DEV)
    want.add_games(dev(st[3:5]), dev(po[3:5]), dev(rw[3:5]), dev(ln[3:5]))
    valid_region_equal(small, want)
    n = len(want)
    for x, y in zip(small.items(torch.arange(n, device=DEV)), want.items(torch.arange(n, device=DEV))):
        assert torch.equal(x, y)
    large = GameBuffer.load(tmp_path / "b.tgr", DEV, capacity=7, max_actions=L + 2)  # and into a larger one
    grown = GameBuffer(7, L + 2, T, S, DEV)
    pad = lambda x: np.concatenate([x, np.zeros_like(x[:, :2])], axis=1)
    grown.add_games(dev(pad(st[2:5])), dev(pad(po[2:5])), dev(pad(rw[2:5])), dev(ln[2:5]))
    valid_region_equal(large, grown)


# ---- graph capture ----------------------------------------------------------------------------------------------------------
def test_captured_pack_and_add_packed_equal_eager():
    C, L, T, S = 8, 4, 2, 4
    rng = np.random.default_rng(5)
    src, _, _ = wrapped_buffer(C, L, T, S, 11, seed=2)
    M, G = len(src), C  # 11 games: the ring is full
    ln = rng.integers(1, L + 1, size=5).astype(np.int32)
    fr, tk, rw = (dev(x) for x in dense_games(rng, ln, T, S))
    ln = dev(ln)
    outs = [[t.zero_() for t in ops.replay_pack(src, M)] for _ in (0, 1)]  # frames, tokens, rewards, lengths, ...
    dst = [GameBuffer(C, L, T, S, DEV) for _ in (0, 1)]

    def run(k):
        ops.replay_pack(src, M, *outs[k])
        ops.replay_add_packed(dst[k], outs[k][0], outs[k][1], outs[k][2], outs[k][3][:G], first_slot=2)
        ops.replay_add_packed(dst[k], fr, tk, rw, ln)

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        run(0)
        run(1)  # warm-up of both, outside capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    for k in (0, 1):
        for t in outs[k]:
            t.zero_()
        for name in ARRAYS:
            getattr(dst[k], name).zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # capture runs nothing
        run(0)
    assert not outs[0][5].any()
    graph.replay()
    run(1)
    torch.cuda.synchronize()
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for name in ARRAYS:
        assert torch.equal(getattr(dst[0], name).view(torch.uint8), getattr(dst[1], name).view(torch.uint8)), name
    assert dst[0].ring.tolist() == [(2 + G + 5) % C, G + 5] and outs[0][5].tolist() == [G, M]


# ---- TensorGameData ---------------------------------------------------------------------------------------------------------
def small_data(seed):
    L = 6
    demos = SyntheticDemos(L, 64, 2, 4, DEV, seed=9)
    data = TensorGameData.from_demos(demos, 96, 0.6, seed=seed, played_capacity=5, best_capacity=2)
    rng = np.random.default_rng(5)
    st, po, rw, ln = random_games(rng, 9, L, 2, 4)
    data.played.add_games(dev(st[:7]), dev(po[:7]), dev(rw[:7]), dev(ln[:7]))  # wraps
    data.best.add_games(dev(st[7:]), dev(po[7:]), dev(rw[7:]), dev(ln[7:]))
    data.set_fractions(0.6, 0.2)
    data.resample_buffer_indexes()
    return data


@pytest.mark.parametrize("with_demos", [True, False])
def test_dataset_round_trip_gives_the_same_batches(tmp_path, with_demos):
    data = small_data(3)
    path = tmp_path / "data.tgd"
    data.save(path, demos=with_demos)
    if with_demos:
        back = TensorGameData.load(path, DEV)
        with pytest.raises(ValueError, match="holds its demos"):
            TensorGameData.load(path, DEV, tokens=data.tokens, targets=data.targets)
    else:
        with pytest.raises(ValueError, match="holds no demos"):
            TensorGameData.load(path, DEV)
        wrong = data.targets.clone()
        wrong[3, 0, 0, 0] += 1
        with pytest.raises(ValueError, match="not the ones"):
            TensorGameData.load(path, DEV, tokens=data.tokens, targets=wrong)
        with pytest.raises(ValueError, match="must be"):
            TensorGameData.load(path, DEV, tokens=data.tokens[:-1], targets=data.targets[:-1])
        back = TensorGameData.load(path, DEV, tokens=data.tokens, targets=data.targets)
    assert torch.equal(back.kind, data.kind) and torch.equal(back.src, data.src)
    assert (back.fract_synth, back.fract_best, back.len_data) == (data.fract_synth, data.fract_best, data.len_data)
    valid_region_equal(back.played, data.played)
    valid_region_equal(back.best, data.best)
    for epoch in range(2):
        if epoch:
            data.resample_buffer_indexes()
            back.resample_buffer_indexes()
            assert torch.equal(back.kind, data.kind) and torch.equal(back.src, data.src)
        gens = [torch.Generator(device=DEV).manual_seed(4 + epoch) for _ in (0, 1)]
        for x, y in zip(data.batches(8, generator=gens[0]), back.batches(8, generator=gens[1])):
            assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(x, y))
    assert int(back.status[0]) == 0 and int(data.status[0]) == 0
    assert {0, 2} <= set(data.kind.tolist())  # synthetic and best rows (the reference's split sends none to played)


# ---- a saved and resumed run ---------------------------------------------------------------------------------------------------
RESUME_CFG = dict(CONFIGS["b"], dim_3d=4, n_steps=12)


@functools.lru_cache(maxsize=None)
def resume_weights():
    return make_weights(RESUME_CFG, 41)


def fresh_run():
    S, T, max_actions = 4, 1, 4
    tr = FusedTrainer.from_state_dict(resume_weights(), dropout_p=0.5, seed=6, device=DEV)
    opt = torch.optim.AdamW([tr.params], lr=1e-3)
    demos = SyntheticDemos(max_actions, 32, T, S, DEV, seed=1)
    data = TensorGameData.from_demos(demos, 32, 0.5, seed=2, played_capacity=12, best_capacity=2)
    gen = torch.Generator(device=DEV).manual_seed(8)
    return tr, opt, data, gen


def run_epoch(tr, opt, data, gen, epoch):
    S, T, B, max_actions = 4, 1, 8, 4
    data.resample_buffer_indexes()
    losses = []
    for batch in itertools.islice(data.batches(8, generator=gen), 2):
        losses += list(tr.train_step(batch, opt))
    start = torch.from_numpy(np.random.default_rng(epoch).integers(-1, 2, size=(B, T, S, S, S)).astype(np.int8)).to(DEV)
    states, policy, rewards, lengths = search.actor_prediction(tr.net().policy(seed=epoch), start, max_actions, n_sim=4,
                                                               n_bar=100, n_logits=3, k=tr.n_samples)
    data.add_act_step(states, policy, rewards, lengths)
    return torch.stack(losses)


def test_a_resumed_run_equals_the_uninterrupted_one(tmp_path):
    a = fresh_run()
    run_epoch(*a, 0)
    want_losses = run_epoch(*a, 1)

    b = fresh_run()
    run_epoch(*b, 0)
    replay_io.save_run(tmp_path / "run", b[0], b[1], b[2], generators={"loader": b[3]}, extra={"epoch": 1})
    del b
    run = replay_io.load_run(tmp_path / "run", DEV)
    tr, data, gen = run.trainer, run.data, run.generators["loader"]
    opt = torch.optim.AdamW([tr.params], lr=1e-3)
    opt.load_state_dict(run.optimizer_state)
    assert run.extra == {"epoch": 1} and tr.calls == 2 and tr.seed == 6 and tr.dropout_p == 0.5
    got_losses = run_epoch(tr, opt, data, gen, run.extra["epoch"])

    assert torch.equal(got_losses.view(torch.int32), want_losses.view(torch.int32))
    assert torch.equal(tr.params.detach().view(torch.int32), a[0].params.detach().view(torch.int32))
    assert torch.equal(tr.net().w.view(torch.int32), a[0].net().w.view(torch.int32))
    valid_region_equal(data.played, a[2].played)
    valid_region_equal(data.best, a[2].best)
    assert data.played.games_added() == 16 and int(data.played.ring[0]) == 4  # the ring of 12 has wrapped
    assert torch.equal(data.kind, a[2].kind) and torch.equal(data.src, a[2].src)
    assert set(data.kind.tolist()) > {0}  # the second epoch trained on played games too
    assert torch.isfinite(want_losses).all()
