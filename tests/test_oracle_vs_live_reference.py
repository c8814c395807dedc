"""The reference's functions on seeded random inputs (tests/golden/reference_random_cases.npz, recorded by running the
reference: make_golden_reference_runs.py) against the oracle -- a check on top of the hand-picked step_cases.  CPU only."""
import numpy as np
import pytest

from oracle import tensor_game as O


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_matches_live_reference(golden, seed):
    g = golden("reference_random_cases")
    for case in range(12):
        tag = f"s{seed}_c{case}_"
        # the dtypes the reference was called with: float32 states, int64 tokens
        st, ac = g[tag + "state"].astype(np.float32), g[tag + "actions"].astype(np.int64)
        kids = np.stack(O.get_child_states(st, ac), axis=1)
        assert np.array_equal(kids, g[tag + "kids"]), case
        done = np.stack([O.done_per_game(kids[:, i, 0]) for i in range(ac.shape[1])], axis=1)
        assert np.array_equal(done, g[tag + "done"])
        assert O.remove_null_actions(st, [kids[:, i] for i in range(ac.shape[1])]) == g[tag + "nonnull"].tolist()
        assert np.array_equal(O.take_actions(list(ac[0]), st[0, 0]), g[tag + "taken"])
        assert np.array_equal(O.action_to_tensor(ac), g[tag + "a2t"])
        assert np.array_equal(O.slice_rank_exact(st[:, 0]), g[tag + "rank"])
        # the int8 build semantics agree with the reference wherever nothing overflows
        kids8, done8, chg8, ovf8 = O.expand_i8(st[:, 0].astype(np.int8), ac.astype(np.int8))
        assert not ovf8.any() and np.array_equal(kids8, g[tag + "kids"][:, :, 0]) and np.array_equal(done8, g[tag + "done"])
    for n in (2, 3, 4, 5):
        assert np.array_equal(O.build_matmul_tensor(2, n, n, n), g[f"s{seed}_mm{n}"])
