"""The batches that tests/test_gpu_stream_edges.py and the walk script of tests/test_gpu_ab_library.py hand to the resident
steppers really contain what they are meant to: a condition on the INPUTS, checked on the oracle trajectory alone.

The unit is the 16-byte chunk of the flat game (a slice at S = 4, a row at S = 16, a chunk at S = 25); at S = 4 the same
classes are also counted on the whole-game norm ("game"), at S = 25 on the tail chunk and on the chunks that straddle two
rows.  |-128| counts as 128.  A step is small when all of the game's token bytes are in 0..3; a unit is fast at step k when
the step is small, 0 <= shift <= 3 and the unit's norm before the step is <= limit = 127 - max(shift, 3 - shift)^3.
    rise                 a fast unit that changed and whose new norm exceeds the limit
    return               a non-fast unit that changed, is back within the limit, and changes again in a small next step
    at_limit, one_above  the norm before a small, changing step is limit / limit + 1
    fast_after_overflow  a fast, changing unit of a game that raised overflow at an earlier step
    minus128             -128 in the unit before a small, changing step
    overflow_after_rise  a small step takes a byte beyond int8 in a unit whose previous change was a rise: the only way a
                         precondition left standing after a digit-form step shows in the bytes
    done_fallback        done[k] set by a step that changed the game with some changed unit not fast
    done_digit           ... with every changed unit fast
    done_undone_done     done[k] set again after the game had been done and then not done
    tight                an entry alone in its unit that a (small) step lands on -129 / -128 / 127 / 128
Every class the shift admits must occur at least four times, and overflow must be raised in some games but not all."""
import numpy as np
import pytest

import stream_walk as W
from oracle import tensor_game as O

CASES = [(S, B, K, shift) for S, B, K in W.GPU_CASES for shift in W.SHIFTS]
# the walk script of test_gpu_ab_library.py: the tiled kinds at B = 200 (and its prefixes) on the lane and team kernels,
# and the batch tiled across s4_stream_kernel<2>'s units
CASES += [(4, 200, 19, shift) for shift in W.SHIFTS] + [(4, 203, 11, 1), (4, 203, 11, 0)]


@pytest.mark.parametrize("S,B,K,shift", CASES)
def test_gpu_batches_hold_every_class(S, B, K, shift):
    st, ac = W.make_walk(S, B, K, shift, W.walk_seed(S, shift))
    assert st.dtype == np.int8 and st.shape == (B, S, S, S) and ac.dtype == np.int8 and ac.shape == (K, B, 3 * S)
    c = W.census(S, shift, st, ac)
    assert W.census_shortfalls(S, shift, c) == [], c


@pytest.mark.parametrize("shift", W.SHIFTS)
def test_lane_layout_holds_every_class_by_the_whole_game_norm(shift):
    """The lane layout of the A/B walk script, one edge walk per wavefront of 64 that leaves the digit form and comes back:
    four of every class the shift admits, as for every other batch -- by the unit, by the whole-game norm, the done
    classes and the tight landings -- and wavefronts that are dragged into the general form and return."""
    st, ac = W.make_walk(4, 200, 19, shift, W.walk_seed(4, shift), lanes=True)
    c = W.census(4, shift, st, ac)
    assert W.census_shortfalls(4, shift, c) == [], c
    if W.digits_limit(shift) >= 0:  # most games are in the digit form at most steps: they can be dragged along
        lim, small = W.digits_limit(shift), ((ac >= 0) & (ac <= 3)).all(axis=2)
        norm0 = np.abs(st.astype(np.int64)).reshape(200, -1).sum(axis=1)
        assert (norm0 <= lim).mean() > 0.8 and small.mean() > 0.8
        # per wavefront and step: is every game of the 64 in the digit form?  Both answers, and the way back, must occur
        cur, fast = st.copy(), np.zeros((19, 4), bool)
        for k in range(19):
            ok = small[k] & (np.abs(cur.astype(np.int64)).reshape(200, -1).sum(axis=1) <= lim)
            fast[k] = [ok[64 * w:64 * w + 64].all() for w in range(4)]
            cur = O.step_i8(cur, ac[k], shift)[0]
        assert fast.sum() >= 8 and (~fast).sum() >= 8 and (~fast[:-1] & fast[1:]).sum() >= 4, fast.astype(int).T


def test_census_counts_a_hand_made_walk():
    """One S = 4 game, shift 1 (limit 119), a single entry walked by one-hot actions: the classes by hand."""
    S, shift = 4, 1
    st = np.zeros((1, S, S, S), np.int8)
    st[0, 0, 0, 0] = 119
    hot = lambda a, b=1: W._one_hot(S, shift, 0, (a, b, 1))
    ac = np.stack([hot(-1),        # 119 -> 120: at the limit, fast, rises
                   hot(2),         # 120 -> 118: one above, not fast, returns (the next step changes it again)
                   hot(-1, 2),     # 118 -> 120: fast, rises
                   hot(-8),        # 120 -> 128: wide (token -7), wraps to -128, overflow
                   hot(-1),        # -128 -> -127: small, -128 present, not fast
                   W._null(S, shift, np.random.default_rng(0))])[:, None, :]
    c = W.census(S, shift, st, ac)
    for scope in ("unit", "game"):
        got = {k: c[scope][k] for k in W.UNIT_CLASSES}
        assert got == {"rise": 2, "return": 1, "at_limit": 1, "one_above": 1, "fast_after_overflow": 0, "minus128": 1,
                       "overflow_after_rise": 0}, (scope, got)
    # (the landing on 128 was not small)
    assert c["tight"] == {-129: 0, -128: 0, 127: 0, 128: 0} and c["overflow_games"] == 1
    st[0, 0, 0, 0] = 120
    c = W.census(S, 2, st, np.stack([W._one_hot(S, 2, 0, (-2, -2, -2))])[:, None, :])
    assert c["tight"][128] == 1 and c["unit"]["one_above"] == 1 and c["unit"]["rise"] == 0
    st[0, 0, 0, 0] = 119   # 119 -> 127 (rise) -> 131: overflow right after the rise
    c = W.census(S, 2, st, np.stack([W._one_hot(S, 2, 0, (-2, -2, -2)), W._one_hot(S, 2, 0, (-2, -2, -1))])[:, None, :])
    assert c["unit"]["rise"] == 1 and c["unit"]["overflow_after_rise"] == 1 and c["game"]["overflow_after_rise"] == 1


@pytest.mark.parametrize("shift", W.SHIFTS)
def test_tight_pairs_are_what_the_factor_range_reaches(shift):
    f = W.small_factors(shift)
    reach = {T for T in W.TIGHT_VALUES for a in f for b in f for c in f if a * b * c != 0 and -128 <= T + a * b * c <= 127}
    assert {T for T, _ in W.tight_pairs(shift)} == reach
    assert reach == {0: {-129, -128}, 3: {127, 128}}.get(shift, set(W.TIGHT_VALUES))
    for T, p in W.tight_pairs(shift):
        st = np.zeros((1, 4, 4, 4), np.int8)
        st[0, 0, 0, 0] = T + p
        new, _, ovf = O.step_i8(st, W._one_hot(4, shift, 0, W._products(shift)[p])[None], shift)
        assert int(new[0, 0, 0, 0]) == np.int64(T).astype(np.int8) and int(ovf[0]) == (T in (-129, 128))
