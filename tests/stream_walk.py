"""Inputs for the resident steppers of tg_step_stream_i8 (tg_stream.h) that sit on the edges of the digit form, and a
census of what a batch really contains.  Pure numpy on top of the oracle: no GPU.

The digit form of a step is exact only while every token byte of the step is in 0..3, 0 <= shift <= 3 and the L1 norm of
the 16-byte unit (a slice at S = 4, a row at S = 16, a chunk of the flat game at S = 25; |-128| counts as 128) is at most
127 - F^3, F = max(shift, 3 - shift).  The steppers carry that norm from step to step, so a batch that is to tell a correct
stepper from a subtly wrong one has to cross the limit in both directions DURING a run, sit exactly on it, raise overflow
and go on in the digit form, finish a game in either form, and so on.  ``make_walk`` builds such a batch by simulating every
scripted game with the oracle; ``census`` counts the events from the oracle trajectory alone, and
``census_shortfalls`` names the classes a batch has too few of (tests/test_stream_walk_cpu.py holds every batch the GPU
tests use to it).

The tight values.  An entry e alone in its unit and a small-token action land e - u_i v_j w_l on -129, -128, 127 or 128;
with factors in [-shift, 3 - shift] the product p = u_i v_j w_l decides what is reachable (p != 0, e = value + p in int8):
    shift 0  (factors  0..3, p in {1,2,3,4,6,8,9,12,18,27}):  -129, -128            (127 / 128 would need p < 0)
    shift 1  (factors -1..2, p in {-4,-2,-1,1,2,4,8}):        -129, -128, 127, 128
    shift 2  (factors -2..1, p in {-8,-4,-2,-1,1,2,4}):       -129, -128, 127, 128
    shift 3  (factors -3..0, p in the negatives of shift 0):              127, 128  (-129 / -128 would need p > 0)
    other shifts (factors -1..2, every step in the fallback):  -129, -128, 127, 128
Only 128 turns an off-by-one in the limit into a carry: e = limit + 1 with p = -F^3 (shifts 2 and 3; at shifts 0 and 1 no
product reaches -F^3, and on the negative side -(limit + 1) - F^3 = -128 is still a digit).  The tight games put that
pair first.

A precondition left standing after a digit-form step (a stale bit, a norm not recomputed) shows in the bytes only when a
later small step really takes a byte beyond int8, so the edge walks also hold climbs: an entry at limit - r that the
largest small product takes to 127 - r (a rise out of the digit form) and the next step beyond int8 -- on a byte that is
not the top byte of its dword, where the carry would fall off the end (census class overflow_after_rise)."""
import numpy as np

from oracle import tensor_game as O

SHIFTS = (0, 1, 2, 3, -1, 4)
TIGHT_VALUES = (-129, -128, 127, 128)
# the batches of tests/test_gpu_stream_edges.py: (S, B, K); B = 203 leaves the last S = 4 team of 16 games with 5 dead lanes
GPU_CASES = ((4, 203, 19), (16, 36, 19), (25, 24, 19))
KIND_TILE = ("plain", "edge", "edge_wide", "tight", "demo", "done_undone_done", "int8_edge", "edge_wide")
BURST = 3                                      # consecutive steps an edge walk spends on one unit
WALK = (0, 1, -1, 0, 2, -2, 1, 0, 3, -1)       # the unit norms an edge walk heads for, relative to the limit


def walk_seed(S, shift):
    return 1000 * S + 10 * (shift + 1)


def digits_limit(shift):
    """s4_digits_limit: the largest unit norm the digit form accepts, -1 when the shift rules it out."""
    F = max(shift, 3 - shift)
    return 127 - F ** 3 if 0 <= shift <= 3 else -1


def small_factors(shift):
    """The factors whose tokens are in 0..3; for a shift outside 0..3 (no digit form at all) -1..2."""
    return list(range(-shift, 4 - shift)) if 0 <= shift <= 3 else [-1, 0, 1, 2]


def _products(shift):
    """product -> one factor triple (a, b, c) with a b c = product, over the small factors (non-zero products only)."""
    f = [x for x in small_factors(shift) if x != 0]
    out = {}
    for a in f:
        for b in f:
            for c in f:
                out.setdefault(a * b * c, (a, b, c))
    return out


def _unit_info(S):
    n = S ** 3
    nu = -(-n // 16)
    tail = [nu - 1] if n % 16 else []
    straddle = [u for u in range(nu) if S == 25 and u not in tail and (16 * u) % 25 > 9]
    return n, nu, tail, straddle


def _tok(S, shift, hot=()):
    """Tokens of a rank-1 action whose factors are zero except ``hot`` = ((position in 0..3S, factor), ...)."""
    t = np.full(3 * S, shift, np.int64)
    for pos, f in hot:
        t[pos] = shift + f
    assert t.min() >= -128 and t.max() <= 127
    return t.astype(np.int8)


def _one_hot(S, shift, flat, triple):
    i, r = divmod(flat, S * S)
    j, l = divmod(r, S)
    return _tok(S, shift, ((i, triple[0]), (S + j, triple[1]), (2 * S + l, triple[2])))


def _sparse_small(S, shift, rng, hit=None, density=0.3, unit=False):
    """A sparse action with small factors (``unit``: of magnitude 1); u, v and w each get a non-zero factor; ``hit`` =
    flat byte that must change."""
    nzf = [x for x in small_factors(shift) if x != 0 and (abs(x) == 1 or not unit)]
    f = np.where(rng.random(3 * S) < density, rng.choice(nzf, size=3 * S), 0)
    for part in range(3):
        if not f[part * S:(part + 1) * S].any():
            f[part * S + rng.integers(0, S)] = rng.choice(nzf)
    if hit is not None:
        i, r = divmod(hit, S * S)
        j, l = divmod(r, S)
        for pos in (i, S + j, 2 * S + l):
            if f[pos] == 0:
                f[pos] = rng.choice(nzf)
    return (f + shift).astype(np.int8)


def _null(S, shift, rng):
    """u = 0: nothing changes, whatever v and w are."""
    t = _sparse_small(S, shift, rng)
    t[:S] = shift
    return t


def _apply(cur, tok, shift):
    return O.step_i8(cur[None], tok[None], shift)[0][0]


def _live(S, u):
    return min(16, S ** 3 - 16 * u)


# ---------------------------------------------------------------------------------------------- the kinds of game
def _plain(S, K, shift, rng, calm=False):
    if calm:  # (the lane layout's neighbours: a small whole-game norm, every step in the digit form where the shift allows)
        st = rng.choice([-1, 0, 0, 0, 1], size=(S, S, S)).astype(np.int8)
        return st, np.stack([_sparse_small(S, shift, rng, density=0.2, unit=True) for _ in range(K)])
    st = rng.integers(-2, 3, size=(S, S, S)).astype(np.int8)
    ac = (rng.choice([-1, 0, 1], p=[0.15, 0.7, 0.15], size=(K, 3 * S)) + shift).astype(np.int8)
    return st, ac


def _walk_tok(S, shift, cur, u, want, prods, rng, dense):
    """One small action that takes unit u's norm as near to ``want`` as a single byte and one product can, changing it."""
    xs = cur.reshape(-1)[16 * u:16 * u + _live(S, u)].astype(np.int64)
    d = want - int(np.abs(xs).sum())
    best, pick = None, []
    for o, x in enumerate(xs):
        for p in prods:
            new = int(x) - p
            if -128 <= new <= 127:
                miss = abs(abs(new) - abs(int(x)) - d)
                if best is None or miss < best:
                    best, pick = miss, []
                if miss == best:
                    pick.append((o, p))
    o, p = pick[rng.integers(0, len(pick))]
    tok = _one_hot(S, shift, 16 * u + o, prods[p])
    if dense:  # the other entries of u: the same byte of other units moves too (the walk is simulated, so it stays exact)
        i = (16 * u + o) // (S * S)
        f = rng.choice(small_factors(shift), size=S)
        f[i] = prods[p][0]
        tok[:S] = (f + shift).astype(np.int8)
    return tok


def _wrap_tok(S, shift, cur, u, lim, rng):
    """A WIDE sparse action: the largest byte of unit u overflows and wraps to a small value, the rest of the game stays."""
    xs = cur.reshape(-1)[16 * u:16 * u + _live(S, u)].astype(np.int64)
    o = int(np.argmax(np.abs(xs)))
    x = int(xs[o])
    sx = 1 if x >= 0 else -1
    q = 256 - abs(x) - int(rng.integers(0, max(2, lim - 20)))
    qb = -(-q // 120)
    qa = q // qb                                   # the byte becomes x + sx qa qb, beyond int8 by construction
    assert abs(x) + qa * qb > 128 and qa > 3
    return _one_hot(S, shift, 16 * u + o, (-sx * qa, qb, 1))


def _climb(shift):
    """(sign of the entry, product of the rise, product of the overflow): an entry of that sign at limit - r, r <= 1, is
    taken by the largest small product to 127 - r in magnitude (the unit was in the digit form and leaves it) and by the next one
    beyond int8 -- a stepper that still believes the unit to be in the digit form carries into the neighbouring byte."""
    prods = _products(shift)
    rise = max(prods, key=abs)
    sgn = 1 if rise > 0 else -1
    assert 4 * sgn in prods and -rise not in prods
    return -sgn, rise, 4 * sgn


def _walk_limit(shift):
    """The norm the scripted games walk along: the digit form's limit, 119 where the shift has none."""
    return digits_limit(shift) if digits_limit(shift) >= 0 else 119


def _edge_units(S, g, rng, single, climb):
    """(the units an edge walk visits, the units that hold a climb).  S = 25: the tail chunk, two chunks that straddle
    two rows and one that does not, in an order that turns with g; the climbs are in a third straddling chunk and, in
    every other game, in the tail chunk as well (before its walk).  S = 4 / 16: 3 / 5 units, the last one kept for the
    climb.  ``single``: one unit for both, with a climb only where ``climb`` says so."""
    n, nu, tail, straddle = _unit_info(S)
    if S == 25:
        units = tail + [straddle[int(x)] for x in rng.choice(len(straddle), 3, replace=False)]
        units.append(int(rng.choice([u for u in range(nu - 1) if u not in straddle])))
        climbers = (tail if g % 2 == 0 else []) + [units.pop(1)]
        turn = g % len(units)
        return units[turn:] + units[:turn], climbers
    units = [int(x) for x in rng.choice(nu, 1 if single else (3 if S == 4 else 5), replace=False)]
    if single:
        return units, units[:1] if climb else []
    climber = units.pop()
    return units, [climber]


def _script_climbs(S, shift, st, climbers, first, taken, rng):
    """{step: action}: for each climber two steps in a row on one byte, from step ``first`` on and clear of the steps in
    ``taken``.  The byte (not the top byte of its dword, where a carry would fall off the end) is set in the flat state
    ``st`` and the rest of its unit cleared."""
    lim, prods = _walk_limit(shift), _products(shift)
    sign, p_rise, p_over = _climb(shift)
    script, at = {}, first
    for u in climbers:
        while {at, at + 1} & (set(taken) | set(script)):
            at += 1
        flat = 16 * u + int(rng.choice([o for o in range(_live(S, u)) if o % 4 != 3]))
        st[16 * u:16 * u + _live(S, u)] = 0
        st[flat] = sign * (lim - int(rng.integers(0, 2)))
        script[at], script[at + 1] = _one_hot(S, shift, flat, prods[p_rise]), _one_hot(S, shift, flat, prods[p_over])
        at += 5
    return script


def _edge(S, K, shift, rng, g, wide, single, climb):
    """An edge walk: single entries at limit + r, r in -2..2, in a few units of an empty game; every BURST steps the
    walk turns to the next unit and takes its norm to the next value of WALK.  ``wide``: full-range tokens at two steps
    in the middle of a block.  The climbs of _script_climbs take their two steps each out of the walk."""
    n = S ** 3
    lim, prods = _walk_limit(shift), _products(shift)
    wide_at = {2 + g % 2: "wrap", 10 + g % 3: "full" if g % 4 == 3 else "wrap"} if wide else {}
    units, climbers = _edge_units(S, g, rng, single, climb)
    st = np.zeros(n, np.int8)
    for u in units:
        sg = {0: 1, 3: -1}.get(shift, int(rng.choice([-1, 1])))  # the sign that small products can bring back down
        st[16 * u + rng.integers(0, _live(S, u))] = np.clip(sg * (lim + int(rng.integers(-2, 3))), -128, 127)
    first = 0 if single or (S == 25 and g % 2 == 0) else 4 + g % 7
    script = _script_climbs(S, shift, st, climbers, first, wide_at, rng)
    st = st.reshape(S, S, S)
    cur, ac, pos = st.copy(), np.zeros((K, 3 * S), np.int8), {u: 0 for u in units}
    for k in range(K):
        u = units[(k // BURST) % len(units)]
        if k in script:
            ac[k] = script[k]
        elif wide_at.get(k) == "full":
            ac[k] = rng.integers(-128, 128, size=3 * S)
        elif wide_at.get(k) == "wrap":
            ac[k] = _wrap_tok(S, shift, cur, u, lim, rng)
        else:
            norm = int(np.abs(cur.reshape(-1)[16 * u:16 * u + _live(S, u)].astype(np.int64)).sum())
            while lim + WALK[pos[u] % len(WALK)] == norm:
                pos[u] += 1
            dense = not single and rng.random() < 0.6
            ac[k] = _walk_tok(S, shift, cur, u, lim + WALK[pos[u] % len(WALK)], prods, rng, dense)
            pos[u] += 1
        cur = _apply(cur, ac[k], shift)
    return st, ac


def tight_pairs(shift):
    """(value, product) with e = value + product an int8 entry: what a small action can land on, hardest pair first."""
    prods = _products(shift)
    pairs = [(T, p) for T in TIGHT_VALUES for p in prods if -128 <= T + p <= 127]
    return sorted(pairs, key=lambda tp: (-abs(tp[1]), -tp[0]))


def _tight(S, K, shift, rng, g, single):
    n, nu, tail, straddle = _unit_info(S)
    prods, pairs = _products(shift), tight_pairs(shift)
    if S == 25:
        units = (tail if g % 2 == 0 else []) + [straddle[int(x)] for x in rng.choice(len(straddle), 5, replace=False)]
        units += [int(x) for x in rng.choice([u for u in range(nu - 1) if u not in straddle], 2, replace=False)]
    else:
        units = [int(x) for x in rng.choice(nu, 1 if single else min(nu, 7), replace=False)]
    st, ac = np.zeros(n, np.int8), []
    for idx, u in enumerate(units):
        T, p = pairs[(g * len(units) + idx) % len(pairs)]
        # (a landing beyond int8 not on the top byte of its dword: a carry there would fall off the end unseen)
        flat = 16 * u + int(rng.choice([o for o in range(_live(S, u)) if o % 4 != 3 or -128 <= T <= 127]))
        st[flat] = T + p
        ac.append(_one_hot(S, shift, flat, prods[p]))
    # the rest: sparse small steps on a game that has raised overflow -- at S = 25 half of them through the tail chunk
    while len(ac) < K:
        hit = n - 1 - int(rng.integers(0, 9)) if S == 25 and rng.random() < 0.5 else None
        ac.append(_sparse_small(S, shift, rng, hit=hit, density=0.1))
    return st.reshape(S, S, S), np.stack(ac[:K])


def _tight_again(S, K, shift, rng, g):
    """The tight game of the lane layout: ONE entry in the whole game, so that it is alone in its unit and in the game,
    and every step a one-hot small action on it.  The first step lands pair g of tight_pairs; from then on the entry
    heads for the next reachable value in the order 127, 128 (wraps to -128), -128, -129 (wraps to 127), lands on it as
    soon as one product does and otherwise takes the product that brings it nearest without leaving int8.  With
    products of both signs that is a landing on each value every six steps; at shifts 0 and 3 the entry has to cross
    the whole of int8 between two pairs of landings, about ten steps of the largest product."""
    prods, pairs = _products(shift), tight_pairs(shift)
    order = [T for T in (127, 128, -128, -129) if T in {T for T, _ in pairs}]
    T, p = pairs[g % len(pairs)]
    flat = int(rng.choice([o for o in range(S ** 3) if o % 4 != 3]))   # (not the top byte of its dword, as in _tight)
    st = np.zeros(S ** 3, np.int8)
    st[flat] = T + p
    ac, v = [], T + p
    for _ in range(K):
        if ac:
            T = order[(order.index(T) + 1) % len(order)]
            inside = [q for q in prods if -128 <= v - q <= 127] or list(prods)
            p = v - T if v - T in prods else min(inside, key=lambda q: (abs(v - q - T), q))
        landed = v - p == T
        ac.append(_one_hot(S, shift, flat, prods[p]))
        v = int(np.int64(v - p).astype(np.int8))
        if not landed:       # still on the way: the same value next time
            T = order[order.index(T) - 1]
    return st.reshape(S, S, S), np.stack(ac)


def _demo(S, K, shift, rng, g):
    """The state is the sum of its K action tensors, one step is wide (the last one in every other game)."""
    n = S ** 3
    wide_at = K - 1 if g % 2 else int(rng.integers(1, K - 1))
    for attempt in range(50):
        ac = np.stack([_sparse_small(S, shift, rng, hit=n - 1 - int(rng.integers(0, 9)) if k == K - 1 else None,
                                     density=0.25 / (1 + attempt)) for k in range(K)])
        pos = [int(rng.integers(0, S)) + part * S for part in range(3)]
        ac[wide_at] = _tok(S, shift, tuple(zip(pos, (int(rng.choice([-7, -5, 4, 6])), int(rng.choice([-2, 3])), 1))))
        if wide_at == K - 1:
            u_hot = (S - 1, int(rng.choice([-7, -5, 4, 6])))
            ac[wide_at] = _tok(S, shift, (u_hot, (2 * S - 1, -2), (3 * S - 1 - int(rng.integers(0, 9)) % S, 1)))
        total = O.action_to_tensor(ac, shift).sum(axis=0)
        if np.abs(total).max() <= 127:
            return total.astype(np.int8), ac
    raise AssertionError("demonstration does not fit int8")


def _done_undone_done(S, K, shift, rng, g):
    """state = tensor of action 0 (done at step 0); later an action and then its inverse (u negated), again and again."""
    n = S ** 3
    f = [x for x in small_factors(shift) if x != 0 and (-x in small_factors(shift) or not 0 < shift < 3)]
    ac = [_sparse_small(S, shift, rng, hit=n - 1 - int(rng.integers(0, 9)), density=0.15)]
    st = O.action_to_tensor(ac[0], shift).astype(np.int8)
    cyc = 0
    while len(ac) < K:
        for _ in range((g + cyc) % 3):
            ac.append(_null(S, shift, rng))
        a = _sparse_small(S, shift, rng, hit=n - 1 - int(rng.integers(0, 9)), density=0.15)
        u = a[:S].astype(np.int64) - shift
        if (g + cyc) % 2:                           # factors beyond the small range: this pair is wide at every shift
            u = u * int(rng.choice([4, 5]))
        else:                                       # u that stays small when negated, where the shift has such factors
            u = np.where(u != 0, rng.choice(f, size=S), 0)
        inv = a.copy()
        a[:S] = (u + shift).astype(np.int8)
        inv[:S] = (-u + shift).astype(np.int8)
        ac += [a] + [_null(S, shift, rng) for _ in range(cyc % 2)] + [inv]
        cyc += 1
    return st, np.stack(ac[:K])


def _int8_edge(S, K, shift, rng):
    n = S ** 3
    st = rng.choice([-128, 127, 0, 1], size=(S, S, S)).astype(np.int8)
    ac = [_sparse_small(S, shift, rng, hit=n - 1 - int(rng.integers(0, 9)) if S == 25 and k % 2 else None, density=0.15)
          for k in range(K)]
    return st, np.stack(ac)


def kinds_of(B, lanes=False):
    if not lanes:
        return [KIND_TILE[b % len(KIND_TILE)] for b in range(B)]
    # the lane kernel decides per WAVEFRONT: of its 64 games one walks along the limit (and drags the other 63 through
    # the general form and back) and holds a climb, two are done, undone and done (their wide steps drag the wavefront
    # along as well), the rest stay calm; every fourth wavefront also opens with the kinds that never return to the
    # digit form -- two more edge walks, int8 edge, demonstration, four tight games -- and never leaves the general form
    kinds = []
    for b in range(B):
        w, r = divmod(b, 64)
        kind = {17: "edge_wide" if w % 2 else "edge", 40: "done_undone_done", 41: "done_undone_done"}.get(r, "calm")
        if w % 4 == 3:  # (its first eight games: B = 200 ends there)
            kind = {0: "edge_wide", 1: "edge", 2: "int8_edge", 3: "demo"}.get(r, "tight" if r < 8 else kind)
        kinds.append(kind)
    return kinds


def make_walk(S, B, K, shift, seed, lanes=False):
    """state int8 (B,S,S,S), actions int8 (K,B,3S): the kinds of game tiled across b.  ``lanes``: the S = 4 layout for
    the one-game-per-lane kernel, events placed by the whole-game norm, one game per wavefront that triggers the fallback."""
    state, actions = np.zeros((B, S, S, S), np.int8), np.zeros((K, B, 3 * S), np.int8)
    for b, kind in enumerate(kinds_of(B, lanes)):
        rng = np.random.default_rng([seed, b])
        g = b // (64 if lanes else len(KIND_TILE))
        single = S == 4 and (lanes or g % 2 == 0)   # S = 4: one unit only, so that the whole-game norm walks as well
        if kind in ("plain", "calm"):
            st, ac = _plain(S, K, shift, rng, calm=kind == "calm")
        elif kind in ("edge", "edge_wide"):
            st, ac = _edge(S, K, shift, rng, g, kind == "edge_wide", single, climb=lanes or g % 4 == 0)
        elif kind == "tight":
            st, ac = _tight_again(S, K, shift, rng, b) if lanes else _tight(S, K, shift, rng, g, single)
        elif kind == "demo":
            st, ac = _demo(S, K, shift, rng, g)
        elif kind == "done_undone_done":
            st, ac = _done_undone_done(S, K, shift, rng, g)
        else:
            st, ac = _int8_edge(S, K, shift, rng)
        state[b], actions[:, b] = st, ac
    return state, actions


def trajectory(state, actions, shift, step=O.step_i8):
    """(final state, done (K,B), sticky overflow (B)) by K oracle steps."""
    K, B = actions.shape[:2]
    done, ovf, cur = np.zeros((K, B), np.uint8), np.zeros(B, np.uint8), state.copy()
    for k in range(K):
        cur, done[k], o = step(cur, actions[k], shift)
        ovf |= o
    return cur, done, ovf


# ---------------------------------------------------------------------------------------------- the census
UNIT_CLASSES = ("rise", "return", "at_limit", "one_above", "fast_after_overflow", "minus128", "overflow_after_rise")
DONE_CLASSES = ("done_fallback", "done_digit", "done_undone_done")


def census(S, shift, state, actions):
    """Counts of the events of the oracle trajectory, per scope: "unit" (all 16-byte units), at S = 4 "game" (the
    whole-game norm, what the lane kernel compares), at S = 25 "tail" and "straddle"; "tight": landings per value;
    "overflow_games", "games".  Definitions in the module docstring of tests/test_stream_walk_cpu.py."""
    K, B = actions.shape[:2]
    n, nu, tail, straddle = _unit_info(S)
    lim = digits_limit(shift)
    valid = lim >= 0
    small = ((actions >= 0) & (actions <= 3)).all(axis=2)                     # (K, B)

    def padded(x):
        flat = np.zeros((B, nu * 16), np.int64)
        flat[:, :n] = x.reshape(B, n)
        return flat.reshape(B, nu, 16)

    cur = state.copy()
    nb, na, chg, m128, uovf = (np.zeros((K, B, nu), t) for t in (np.int64, np.int64, bool, bool, bool))
    done, ovf = np.zeros((K, B), bool), np.zeros((K, B), bool)
    tight = {T: 0 for T in TIGHT_VALUES}
    for k in range(K):
        new, d, o = O.step_i8(cur, actions[k], shift)
        true = cur.astype(np.int64) - O.action_to_tensor(actions[k], shift)   # before the wrap
        assert np.array_equal(true.astype(np.int8), new)
        old_u, new_u, true_u = padded(cur), padded(new), padded(true)
        nb[k], na[k] = np.abs(old_u).sum(axis=2), np.abs(new_u).sum(axis=2)
        chg[k] = (old_u != new_u).any(axis=2)
        m128[k] = (old_u == -128).any(axis=2)
        uovf[k] = ((true_u < -128) | (true_u > 127)).any(axis=2)
        done[k], ovf[k] = d != 0, o != 0
        alone = (np.abs(old_u) == nb[k][:, :, None]) & (true_u != old_u)
        if valid:
            alone &= small[k][:, None, None]
        for T in TIGHT_VALUES:
            tight[T] += int((alone & (true_u == T)).sum())
        cur = new
    ovf_before = np.zeros((K, B), bool)
    ovf_before[1:] = np.cumsum(ovf, axis=0)[:-1] > 0
    gchg = chg.any(axis=2)
    redone = np.zeros((K, B), bool)                                          # done again after having been done and not done
    was_done, left = np.zeros(B, bool), np.zeros(B, bool)
    for k in range(K):
        redone[k] = done[k] & left
        left = (left & ~done[k]) | (was_done & ~done[k])
        was_done |= done[k]

    def classes(nb, na, chg, m128, uovf, mask=None):
        sm = small[:, :, None]
        fast = sm & valid & (nb <= lim)
        nxt = np.zeros_like(chg)
        nxt[:-1] = sm[1:] & chg[1:]
        out = {"rise": fast & chg & (na > lim), "return": valid & ~fast & chg & (na <= lim) & nxt,
               "at_limit": valid & sm & chg & (nb == lim), "one_above": valid & sm & chg & (nb == lim + 1),
               "fast_after_overflow": fast & chg & ovf_before[:, :, None], "minus128": sm & chg & m128}
        last_rise, oar = np.zeros(chg.shape[1:], bool), 0
        for k in range(K):   # a small step takes a byte beyond int8 in a unit whose last change was a rise
            oar += int((sm[k] & valid & uovf[k] & chg[k] & last_rise).sum())
            last_rise = np.where(chg[k], out["rise"][k], last_rise)
        out = {c: int(v.sum()) for c, v in out.items()}
        out["overflow_after_rise"] = oar
        if mask is not None or nb.shape[2] == nu:                              # (the done classes are per game)
            slow_chg, all_fast = (chg & ~fast).any(axis=2), (~chg | fast).all(axis=2)
            out["done_fallback"] = int((done & gchg & slow_chg).sum())
            out["done_digit"] = int((done & gchg & all_fast & chg.any(axis=2)).sum())
            out["done_undone_done"] = int((redone & chg.any(axis=2)).sum())
        return out

    def masked(mask):
        # units outside the mask count as unchanged and fast: the done classes then ask for the mask's units alone
        c = chg.copy()
        keep = np.zeros(nu, bool)
        keep[mask] = True
        c[:, :, ~keep] = False
        out = classes(nb, na, c, m128, uovf, mask)
        all_fast = (~chg | (small[:, :, None] & valid & (nb <= lim))).all(axis=2)
        out["done_digit"] = int((done & all_fast & c.any(axis=2)).sum())
        return out

    res = {"unit": classes(nb, na, chg, m128, uovf), "tight": tight, "games": B,
           "overflow_games": int(ovf.any(axis=0).sum())}
    if S == 4:  # the whole game as one unit
        g_old = lambda a: a.sum(axis=2, keepdims=True)
        res["game"] = classes(g_old(nb), g_old(na), chg.any(axis=2, keepdims=True), m128.any(axis=2, keepdims=True),
                              uovf.any(axis=2, keepdims=True))
    if S == 25:
        res["tail"], res["straddle"] = masked(tail), masked(straddle)
    return res


def admitted(S, shift):
    """[(scope, class)] the shift admits; ("tight", value) for the tight landings its factor range reaches."""
    valid = digits_limit(shift) >= 0
    done = DONE_CLASSES if valid else ("done_fallback", "done_undone_done")
    want = [("unit", c) for c in (UNIT_CLASSES if valid else ()) + done]
    if S == 4 and valid:
        want += [("game", c) for c in UNIT_CLASSES]
    if S == 25:
        want += [(scope, c) for scope in ("tail", "straddle") for c in (UNIT_CLASSES if valid else ()) + done]
    return want + [("tight", T) for T in sorted({T for T, _ in tight_pairs(shift)})]


def census_shortfalls(S, shift, c, minimum=4):
    """The admitted classes that occur fewer than ``minimum`` times, and an overflow flag raised in no or in every game."""
    short = [f"{scope}.{cls} = {c[scope][cls]}" for scope, cls in admitted(S, shift) if c[scope][cls] < minimum]
    if not 0 < c["overflow_games"] < c["games"]:
        short.append(f"overflow in {c['overflow_games']} of {c['games']} games")
    return short
