/*
 * tensor_game_flips.h -- C ABI of libtensorgame.so: random walks on the flip graph, which lower the rank of a
 * factorisation that is already known.
 *
 * The archive (tensor_game_solutions.h, tensor_game_orbits.h) proves, canonicalises and stores factorisations; nothing
 * there improves one.  The flip graph of Kauers and Moosbauer ("Flip graphs for matrix multiplication", 2022) does: two
 * terms that share a factor are rewritten into two other terms with the same sum, and whenever two terms come to share
 * two factors they merge into one and the rank drops.  A walk is a list of at most TG_FLIP_MAX_K terms and a few words;
 * it is independent of every other walk, uses no floating point, and draws from Philox keyed by its global id, so every
 * result below is a function of (the walk's list, seed, walk id, step index) alone.  The reference has no counterpart.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * Terms.  A term is three integer vectors of S values, (u, v, w), and stands for u (x) v (x) w.  As a token row it is
 *   the 3S bytes cat(u, v, w) + shift, as in tensor_game_solutions.h.  A term is null if one of its vectors is all zero.
 *   A vector is normalised if its first non-zero value is positive.
 *
 * Stored form.  A term is in stored form if u and v are normalised (w carries the term's sign).  To bring (u, v, w) to
 *   stored form: for each of u, v, w whose first non-zero value is negative, negate that vector and flip a sign sigma
 *   that starts at +1; the stored term is (u, v, sigma * w).  Of a stored term, n_0 = u, n_1 = v, s = the sign of the
 *   first non-zero value of w, and n_2 = s * w; so the term is s * n_0 (x) n_1 (x) n_2 with all three n_m normalised.
 *
 * Walk state, per walk (W walks):
 *   cur        int8  (W,K,3S)  the list: L = cur_rank live terms in stored form as tokens; rows at or beyond L are
 *                              zero BYTES (not zero values)
 *   cur_rank   int32 (W)       L
 *   best       int8  (W,K,3S)  the shortest list the walk has held (the first one, if several are equally short)
 *   best_rank  int32 (W)
 *   best_step  int64 (W)       the number of steps after which it was held (0: the list tg_flip_begin made)
 *   flips      int64 (W)       accepted flips
 *   state      int32 (W)       0 walking, 1 stuck (no flip exists), -1 bad (tg_flip_begin refused the row)
 *
 * Removing slot p of a list: if p != L - 1 the term in slot L - 1 moves into slot p; then L decreases by one.
 *
 * Reduce.  Repeat until a whole scan merges nothing.  A scan visits the pairs i < j < L in ascending (i, j) order (i
 *   first):
 *     1. The pair qualifies if n_m(i) == n_m(j) in at least two of the modes m = 0, 1, 2.
 *     2. d = the mode that is not shared, or 2 if all three are.
 *     3. z = s_i * n_d(i) + s_j * n_d(j), in int32.  (The two terms sum to z in mode d and the shared vectors elsewhere.)
 *     4. If some |z[e]| > bound the pair is skipped: the scan goes on with the next pair.  (z does not change while
 *        neither term does, so a skipped pair stays skipped until then.)
 *     5. If z is all zero both terms are removed: slot j first, then slot i.
 *     6. Otherwise term i becomes: z in mode d, n_m(i) in the two other modes, brought to stored form (s_i becomes the
 *        sign of the first non-zero value of z); then slot j is removed.
 *   After 5 or 6 the scan ends and the next one starts at (0, 1).  An implementation may look only at pairs that
 *   involve a changed or moved term, as long as it gives what these scans give.
 *
 * tg_flip_begin, for walk w, with m = src ? src[w] : w:
 *     a. m outside [0, M): bad, bit TG_FLIP_BAD_SRC.  Checked before m addresses anything.
 *     b. else L0 = lengths[m] outside [0, K]: bad, bit TG_FLIP_BAD_LENGTH.  Checked before it addresses anything.
 *     c. else some value tokens[m][t][e] - shift with t < L0 outside [-bound, bound] (null terms included): bad, bit
 *        TG_FLIP_BAD_RANGE.  Rows t >= L0 are not read.
 *   A bad walk gets state -1, all-zero cur and best rows, cur_rank = best_rank = 0, best_step = flips = 0, and touches
 *   no other walk; exactly one bit is set per bad walk (the first of a, b, c that applies).  The bits are ORed into
 *   *status (sticky; the call never clears them).  Otherwise, in this order:
 *     1. Drop the null terms; the others keep their order.
 *     2. Bring every term to stored form.
 *     3. Reduce.
 *     4. best = cur, best_rank = cur_rank, best_step = 0, flips = 0, state = 0.
 *
 * tg_flip_advance runs steps t = step0 .. step0 + n_steps - 1 of every walk with state 0, walk w having the global id
 *   g = walk0 + w.  A walk with state 1 or -1, or whose cur_rank is outside [0, K], is left exactly as it is.  One step:
 *     1. Matches.  All (i, j, m) with i < j < L and n_m(i) == n_m(j), compared on the values.  They are numbered
 *        0 .. C-1 in ascending (i, j, m) order (i first, m last).  If C == 0 the state becomes 1 and this step and every
 *        later one changes nothing else (best_step and flips keep their values).
 *     2. Draw.  o = Philox-4x32-10 with counter (g mod 2^32, g >> 32, t, 0x46000000) and key (seed mod 2^32,
 *        seed >> 32); c = (o.x * 8C) >> 32 in 64-bit arithmetic; the match is number c >> 3, the variant is c & 7:
 *          bit 0: eps = +1 if clear, -1 if set;
 *          bit 1: (q, r) = the two modes other than m, ascending if clear, swapped if set;
 *          bit 2: (a, b) = (i, j) if clear, (j, i) if set.
 *     3. Flip.  With x = n_m(a) = n_m(b), in int32:
 *          a' has x in mode m, n_q(a) + eps * n_q(b) in mode q and s_a * n_r(a) in mode r;
 *          b' has x in mode m, n_q(b) in mode q and s_b * n_r(b) - eps * s_a * n_r(a) in mode r.
 *        a' + b' = a + b.  If any value of a' or b' is outside [-bound, bound] the flip is refused: the step is spent
 *        and nothing changes.  Otherwise flips += 1; a' goes into slot a and b' into slot b, each brought to stored
 *        form unless it is null; then the null ones are removed, the higher slot first; then Reduce.
 *     4. Best.  If L < best_rank: best = cur, best_rank = L, best_step = t + 1.
 *   Steps are consecutive: advancing n1 steps from step0 and then n2 steps from step0 + n1 gives what n1 + n2 steps from
 *   step0 give, and walks [0, W) with walk0 = g0 give what rows g0 .. g0 + W - 1 of a larger call with walk0 = 0 give.
 *
 * Every value of every list stays in [-bound, bound] and bound + shift <= 127, so every stored value is a token.
 */
#ifndef TENSOR_GAME_FLIPS_H_
#define TENSOR_GAME_FLIPS_H_

#include "tensor_game_solutions.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_FLIP_MAX_K 128        /* terms per walk */
#define TG_FLIP_MAX_BOUND 63
#define TG_FLIP_MAX_STEPS 65536  /* per launch: no launch runs unboundedly long */
#define TG_FLIP_BAD_LENGTH 1     /* bits of *status */
#define TG_FLIP_BAD_RANGE 2
#define TG_FLIP_BAD_SRC 4
#define TG_FLIP_DOMAIN 0x46000000u /* the Philox counter's fourth word */

/* Host only, no device work: the size checks of the two entries below alone.  M >= 0, W >= 0, 1 <= K <= TG_FLIP_MAX_K,
 * 1 <= S <= TG_MAX_S, 0 <= shift <= TG_SOL_MAX_SHIFT, 1 <= bound <= TG_FLIP_MAX_BOUND, 1 <= n_steps <= TG_FLIP_MAX_STEPS,
 * step0 >= 0 and step0 + n_steps <= 2^32.  (tg_flip_begin checks what it takes: M, W, K, S, shift, bound.) */
int tg_flip_check(int64_t M, int64_t W, int K, int S, int shift, int bound, int64_t step0, int64_t n_steps);

/* The start of W walks, in ONE kernel launch (a wavefront per walk).
 *   tokens: int8 (M,K,3S), any alignment.  lengths: int64 (M).  src: int64 (W) or NULL (then W must equal M).
 *   cur, best: int8 (W,K,3S), any alignment, distinct from tokens and from each other.  cur_rank, best_rank, state:
 *   int32 (W).  best_step, flips: int64 (W).  status: uint32 (1) or NULL.
 * W = 0 returns 0 at once. */
int tg_flip_begin(const int8_t* tokens, const int64_t* lengths, int64_t M, const int64_t* src, int64_t W, int K, int S,
                  int shift, int bound, int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank,
                  int64_t* best_step, int64_t* flips, int32_t* state, uint32_t* status, tg_stream_t stream);

/* n_steps steps of W walks in place, in ONE kernel launch (a wavefront per walk; no wavefront waits for another).
 * The walk state as tg_flip_begin left it (the same K, S, shift and bound).  W = 0 returns 0 at once. */
int tg_flip_advance(int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank, int64_t* best_step, int64_t* flips,
                    int32_t* state, int64_t W, int K, int S, int shift, int bound, uint64_t seed, uint64_t walk0,
                    int64_t step0, int64_t n_steps, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_FLIPS_H_ */
