/*
 * tensor_game_flips_mod2.h -- C ABI of libtensorgame.so: flip-graph walks over Z_2, the field with two elements, and the
 * exact proof of what they reach.
 *
 * The walks of tensor_game_flips.h and tensor_game_flips_plus.h work over the integers with a coefficient bound: many
 * drawn flips are refused, and many components of the graph cannot be reached.  The flip-graph results that matter were
 * found over Z_2 and lifted afterwards (Kauers and Moosbauer, "Flip graphs for matrix multiplication", 2022, and its
 * follow-ups; AlphaTensor's 47 for <4,4,4>).  Over Z_2 there are no signs, no bound and no normal form: no flip is ever
 * refused, a factor of S <= 32 values is one 32-bit word, "the same vector" is one integer compare, a flip is two XORs
 * and a merge is one.  The reference has no counterpart.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * Terms.  A term is three uint32 masks (m_0, m_1, m_2) and stands for m_0 (x) m_1 (x) m_2 over Z_2: bit e of m_d is
 *   the e-th value of the mode-d vector mod 2.  Masks are stored as int32 bit patterns (with S = 32, bit 31 is in use).
 *   A term is null if any of its masks is 0.  Bits at or above S are always 0.
 *   From a token row (3S bytes cat(u, v, w) + shift, as in tensor_game_solutions.h): bit e of m_d =
 *   (tokens[d*S + e] - shift) & 1, on the two's complement pattern, so that -1 and -3 are odd.  Every integer list has a
 *   reduction mod 2: there is no range error.
 *
 * Walk state, per walk (W walks):
 *   cur        int32 (W,K,3)   the list: L = cur_rank live terms; rows at or beyond L are zero
 *   cur_rank   int32 (W)       L
 *   best       int32 (W,K,3)   the shortest list the walk has held (the first one, if several are equally short)
 *   best_rank  int32 (W)
 *   best_step  int64 (W)       the number of steps after which it was held (0: the list tg_flip2_begin made)
 *   flips      int64 (W)       flips made
 *   state      int32 (W)       0 walking, 1 stuck, -1 bad (tg_flip2_begin refused the row), as in tensor_game_flips.h
 *   since      int32 (W)       the steps since the walk last lowered its rank or made a plus (saturating at 2^31 - 1)
 *   pluses     int64 (W)       plus transitions made
 *
 * Removing slot p of a list: if p != L - 1 the term in slot L - 1 moves into slot p; then L decreases by one.
 *
 * Reduce.  Repeat until a whole scan merges nothing.  A scan visits the pairs i < j < L in ascending (i, j) order (i
 *   first):
 *     1. The pair qualifies if m_d(i) == m_d(j) in at least two of the modes d = 0, 1, 2.
 *     2. If it does so in all three modes the two terms cancel: both are removed, slot j first, then slot i.
 *     3. Otherwise, with d the mode that is not shared, m_d(i) ^= m_d(j) (not zero, as the two differ) and slot j is
 *        removed.
 *   After 2 or 3 the scan ends and the next one starts at (0, 1).  No pair is ever skipped, so a reduced list has no
 *   qualifying pair.  An implementation may look only at pairs that involve a changed or moved term, as long as it
 *   gives what these scans give.
 *
 * tg_flip2_begin, for walk w, with m = src ? src[w] : w:
 *     a. m outside [0, M): bad, bit TG_FLIP_BAD_SRC.  Checked before m addresses anything.
 *     b. else L0 = lengths[m] outside [0, K]: bad, bit TG_FLIP_BAD_LENGTH.  Checked before it addresses anything.
 *   There is no TG_FLIP_BAD_RANGE.  A bad walk gets state -1, all-zero cur and best rows, cur_rank = best_rank = 0,
 *   best_step = flips = pluses = since = 0, and touches no other walk; exactly one bit is set per bad walk.  The bits are
 *   ORed into *status (sticky; the call never clears them).  Otherwise, in this order (rows t >= L0 are not read):
 *     1. Take the masks of rows t < L0.
 *     2. Drop the null terms; the others keep their order.
 *     3. Reduce.
 *     4. best = cur, best_rank = cur_rank, best_step = flips = pluses = since = 0, state = 0.
 *
 * tg_flip2_advance runs steps t = step0 .. step0 + n_steps - 1 of every walk with state 0, walk w having the global id
 *   g = walk0 + w.  A walk with state != 0, or whose cur_rank is outside [0, K], is left exactly as it is, all nine
 *   tensors.  One step, with L = cur_rank and best_rank the value from before the step:
 *     1. Matches.  All (i, j, d) with i < j < L and m_d(i) == m_d(j).  They are numbered 0 .. C-1 in ascending
 *        (i, j, d) order (i first, d last).
 *     2. Draw.  o = Philox-4x32-10 with counter (g mod 2^32, g >> 32, t, TG_FLIP2_DOMAIN) and key (seed mod 2^32,
 *        seed >> 32).
 *     3. Choice.  cap = min(K, best_rank + plus_slack); want = plus_after > 0 && (C == 0 || since >= plus_after);
 *        can = L >= 2 && L < cap.
 *          If want && can: a plus step (5).
 *          Else if C == 0: the state becomes 1 and this step and every later one changes nothing else.
 *          Else: a flip step (4).
 *     4. Flip.  c = (o.x * 4C) >> 32 in 64-bit arithmetic; the match is number c >> 2;
 *          bit 0 of c: (q, r) = the two modes other than d, ascending if clear, swapped if set;
 *          bit 1 of c: (a, b) = (i, j) if clear, (j, i) if set.
 *        With x = m_d(a) = m_d(b):
 *          a' has x in mode d, m_q(a) ^ m_q(b) in mode q and m_r(a) in mode r;
 *          b' has x in mode d, m_q(b) in mode q and m_r(b) ^ m_r(a) in mode r.
 *        a' + b' = a + b over Z_2.  The flip is never refused: flips += 1; a' goes into slot a and b' into slot b; then
 *        the null ones are removed, the higher slot first; then Reduce.  Afterwards, if L is below what it was before
 *        the step, since = 0; otherwise since = min(since + 1, 2^31 - 1).
 *     5. Plus.  P = L (L - 1) / 2; the pair (i, j) is number (o.y * P) >> 32 of the pairs i < j < L in ascending (i, j)
 *        order (i first).  v = (o.z * 12) >> 32:
 *          bit 0 of v: (a, b) = (i, j) if clear, (j, i) if set;
 *          (p, q, r) = permutation number v >> 1 of (0, 1, 2) in lexicographic order: 012, 021, 102, 120, 201, 210.
 *        From the two terms as they are before the step:
 *          t1 has m_p(a) ^ m_p(b) in mode p, m_q(a) in mode q and m_r(a) in mode r, and goes into slot a;
 *          t2 has m_p(b) in mode p, m_q(a) in mode q and m_r(a) ^ m_r(b) in mode r, and goes into the new slot L;
 *          t3 has m_p(b) in mode p, m_q(b) ^ m_q(a) in mode q and m_r(b) in mode r, and goes into slot b.
 *        t1 + t2 + t3 = a + b over Z_2.  The plus is never refused: pluses += 1; the three terms are written; L += 1; then
 *        the null ones are removed, the highest slot first; then Reduce; since = 0.  flips does not count a plus.
 *     6. Best.  If L < best_rank: best = cur, best_rank = L, best_step = t + 1.
 *
 * Properties:
 *   Steps are consecutive: advancing n1 steps from step0 and then n2 steps from step0 + n1 gives what n1 + n2 steps from
 *     step0 give.
 *   Walks [0, W) with walk0 = g0 give what rows g0 .. g0 + W - 1 of a larger call with walk0 = 0 give.
 *   The XOR of all terms of a list (the tensor it sums to over Z_2) never changes: not in tg_flip2_begin, which keeps the
 *     parity of the tokens' sum, and not in any step.
 *   With plus_after == 0 no plus is ever taken; since is still maintained, but never read.
 *   With plus_slack == 0 no plus is ever taken from a state these entries made (L >= best_rank = cap).
 *   cur_rank <= K always (a plus needs L < cap <= K).
 */
#ifndef TENSOR_GAME_FLIPS_MOD2_H_
#define TENSOR_GAME_FLIPS_MOD2_H_

#include "tensor_game_flips.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_FLIP2_DOMAIN 0x46320000u         /* the Philox counter's fourth word */
#define TG_FLIP2_MAX_PLUS_AFTER 2147483647  /* since saturates there */

/* Host only, no device work: the size checks of the entries below alone.  M >= 0, W >= 0, 1 <= K <= TG_FLIP_MAX_K,
 * 1 <= S <= TG_MAX_S, 0 <= shift <= TG_SOL_MAX_SHIFT, 1 <= n_steps <= TG_FLIP_MAX_STEPS, step0 >= 0 and
 * step0 + n_steps <= 2^32, 0 <= plus_after <= TG_FLIP2_MAX_PLUS_AFTER, 0 <= plus_slack <= TG_FLIP_MAX_K.
 * (tg_flip2_begin checks what it takes: M, W, K, S, shift.) */
int tg_flip2_check(int64_t M, int64_t W, int K, int S, int shift, int64_t step0, int64_t n_steps, int64_t plus_after,
                   int64_t plus_slack);

/* The start of W walks, in ONE kernel launch (a wavefront per walk).
 *   tokens: int8 (M,K,3S), any alignment.  lengths: int64 (M).  src: int64 (W) or NULL (then W must equal M).
 *   cur, best: int32 (W,K,3), distinct from each other.  cur_rank, best_rank, state, since: int32 (W).  best_step, flips,
 *   pluses: int64 (W).  status: uint32 (1) or NULL.
 * W = 0 returns 0 at once. */
int tg_flip2_begin(const int8_t* tokens, const int64_t* lengths, int64_t M, const int64_t* src, int64_t W, int K, int S,
                   int shift, int32_t* cur, int32_t* cur_rank, int32_t* best, int32_t* best_rank, int64_t* best_step,
                   int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses, uint32_t* status, tg_stream_t stream);

/* n_steps steps of W walks in place, in ONE kernel launch (a wavefront per walk; no wavefront waits for another).  The
 * walk state as tg_flip2_begin left it (the same K and S).  W = 0 returns 0 at once. */
int tg_flip2_advance(int32_t* cur, int32_t* cur_rank, int32_t* best, int32_t* best_rank, int64_t* best_step,
                     int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses, int64_t W, int K, int S,
                     uint64_t seed, uint64_t walk0, int64_t step0, int64_t n_steps, int64_t plus_after, int64_t plus_slack,
                     tg_stream_t stream);

/* The proof, in ONE kernel launch (a wavefront per list), exact:
 *   residual[m] = the number of cells (i, j, k) where targets[m][i][j][k] & 1 differs from the parity of the number of
 *   terms t < ranks[m] with bit i of m_0, bit j of m_1 and bit k of m_2 all set; -1 if ranks[m] is outside [0, K].
 *   Rows at or beyond the rank are not read.
 *   targets: int8 (M,S,S,S), any alignment.  lists: int32 (M,K,3).  ranks, residual: int32 (M).
 * M = 0 returns 0 at once. */
int tg_flip2_residual(const int8_t* targets, const int32_t* lists, const int32_t* ranks, int64_t M, int K, int S,
                      int32_t* residual, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_FLIPS_MOD2_H_ */
