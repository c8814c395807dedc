/*
 * tensor_game_flips_plus.h -- C ABI of libtensorgame.so: flip-graph walks with plus transitions, so that a walk that has
 * no flip left, or has not lowered its rank for a while, goes on.
 *
 * The walks of tensor_game_flips.h only move inside one component of the flip graph: a list without a match is stuck for
 * good.  The "plus" transition of the later flip-graph papers (Arai, Ichikawa and Hukushima, "Adaptive flip graph
 * algorithm for matrix multiplication"; Kauers and Moosbauer's follow-ups) rewrites two terms that need not share
 * anything into three terms with the same sum: the rank rises by one, the new terms share factors, and the walk is in
 * another component.  Everything of tensor_game_flips.h holds here too: the conventions, terms, the stored form, the
 * walk state, removing a slot, Reduce, the Philox draw; tg_flip_begin starts the walks and tg_flip_advance is unchanged.
 * The reference has no counterpart.
 *
 * New walk state, per walk, which the caller provides zeroed for a fresh walk (tg_flip_begin does not know them):
 *   since      int32 (W)       the steps since the walk last lowered its rank or made an accepted plus (saturating)
 *   pluses     int64 (W)       accepted plus transitions
 * New arguments: plus_after in [1, 2^31 - 1]; plus_slack in [0, TG_FLIP_MAX_K].
 *
 * tg_flip_advance_plus runs steps t = step0 .. step0 + n_steps - 1 of every walk with state 0, walk w having the global id
 *   g = walk0 + w.  A walk with state 1 or -1, or whose cur_rank is outside [0, K], is left exactly as it is, since and
 *   pluses included.  One step, with L = cur_rank and best_rank the value from before the step:
 *     1. Matches.  C and the numbering of the matches as in tg_flip_advance step 1 (the state does not change here).
 *     2. Draw.  o = Philox-4x32-10 with counter (g mod 2^32, g >> 32, t, TG_FLIP_DOMAIN) and key (seed mod 2^32,
 *        seed >> 32): the very output tg_flip_advance draws.  o.x, o.y and o.z are used.
 *     3. Choice.  cap = min(K, best_rank + plus_slack); want = (C == 0) || (since >= plus_after);
 *        can = (L >= 2) && (L < cap).
 *          If want && can: a plus step (4).
 *          Else if C == 0: the state becomes 1 and this step and every later one changes nothing else (since, pluses,
 *            best_step and flips keep their values).
 *          Else: a flip step: tg_flip_advance's steps 2 and 3 word for word, drawing from o.x.  Afterwards, if L is
 *            below what it was before the step, since = 0; otherwise since = min(since + 1, 2^31 - 1) (after a refused
 *            flip too).
 *     4. Plus.  P = L (L - 1) / 2; c = (o.y * P) >> 32 in 64-bit arithmetic; (i, j) is pair number c of the pairs
 *        i < j < L in ascending (i, j) order (i first).  v = (o.z * 24) >> 32:
 *          bit 0: (a, b) = (i, j) if clear, (j, i) if set;
 *          bit 1: eps = +1 if clear, -1 if set;
 *          (p, q, r) = permutation number v >> 2 of (0, 1, 2) in lexicographic order: 012, 021, 102, 120, 201, 210.
 *        In int32: A_p = n_p(a), A_q = n_q(a), A_r = s_a * n_r(a); B_p = eps * n_p(b), B_q = n_q(b),
 *        B_r = eps * s_b * n_r(b); so a = A_p (x) A_q (x) A_r and b = B_p (x) B_q (x) B_r, each vector in its mode.
 *          t1 has A_p - B_p in mode p, A_q in mode q and A_r in mode r, and goes into slot a;
 *          t2 has B_p in mode p, A_q in mode q and A_r + B_r in mode r, and goes into the new slot L;
 *          t3 has B_p in mode p, B_q - A_q in mode q and B_r in mode r, and goes into slot b.
 *        t1 + t2 + t3 = a + b (expanded, the cross terms cancel in pairs).  If any value of the three new vectors
 *        A_p - B_p, A_r + B_r, B_q - A_q is outside [-bound, bound] the plus is refused: the step is spent, nothing
 *        changes, and since = min(since + 1, 2^31 - 1).  Otherwise, in this order: pluses += 1; the three terms are
 *        written, each brought to stored form unless it is null; L += 1; the null ones are removed, the highest slot
 *        first; Reduce; since = 0.  flips does not count a plus.
 *        (Nothing is special about terms that share a vector: with a shared mode p and eps = +1, or a shared mode q, t1
 *        or t3 is null and is dropped; with both only t2 is left, the merge of a and b, which in a reduced list leaves
 *        the bound, so that plus is refused.  n_r(a) = n_r(b) with s_a = -eps * s_b makes t2 null.)
 *     5. Best.  If L < best_rank: best = cur, best_rank = L, best_step = t + 1.
 *
 * Properties:
 *   Steps are consecutive: advancing n1 steps from step0 and then n2 steps from step0 + n1 gives what n1 + n2 steps from
 *     step0 give, since and pluses carried from one call to the next.
 *   Walks [0, W) with walk0 = g0 give what rows g0 .. g0 + W - 1 of a larger call with walk0 = 0 give.
 *   With plus_slack == 0 no plus is ever taken from a state tg_flip_begin and these entries made (L >= best_rank = cap):
 *     the seven state tensors of tensor_game_flips.h come out exactly as tg_flip_advance leaves them, and pluses stays
 *     as it was.
 *   Every value of every list stays in [-bound, bound], and cur_rank <= K always (a plus needs L < cap <= K).
 *   Walks with state != 0, or with cur_rank outside [0, K], are left exactly as they are, since and pluses included.
 */
#ifndef TENSOR_GAME_FLIPS_PLUS_H_
#define TENSOR_GAME_FLIPS_PLUS_H_

#include "tensor_game_flips.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_FLIP_MAX_PLUS_AFTER 2147483647 /* since saturates there */

/* Host only, no device work: the size checks of tg_flip_advance_plus alone: those of tg_flip_check (with M = 0), and
 * 1 <= plus_after <= TG_FLIP_MAX_PLUS_AFTER, 0 <= plus_slack <= TG_FLIP_MAX_K. */
int tg_flip_plus_check(int64_t W, int K, int S, int shift, int bound, int64_t step0, int64_t n_steps, int64_t plus_after,
                       int64_t plus_slack);

/* n_steps steps of W walks in place, in ONE kernel launch (a wavefront per walk; no wavefront waits for another).  The
 * seven state tensors as tg_flip_begin left them (the same K, S, shift and bound); since: int32 (W), 4-byte aligned;
 * pluses: int64 (W), 8-byte aligned.  Refuses, before any launch and naming the argument, what tg_flip_advance and
 * tg_flip_plus_check refuse, and a null or misaligned since or pluses.  W = 0 returns 0 at once. */
int tg_flip_advance_plus(int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank, int64_t* best_step,
                         int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses, int64_t W, int K, int S, int shift,
                         int bound, uint64_t seed, uint64_t walk0, int64_t step0, int64_t n_steps, int64_t plus_after,
                         int64_t plus_slack, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_FLIPS_PLUS_H_ */
