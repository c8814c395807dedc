/*
 * tensor_game_lift.h -- C ABI of libtensorgame.so: the sign lift of a Z_2 list to the integers, with an exact check.
 *
 * The walks of tensor_game_flips_mod2.h end in lists that are right mod 2.  The sign lift keeps such a list's support
 * and looks for coefficients in {-1, 0, 1} on it that give the INTEGER target: one unknown per support position says
 * whether the coefficient there is -1.  Those unknowns obey one linear system over Z_2, which makes the list right mod
 * 4; every solution of that system is a concrete +-1 candidate, and each candidate is checked exactly over the
 * integers.  Nothing is reported as lifted but through that exact check.  (Level-by-level Hensel lifting, with unknowns
 * on all 3 R S positions and an arbitrary solution per level, loses the +-1 lifts that exist: DESIGN.md, sign lift.)
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * Lists are those of tensor_game_flips_mod2.h: a term is three uint32 masks (m_0, m_1, m_2) stored as int32 bit
 * patterns, bit e of m_d the e-th value of the mode-d vector; bits at or above S are taken as 0.
 *
 * tg_lift2_signs, for list w with the global id g = list0 + w and R = ranks[w].  Every output of list w is a function
 * of its own row (targets[w], lists[w], ranks[w]), `seed`, g and `tries` alone.
 *   0. R outside [0, K]: status -1, try_used -1, unknowns = sys_rank = 0, miss -1, all-zero token rows.  R is checked
 *      before it addresses anything.  Rows at or beyond R are never read.
 *   1. X0[r][d][e] = bit e of m_d(r) for r < R.  D = targets[w] - sum_r X0[r][0] (x) X0[r][1] (x) X0[r][2], in int32.
 *      If any entry of D is odd: status 1 (TG_LIFT2_NOT_MOD2), miss = the number of odd entries (tg_flip2_residual's
 *      count), try_used -1, unknowns = sys_rank = 0, all-zero token rows.
 *   2. Unknowns and right-hand side.  The unknowns are the support positions (r, d, e) with X0[r][d][e] = 1, numbered
 *      c = 0 .. N-1 in ascending (r, d, e) order (r first, e last).  unknowns = N.  Column c is the tensor obtained from
 *      term r by replacing its mode-d factor with the unit vector e, taken mod 2 (a null term has all-zero columns).
 *      The right-hand side is b = (D >> 1) & 1 per cell, with an arithmetic shift.  The system is
 *      sum_c x_c column_c = b over Z_2: setting X[r][d][e] = -1 where x_c = 1 (and X = X0 elsewhere) makes
 *      sum_r X[r][0] (x) X[r][1] (x) X[r][2] == targets[w] mod 4.
 *   3. Pivots.  Column c is a pivot column iff it is not in the Z_2 span of the columns c' < c.  sys_rank = their
 *      number P.  The other N - P columns are free, numbered f = 0, 1, .. in ascending c.  If b is not in the span of
 *      the columns: status 2 (TG_LIFT2_INCONSISTENT), try_used -1, miss -1, all-zero token rows (unknowns and sys_rank
 *      are still N and P).
 *   4. Tries t = 0 .. tries-1, in this order.  Free variable f is 0 at t = 0; for t > 0 it is bit (f & 31) of word
 *      ((f >> 5) & 3) (x, y, z, w = 0, 1, 2, 3) of Philox-4x32-10 with counter (g mod 2^32, g >> 32, t,
 *      TG_LIFT2_DOMAIN + (f >> 7)) and key (seed mod 2^32, seed >> 32).  x is the unique solution of the system with
 *      those free values.  The candidate has the coefficient -1 where x_c = 1, +1 elsewhere on the support, 0 off it.
 *      miss_t = the number of non-zero entries of targets[w] - sum of the candidate's terms, in int32, which cannot
 *      wrap.  The first t with miss_t = 0 gives status 0 (TG_LIFT2_OK), try_used = t, miss = 0, token rows r < R =
 *      cat(u, v, w) of the candidate + shift (as in tensor_game_solutions.h), rows r >= R zero bytes.  If no try is
 *      exact: status 3 (TG_LIFT2_NOT_EXACT), try_used -1, miss = min_t miss_t, all-zero token rows.
 *
 * The pivot columns, sys_rank and x are properties of the system, not of how it is eliminated: an implementation is
 * free in its method as long as it gives these values.  It may compact columns, skip all-zero rows, factor once for all
 * tries and stop after the first exact try.
 *
 * Properties:
 *   Lists [0, W) with list0 = g0 give what rows g0 .. g0 + W - 1 of a larger call with list0 = 0 give.
 *   The outputs do not depend on ws_lists, on the workspace's contents before the call, or on the other lists.
 *   status 0 is a proof: the token rows sum to targets[w] exactly.  (SolutionArchive proves them again by itself.)
 */
#ifndef TENSOR_GAME_LIFT_H_
#define TENSOR_GAME_LIFT_H_

#include "tensor_game_flips_mod2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_LIFT2_DOMAIN 0x4C320000u /* the Philox counter's fourth word, plus f >> 7 */
#define TG_LIFT2_MAX_TRIES 1024
#define TG_LIFT2_MAX_WS_LISTS 65536

#define TG_LIFT2_OK 0
#define TG_LIFT2_NOT_MOD2 1
#define TG_LIFT2_INCONSISTENT 2
#define TG_LIFT2_NOT_EXACT 3

/* Host only, no device work: bytes of scratch per concurrently resident list for lists of up to K terms over S values
 * (a multiple of 256).  0 where the system of every such list fits in a workgroup's LDS: no workspace is needed then
 * (S <= 9 at every K <= 32 is among these).  -1 (TG_ERR_INVALID) for K outside [1, TG_FLIP_MAX_K] or S outside
 * [1, TG_MAX_S]. */
int64_t tg_lift2_workspace_bytes(int K, int S);

/* Host only, no device work: the size checks of tg_lift2_signs alone.  W >= 0 (and small enough that every byte offset
 * stays inside int64), 1 <= K <= TG_FLIP_MAX_K, 1 <= S <= TG_MAX_S, 0 <= shift <= TG_SOL_MAX_SHIFT,
 * 1 <= tries <= TG_LIFT2_MAX_TRIES, 0 <= ws_lists <= TG_LIFT2_MAX_WS_LISTS, and ws_lists >= 1 where
 * tg_lift2_workspace_bytes(K, S) > 0. */
int tg_lift2_check(int64_t W, int K, int S, int shift, int64_t tries, int64_t ws_lists);

/* The sign lift of W lists, in ONE kernel launch (a workgroup per list; no workgroup waits for another).
 *   targets: int8 (W,S,S,S), any alignment: the INTEGER targets.  lists: int32 (W,K,3).  ranks: int32 (W).
 *   tokens: int8 (W,K,3S), out, any alignment.  status, try_used, unknowns, sys_rank, miss: int32 (W), out.
 *   workspace: ws_lists * tg_lift2_workspace_bytes(K, S) bytes, 16-byte aligned, contents arbitrary; NULL is allowed
 *   when that size is 0.  At most ws_lists lists are in work at a time (it bounds the grid; more is never slower).
 * W = 0 returns 0 at once. */
int tg_lift2_signs(const int8_t* targets, const int32_t* lists, const int32_t* ranks, int64_t W, int K, int S, int shift,
                   uint64_t seed, uint64_t list0, int64_t tries, int8_t* tokens, int32_t* status, int32_t* try_used,
                   int32_t* unknowns, int32_t* sys_rank, int32_t* miss, void* workspace, int64_t ws_lists,
                   tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_LIFT_H_ */
