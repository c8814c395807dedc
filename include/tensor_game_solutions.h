/*
 * tensor_game_solutions.h -- C ABI of libtensorgame.so: exact verification and the canonical form of a factorisation.
 *
 * The solution search (tensor_game_rollout.h, tensor_game_rollout_slots.h) ends with action lists that replayed a
 * start state to zero IN INT8: the steppers narrow with wrap and do not stop a row on overflow, so a head can wrap back
 * to zero and be reported as solved.  The reference has no counterpart (it prints num_solutions_found,
 * training.py:346).  tg_solution_canon proves a list exactly, reduces it to a canonical form, and derives an effective
 * rank and a 64-bit key from that form, so that equal factorisations found again can be told apart from new ones.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * Semantics, for solution m with L = lengths[m]:
 *
 * Terms.  Term t < L has the factors f = tok - shift of tokens[m][t], taken in 32 bits: u = f[0:S], v = f[S:2S],
 *   w = f[2S:3S].  The rows t >= L of tokens[m] are not read.
 *
 * Verification.  residual = targets[m] - sum_{t<L} u (x) v (x) w in int32, which cannot wrap: a token is an int8 and
 *   0 <= shift <= 64, so |f| <= 192, a term's entry is at most 192^3 = 7 077 888 in magnitude and the sum of
 *   L <= TG_SOL_MAX_K = 256 of them at most 1 811 939 328 < 2^31 - 128.  residual_nnz[m] = the number of non-zero
 *   entries of the residual; the list is a proven factorisation of targets[m] exactly when it is 0.  It is computed from
 *   the ORIGINAL terms, not from the canonical ones.
 *
 * Canonical form, in this order:
 *   1. Drop the null terms: those with u, v or w all zero.
 *   2. Normalise the signs.  For each of u, v, w: if its first non-zero value is negative, negate the vector and flip
 *      the term's sign sigma (which starts at +1).  The term is now sigma * u (x) v (x) w with all three vectors
 *      "first non-zero positive".
 *   3. Order the terms by their 3S normalised values (u, v, w), compared lexicographically as signed integers, ascending.
 *   4. Merge.  For each run of equal (u, v, w) let c = the sum of sigma over the run.  |c| copies are kept; if c < 0,
 *      w is negated in each copy; a run with c = 0 disappears.
 *   5. rank[m] = the number of terms kept.
 *   6. canon[m][0:rank] holds the kept terms as tokens (value + shift) in that order; the remaining rows of canon[m]
 *      are zero bytes (the padding RolloutResult.solutions() uses).
 *   The sum of the canonical terms equals the sum of the original terms.  The form does not depend on the order of the
 *   input terms, on how signs were distributed inside a term, or on inserted null terms or cancelling pairs.  Two things
 *   are NOT factored out here: rescalings between factors, such as (2u) (x) v = u (x) (2v), and symmetries of the target
 *   (tg_orbit_canon, tensor_game_orbits.h, factors out a set of symmetries the caller supplies).
 *
 * Key.  The n = rank * 3S canonical token bytes are read as one byte stream, zero-padded to 8-byte little-endian words
 *   w_k:  key = fmix64( (sum_k fmix64(w_k + (k+1)*0x9E3779B97F4A7C15)) ^ (n * 0xC2B2AE3D27D4EB4F) ), which is
 *   tg_hash_u64's rule and its fmix64 (tensor_game.h) with n in place of S^3.  The empty form (rank 0) has key 0.
 *
 * Bad rows.  A row is bad if L < 0 or L > K (bit 0 of *status), or if a negation of step 2 (of a term that step 1 keeps)
 *   or of step 4 (of a copy that is kept) gives a token 2*shift - tok outside [-128,127] (bit 1).  A bad row gives
 *   rank = 0, an all-zero canon row, key = 0 and residual_nnz = -1, and leaves every other row untouched.  A length is
 *   checked before it addresses anything.  The bits are ORed into *status (sticky; the call never clears them).
 *
 * Every output is a function of its own row alone: no result depends on scheduling; no floating point is used.
 */
#ifndef TENSOR_GAME_SOLUTIONS_H_
#define TENSOR_GAME_SOLUTIONS_H_

#include "tensor_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_SOL_MAX_K 256      /* terms per list */
#define TG_SOL_MAX_SHIFT 64
#define TG_SOL_BAD_LENGTH 1   /* bits of *status */
#define TG_SOL_BAD_NEGATION 2

/* Host only, no device work: the size checks of tg_solution_canon alone.  M >= 0, 1 <= K <= TG_SOL_MAX_K,
 * 1 <= S <= TG_MAX_S, 0 <= shift <= TG_SOL_MAX_SHIFT. */
int tg_solution_check(int64_t M, int K, int S, int shift);

/* The semantics above, for M lists, in ONE kernel launch (a wavefront per list at K <= 64, a 256-thread workgroup above).
 *   targets: int8 (M,S,S,S), C-contiguous, any alignment; may be NULL together with residual_nnz (no verification).
 *   tokens: int8 (M,K,3S) = cat(u,v,w) + shift as RolloutResult.solutions() returns them, any alignment.
 *   lengths: int64 (M).  canon: int8 (M,K,3S), out of place, any alignment.  rank: int32 (M).
 *   key: uint64 (M), 8-byte aligned.  residual_nnz: int32 (M) or NULL.  status: uint32 (1) or NULL.
 * M = 0 returns 0 at once. */
int tg_solution_canon(const int8_t* targets, const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int S,
                      int shift, int8_t* canon, int32_t* rank, uint64_t* key, int32_t* residual_nnz, uint32_t* status,
                      tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_SOLUTIONS_H_ */
