/*
 * tensor_game_bases.h -- C ABI of libtensorgame.so: the way BACK from a changed basis.
 *
 * tg_sample_basis_i8 draws a unimodular triple (A,B,C), P = L*U per mode, and tg_change_basis_i8 moves a TARGET into
 * it: T' = (A,B,C).T (tensor_game.h).  A search that runs on T' finds T' = sum u' (x) v' (x) w', and then
 * T = sum (A^-1 u') (x) (B^-1 v') (x) (C^-1 w'): a factorisation of the original target, usually another one than a
 * search in the given basis finds (the change of basis of the AlphaTensor paper; not in the reference).  This header
 * has the two pieces that map an action list back on the device: the exact integer inverse of a sampled basis, and the
 * application of a matrix triple to the factors of every term of a list.  The mapped factors are int8 tokens, not
 * vocabulary tokens: they feed tg_solution_canon (tensor_game_solutions.h) and the archive, not the network.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.  All arithmetic is integer and exact; every output is a function of its own
 * triple / its own row alone, so no result depends on scheduling.  The one atomic is the OR of the sticky bits into
 * *status (the call never clears them), whose value does not depend on the order of the ORs.
 *
 * ---- tg_basis_inverse_i32 ----
 *
 * Semantics, as in unbounded integers, for triple n and each mode x of it, with L = lower[n][x], U = upper[n][x]:
 *
 * Substitution.  X = L^-1 column by column, forward:  X[r][c] = L[r][r] * ((r == c) - sum_{c <= k < r} L[r][k] X[k][c])
 *   for r >= c, 0 above the diagonal.  Y = U^-1 column by column, backward:
 *   Y[r][c] = U[r][r] * ((r == c) - sum_{r < k <= c} U[r][k] Y[k][c]) for r <= c, 0 below.  The only division is by a
 *   diagonal entry +-1, which is the multiplication by it.  The triangle that ought to be zero (the upper one of L, the
 *   lower one of U) is NOT READ.  inv_out[n][x] = Y * X = U^-1 L^-1 = (L U)^-1.
 *
 * Bad triples.  A triple is bad when a diagonal entry of any of its six factors is not +-1 (TG_BASIS_BAD_DIAGONAL);
 *   nothing else is looked at for such a triple.  A triple whose diagonals are all +-1 is bad when any entry of one of
 *   its six X, Y has magnitude >= 2^28, or any entry of one of its three products lies outside int32
 *   (TG_BASIS_BAD_RANGE).  A bad triple gives all three matrices of inv_out[n] zero and bad[n] = 1, and leaves every
 *   other triple untouched; a good one gives bad[n] = 0.
 *
 * Why 64-bit arithmetic is exact.  An accepted entry of X or Y is below 2^28 in magnitude.  A substitution sum has at
 *   most TG_MAX_S - 1 = 31 products of an int8 (at most 2^7) by an accepted entry: below 31 * 2^35 < 2^40; the
 *   multiplication by the diagonal +-1 changes nothing.  A product entry has at most 32 products of two accepted
 *   entries: below 32 * 2^56 = 2^61.  So an implementation in int64 that replaces an out-of-range entry by 0 and carries
 *   on never wraps, and it flags exactly the triples the unbounded rule flags: the first entry out of range, in the
 *   order of the dependencies, is computed from accepted entries alone and is therefore the exact one; and where no
 *   entry is out of range nothing was replaced.  What it computes after a replacement is discarded: the triple is
 *   zeroed anyway.
 *
 * ---- tg_solution_rebase ----
 *
 * Semantics, for row m with L = lengths[m] and g = index[m] (g = m when index is NULL):
 *
 * Terms.  For each term t < L: f = tok - shift in 32 bits; for each mode x in {0,1,2} with the block
 *   f_x = f[xS:(x+1)S]:  f'_x[a] = sum_b mats[g][x][a][b] * f_x[b], computed in 64 bits, which cannot wrap:
 *   |mats| <= 2^31, |f| <= 128 + 64 = 192, at most 32 products: 2^31 * 192 * 32 < 2^44.  out = f' + shift.
 *   The rows t >= L of tokens[m] are not read; in tokens_out[m] they are zero bytes (the padding
 *   RolloutResult.solutions() uses).  lengths_out[m] = L, bad[m] = 0.
 *
 * Bad rows.  A row is bad if L < 0 or L > K (TG_REBASE_BAD_LENGTH), if g < 0 or g >= G (TG_REBASE_BAD_INDEX; a row can
 *   set both), or -- length and index being good -- if any `out` value of a term t < L lies outside [-128,127]
 *   (TG_REBASE_BAD_RANGE).  Length and index are checked before they address anything.  A bad row is all zero bytes in
 *   tokens_out, has lengths_out[m] = 0 and bad[m] = 1, and leaves every other row untouched: the row's range flag is
 *   settled before anything of the row is stored.
 *
 * With the inverse of a basis as `mats` this is the map back described at the top; with the basis itself (widened to
 * int32) it moves a known factorisation INTO the basis, (u,v,w) -> (Au,Bv,Cw), as tg_gen_demos_i8 does for its own.
 */
#ifndef TENSOR_GAME_BASES_H_
#define TENSOR_GAME_BASES_H_

#include "tensor_game.h"
#include "tensor_game_solutions.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_BASIS_BAD_DIAGONAL 1 /* bits of *status of tg_basis_inverse_i32 */
#define TG_BASIS_BAD_RANGE 2
#define TG_REBASE_BAD_LENGTH 1  /* bits of *status of tg_solution_rebase */
#define TG_REBASE_BAD_INDEX 2
#define TG_REBASE_BAD_RANGE 4

/* Host only, no device work: the size checks of tg_basis_inverse_i32 alone.  N >= 0, 1 <= S <= TG_MAX_S. */
int tg_basis_inverse_check(int64_t N, int S);

/* Host only, no device work: the size checks of tg_solution_rebase alone.  M >= 0, 1 <= K <= TG_SOL_MAX_K,
 * 1 <= S <= TG_MAX_S, G >= 1 unless M = 0, 0 <= shift <= TG_SOL_MAX_SHIFT. */
int tg_solution_rebase_check(int64_t M, int K, int S, int64_t G, int shift);

/* The inverse semantics above for N triples, in ONE kernel launch (a workgroup per triple, a wavefront per matrix, a
 * lane per column of the substitution).
 *   lower, upper: int8 (N,3,S,S), the L and U tg_sample_basis_i8 emits, any alignment.
 *   inv_out: int32 (N,3,S,S).  bad: uint8 (N) or NULL.  status: uint32 (1) or NULL.
 * N = 0 returns 0 at once. */
int tg_basis_inverse_i32(const int8_t* lower, const int8_t* upper, int64_t N, int S, int32_t* inv_out, uint8_t* bad,
                         uint32_t* status, tg_stream_t stream);

/* The rebase semantics above for M lists, in ONE kernel launch (a wavefront per list, the row's three matrices staged
 * once in LDS, a lane per output position).
 *   tokens: int8 (M,K,3S) = cat(u,v,w) + shift as RolloutResult.solutions() returns them, any alignment.
 *   lengths: int64 (M).  mats: int32 (G,3,S,S).  index: int64 (M), or NULL: row m uses triple m, which needs G == M.
 *   tokens_out: int8 (M,K,3S), out of place (tokens_out == tokens is refused), any alignment.  lengths_out: int64 (M).
 *   bad: uint8 (M) or NULL.  status: uint32 (1) or NULL.
 * M = 0 returns 0 at once. */
int tg_solution_rebase(const int8_t* tokens, const int64_t* lengths, const int32_t* mats, const int64_t* index, int64_t M,
                       int K, int S, int64_t G, int shift, int8_t* tokens_out, int64_t* lengths_out, uint8_t* bad,
                       uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_BASES_H_ */
