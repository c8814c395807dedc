/*
 * tensor_game_orbits.h -- C ABI of libtensorgame.so: the canonical form of a factorisation modulo a set of symmetries
 * of its target.
 *
 * tg_solution_canon (tensor_game_solutions.h) factors out term order, signs inside a term, null terms and cancelling
 * pairs.  Two lists can still be the same factorisation moved by a symmetry of the target: <2,2,2> has 1 536 signed
 * index permutations and mode permutations that keep the vocabulary, so one Strassen-type algorithm has hundreds of
 * plain canonical forms.  tg_orbit_canon takes the smallest plain form over a set of group elements the caller
 * supplies, and tg_orbit_fixes tells whether every element of that set fixes a target.  The reference has no
 * counterpart.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * The set.  sym is uint8 (G, 3S+1), C-contiguous, in exactly the encoding of tensor_game_symmetry.h: byte 0 is the
 *   code of the mode permutation rho (0..5), byte 1 + m*S + a = pi_m[a] | 0x80 for s_m[a] = -1.  The same bytes feed
 *   tg_symmetry_apply.  A row is BAD when its rho code is above 5 or any index is >= S; it is checked before it
 *   addresses anything.  Indices that are in range but REPEAT are not checked (as in tg_symmetry_apply): the row is
 *   applied as the gather it describes.  The set need not be closed and need not hold the identity: the entries work on
 *   what they are given.
 *
 * The action on a list.  Element g maps the factor values f = tok - shift of a term, taken in 32 bits, to
 *   f^g[m*S + a] = s_m[a] * f[rho[m]*S + pi_m[a]]  (the token rule of tensor_game_symmetry.h without its int8
 *   narrowing); g.X is the list of the mapped terms.  If g fixes T and X sums to T, g.X sums to T.
 *
 * tg_orbit_canon, for list m with L = lengths[m]:
 *   residual_nnz[m] is that of tg_solution_canon: computed from the ORIGINAL terms against targets[m].
 *   For every g, C_g = steps 1-5 of tensor_game_solutions.h's canonical form applied to g.X, as a row of K terms of
 *   tokens (value + shift) with zero bytes behind its rank.  canon[m] is the smallest C_g, rows compared byte by byte
 *   as signed tokens, lexicographically ascending.  For a set of signed permutations the rank is the same for every g
 *   (g is a bijection on terms and commutes with nullness, sign normalisation and equality), so this compares the
 *   rank * 3S values (token - shift) in canonical order.  rank[m] is the rank of that row, key[m] the key rule of
 *   tensor_game_solutions.h on it, which[m] the smallest index g that attains the minimum and stab[m] the number of g
 *   that attain it: the size of the list's own stabiliser inside the set when the set is a group.
 *   The entry does not look at whether g fixes the target: that is tg_orbit_fixes' question.
 *
 * Bad rows.  Three sticky bits are ORed into *status, each decided on its own:
 *   TG_ORBIT_BAD_LENGTH    some list has L < 0 or L > K; that list is bad.  A length is checked before it addresses
 *                          anything.
 *   TG_ORBIT_BAD_NEGATION  some list with a good length has, for some good row g, a normalised value of step 2 (of a
 *                          term that step 1 keeps) or a negated w of step 4 (of a copy that is kept) whose token
 *                          value + shift lies outside [-128,127]; that list is bad.  (The values of g.X before step 2 are
 *                          32-bit and are not held to int8.)
 *   TG_ORBIT_BAD_GROUP     some row of sym is bad; every list is bad.
 *   A bad list gives rank 0, an all-zero canon row, key 0, residual_nnz -1, which -1 and stab 0.
 *
 * With G = 1 and the identity row every output shared with tg_solution_canon equals that entry's, bit for bit.
 * No floating point.  Every output is a function of its own list and the set alone: it depends neither on scheduling nor
 * on how the set is spread over workgroups (the slicing below).
 *
 * Not factored out: rescalings between the factors of a term, such as (2u) (x) v = u (x) (2v); and symmetries of the
 * target outside the set.  Finding a target's stabiliser is the caller's business.
 */
#ifndef TENSOR_GAME_ORBITS_H_
#define TENSOR_GAME_ORBITS_H_

#include "tensor_game.h"
#include "tensor_game_solutions.h" /* TG_SOL_MAX_K, TG_SOL_MAX_SHIFT */

#ifdef __cplusplus
extern "C" {
#endif

#define TG_ORBIT_MAX_G 2048         /* rows of sym */
#define TG_ORBIT_MAX_ROW 24576      /* K * 3S: TG_SOL_MAX_K * 3 * TG_MAX_S, the whole range of tg_solution_check */
#define TG_ORBIT_BAD_LENGTH 1       /* bits of *status (tg_orbit_canon) */
#define TG_ORBIT_BAD_NEGATION 2
#define TG_ORBIT_BAD_GROUP 4

/* Host only, no device work: the size checks of tg_orbit_canon alone.  M, K, S, shift as tg_solution_check;
 * 1 <= G <= TG_ORBIT_MAX_G; K * 3S <= TG_ORBIT_MAX_ROW (the kernel's LDS plan: four images of a row, 96 KiB at the
 * limit, which K <= TG_SOL_MAX_K and S <= TG_MAX_S cannot exceed). */
int tg_orbit_check(int64_t M, int K, int S, int shift, int G);

/* Host only: *bytes = the workspace with which tg_orbit_canon spreads the set of one list over several workgroups
 * (0 when M lists alone fill the device, or the set is too small to slice).  Sizes as tg_orbit_check. */
int tg_orbit_workspace_size(int64_t M, int K, int S, int G, int64_t* bytes);

/* fixes[m] = 1 iff every row g of sym fixes targets[m]:  s_0[a0] * s_1[a1] * s_2[a2] * T[b0,b1,b2] == T[a0,a1,a2] for
 * all entries, b_{rho[m]} = pi_m[a_m] as in tensor_game_symmetry.h, compared in int32 (so -128 needs no special case);
 * else 0.  targets: int8 (M,S,S,S), C-contiguous, any alignment.  sym: uint8 (G,3S+1).  fixes: uint8 (M).
 * A bad row of sym sets bit 0 of *status (uint32, may be NULL; sticky) and makes every fixes[m] = 0.
 * Sizes: M >= 0, 1 <= S <= TG_MAX_S, 1 <= G <= TG_ORBIT_MAX_G; M = 0 returns 0 at once.  ONE kernel launch. */
int tg_orbit_fixes(const int8_t* targets, int64_t M, int S, const uint8_t* sym, int G, uint8_t* fixes, uint32_t* status,
                   tg_stream_t stream);

/* The semantics above for M lists.  targets, tokens, lengths, canon, rank, key, residual_nnz, status: as
 * tg_solution_canon (targets and residual_nnz may both be NULL).  sym: uint8 (G,3S+1).  which, stab: int32 (M).
 * workspace: NULL, or 16-byte aligned with workspace_bytes >= tg_orbit_workspace_size's answer.  With NULL (or an
 * answer of 0) a workgroup walks the whole set for its list: ONE kernel launch.  Otherwise the set is cut into slices,
 * a workgroup finds the smallest row of its slice, and a second launch takes the smallest of the slice winners.  Both
 * give the same outputs.  M = 0 returns 0 at once. */
int tg_orbit_canon(const int8_t* targets, const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int S, int shift,
                   const uint8_t* sym, int G, int8_t* canon, int32_t* rank, uint64_t* key, int32_t* residual_nnz,
                   int32_t* which, int32_t* stab, uint32_t* status, void* workspace, int64_t workspace_bytes,
                   tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_ORBITS_H_ */
