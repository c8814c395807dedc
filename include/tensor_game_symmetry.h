/*
 * tensor_game_symmetry.h -- C ABI of libtensorgame.so: symmetry augmentation of training items.
 *
 * The reference has no counterpart: it trains on the items as generated.  The subgroup of the tensor's symmetries that
 * maps every (state, action) item to an item whose tokens stay in the vocabulary is the signed permutations of each
 * mode times the six permutations of the three modes; it keeps every value in int8 and is exact and invertible.
 * (tg_change_basis_i8 applies a general GL(S,Z) basis to a TARGET; that pushes action tokens out of the vocabulary.)
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).
 *
 * The group action.  An element g for one item is a mode permutation rho in S_3, three index permutations
 * pi_0, pi_1, pi_2 in S_S and three sign vectors s_0, s_1, s_2 in {+1,-1}^S.  Output mode m takes input mode rho[m].
 * Every frame f of the item (all T frames use the same g):
 *   out[f][a0,a1,a2] = s_0[a0] * s_1[a1] * s_2[a2] * in[f][b0,b1,b2]     with b_{rho[m]} = pi_m[a_m]   (m = 0,1,2)
 * The action's tokens, block m, position a:
 *   out_tok[m*S + a] = s_m[a] * (in_tok[rho[m]*S + pi_m[a]] - shift) + shift
 * With in = u_0 (x) u_1 (x) u_2 this gives out = u^g_0 (x) u^g_1 (x) u^g_2, so the action on states and on actions
 * commutes with the step.  Scalars and rewards are unchanged and do not pass through these entries.
 *
 * Encoding.  sym is uint8 (N, 3S+1), C-contiguous.  sym[n][0] is the code of rho, 0..5, the lexicographic rank of
 * (rho[0],rho[1],rho[2]): 0 = (0,1,2), 1 = (0,2,1), 2 = (1,0,2), 3 = (1,2,0), 4 = (2,0,1), 5 = (2,1,0).
 * sym[n][1 + m*S + a] = pi_m[a] | (0x80 if s_m[a] = -1); S <= TG_MAX_S = 32 fits in the low 7 bits.
 */
#ifndef TENSOR_GAME_SYMMETRY_H_
#define TENSOR_GAME_SYMMETRY_H_

#include "tensor_game.h"
#include "tensor_game_demos.h" /* TG_DEMO_MAX_T */

#ifdef __cplusplus
extern "C" {
#endif

#define TG_SYM_MODES 1 /* flags of tg_symmetry_sample: draw mode permutations */
#define TG_SYM_PERMS 2 /* ... index permutations */
#define TG_SYM_SIGNS 4 /* ... signs */

/* frames_out[n], actions_out[n] = sym[n] applied to frames_in[n], actions_in[n] (the group action above).
 * frames_in: int8 (N,T,S,S,S), C-contiguous, any alignment.  actions_in: int8 (N,3S); may be NULL together with
 * actions_out.  frames_out: C-contiguous (N,T,S,S,S) of out_dtype 0 = float32, 1 = float16, 2 = bfloat16 (the int8
 * value, exact in all three, as tg_demo_items) or 3 = int8, aligned to its element size only.  actions_out: int8 (N,3S).
 * Out of place only: frames_out == frames_in or actions_out == actions_in (non-NULL) is refused with TG_ERR_INVALID.
 * Overflow: the only ways to leave int8 are the negation of a frame entry -128 and a negated token 2*shift - tok
 * outside [-128,127].  Both wrap in two's complement and set overflow[n] (uint8 (N), may be NULL), sticky, for that
 * item only.
 * Bad rows: a row of sym whose rho code is above 5 or with any index >= S gives an all-zero item (frames and action),
 * sets bit 0 of *status (uint32, may be NULL) and leaves the other items untouched; the row is checked before any of
 * its bytes addresses anything.  A row whose indices are in range but REPEAT is not checked: it is applied as the
 * gather it describes (and is then not invertible).
 * Sizes: 1 <= S <= TG_MAX_S, 1 <= T <= TG_DEMO_MAX_T; N = 0 is a no-op.  One kernel launch. */
int tg_symmetry_apply(const int8_t* frames_in, const int8_t* actions_in, const uint8_t* sym, int64_t N, int T, int S,
                      int shift, int out_dtype, void* frames_out, int8_t* actions_out, uint8_t* overflow,
                      uint32_t* status, tg_stream_t stream);

/* One group element per item, drawn for the GLOBAL item id = item_offset + n, so any split of a range of ids over
 * calls or ranks gives the same bytes.  sym_out: uint8 (N, 3S+1).
 * Generator: Philox-4x32-10, key (seed_lo, seed_hi), counter (id_lo, id_hi, block, 0x53000000); block b yields the
 * 32-bit words w[4b .. 4b+3]; 3S+1 words in all:
 *   rho code = (w[0] * 6) >> 32                                                     (64-bit product)
 *   mode m = 0,1,2: pi_m = identity; for a = S-1 down to 1:
 *       j = (w[1 + m*S + (S-1-a)] * (a+1)) >> 32;  swap pi_m[a] and pi_m[j]          (Fisher-Yates)
 *   sign of position a of mode m = bit a of w[1 + m*S + (S-1)], 1 meaning -1.
 * The multiply-shift maps 2^32 words onto a+1 <= S values, so a value's probability is off the uniform one by at most
 * 2^-32, and a permutation's by at most S * 2^-32 relative: a bias of at most S * 2^-32.
 * flags: TG_SYM_MODES | TG_SYM_PERMS | TG_SYM_SIGNS; a part whose bit is clear is drawn and then replaced by the
 * identity, so the stream position never depends on the flags.  Other bits are refused.
 * Sizes: 1 <= S <= TG_MAX_S; N = 0 is a no-op.  One kernel launch. */
int tg_symmetry_sample(uint8_t* sym_out, int64_t N, int S, uint64_t seed, uint64_t item_offset, int flags,
                       tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_SYMMETRY_H_ */
