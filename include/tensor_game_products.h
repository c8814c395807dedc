/*
 * tensor_game_products.h -- C ABI of libtensorgame.so: the R block products of a bilinear algorithm for <n,m,p> on
 * bfloat16 or float16 operands, in ONE kernel launch.  The block combinations of tensor_game_rect.h are formed while the
 * product loads its tiles and are never written to memory; the products are accumulated in float32 on the matrix cores.
 * What remains of a matrix multiplication is tg_bilinear_rect_decode_f32 on the grid n x p.
 *
 * Convention: that of tensor_game_rect.h, word for word.  <n,m,p>: A is cut on the grid n x m with part 0, B on the grid
 *   m x p with part 1; a matrix of rows x cols on a grid gr x gc is gr x gc row-major blocks of (rows / gr) x (cols / gc),
 *   block e being rows (e / gc)*(rows / gr) .. and columns (e % gc)*(cols / gc) ..  The coefficient of term r, part d and
 *   block e is c_r[d][e] = tokens[r][d*S + e] - shift, taken in 32 bits, for e < gr*gc; no entry of a row at or beyond
 *   d*S + gr*gc is read for part d, part 2 is not read at all, and only the first R rows are read.  A token row is 3S
 *   bytes; max(n*m, m*p, n*p) <= S <= TG_MAX_S.  The square case is n = m = p, S = n*n.
 *
 * Shapes.  A: `batch` matrices of P x Q, element (y, x) of matrix b at A[b*stride_a + y*lda + x]; B: Q x T, at
 *   B[b*stride_b + y*ldb + x] (strides in elements of H).  h = P / n, q = Q / m, w = T / p.  M: contiguous float32
 *   (batch, R, h, w).  Any 2-byte aligned operand pointer, any lda >= Q and ldb >= T are legal; every shape >= 1 is.
 *
 * Arithmetic rule.  H is the operand type: bfloat16 (_bf16) or IEEE binary16 (_f16), passed as its 16 bits.
 *   1. An element of H converts to float32 exactly.
 *   2. Ahat_r[y][x] = rn_H(acc), where acc is the float32 block combination of A by rules 1-5 of tensor_game_rect.h: the
 *      accumulator starts at +0; the terms are taken in ascending e; a zero coefficient contributes nothing and its
 *      operand does not enter the sum, so a NaN or an infinity behind it never enters; a non-zero term is
 *      t = round(c * x) in float32, then the accumulator becomes round(acc + t) in float32, round to nearest, ties to even;
 *      there is no fused multiply-add.  rn_H is IEEE round-to-nearest-even from float32 to H, with overflow to infinity.
 *      Bhat_r is defined likewise from B and part 1.  Every bit of Ahat_r and Bhat_r is thereby a function of the inputs
 *      alone.
 *   3. M[b][r][y][x] = sum_k Ahat_r[y][k] * Bhat_r[k][x], k = 0 .. q-1.  Each product is exact in float32.  The sum is
 *      accumulated in float32 on the matrix cores; the order and the rounding of partial sums are not fixed.  The contract
 *      is |M - s| <= q * 2^-23 * sum_k |Ahat_r[y][k] * Bhat_r[k][x]|, s being the real sum: at most q - 1 additions of one
 *      unit in the last place each, which covers a truncating adder as well as a rounding one.  The bound is derived, not
 *      measured.
 *   4. Consequences that are part of the contract: where every partial sum in every order is an integer below 2^24, M is
 *      exact.  The same arguments give the same bits on every call: there are no atomics and no split-K.  The load path
 *      (below) changes no bit.  The sign of a zero result and the payload of a NaN are not defined.  Denormals, in H or
 *      in float32, are outside the rule.
 *
 * Load path, decided once per call on the host, per operand, from the arguments alone: 16-byte loads for an operand whose
 *   pointer is 16-byte aligned and whose ld, batch stride (when batch > 1) and block width (q for A, w for B) are
 *   multiples of 8 elements; single elements otherwise.
 *
 * The input ranges (the matrices read, and the R rows of tokens, R*3S bytes) must not overlap M; an overlap is refused.
 * All index arithmetic is 64-bit, and no size is bounded by a grid dimension.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.  The reference has no counterpart.
 */
#ifndef TENSOR_GAME_PRODUCTS_H_
#define TENSOR_GAME_PRODUCTS_H_

#include "tensor_game_solutions.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no device work: the size checks of the entries below and nothing else.  n, m, p >= 1; n*m, m*p, n*p <= S <=
 * TG_MAX_S; 1 <= R <= TG_SOL_MAX_K; 0 <= shift <= TG_SOL_MAX_SHIFT; batch >= 0; P, Q, T positive multiples of n, m, p;
 * lda >= Q, ldb >= T; stride_a >= P * lda and stride_b >= Q * ldb when batch > 1; and every byte offset of A, B and M
 * inside int64. */
int tg_bilinear_products_check(int64_t batch, int64_t P, int64_t Q, int64_t T, int64_t lda, int64_t stride_a, int64_t ldb,
                               int64_t stride_b, int R, int S, int n, int m, int p, int shift);

/* M[b][r] = Ahat_r * Bhat_r for every b < batch and r < R, by the rule above.  batch = 0 returns 0 at once.  Refused
 * beyond the size checks: a null A, B, tokens or M; A or B not 2-byte aligned; M not 4-byte aligned; M overlapping A, B or
 * the R token rows. */
int tg_bilinear_products_bf16(const uint16_t* A, const uint16_t* B, int64_t batch, int64_t P, int64_t Q, int64_t T,
                              int64_t lda, int64_t stride_a, int64_t ldb, int64_t stride_b, const int8_t* tokens, int R,
                              int S, int n, int m, int p, int shift, float* M, tg_stream_t stream);
int tg_bilinear_products_f16(const uint16_t* A, const uint16_t* B, int64_t batch, int64_t P, int64_t Q, int64_t T,
                             int64_t lda, int64_t stride_a, int64_t ldb, int64_t stride_b, const int8_t* tokens, int R,
                             int S, int n, int m, int p, int shift, float* M, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_PRODUCTS_H_ */
