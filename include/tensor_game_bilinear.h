/*
 * tensor_game_bilinear.h -- C ABI of libtensorgame.so: a factorisation of <n,n,n> used for what it is, a bilinear
 * algorithm that multiplies matrices with R block products where the schoolbook method takes n^3.
 *
 * The archive (tensor_game_solutions.h) proves lists against the matmul tensor in the index convention of
 * tg_reset_matmul_i8: a = i*n + j, b = j*n + k, c = i*n + k.  Read as an algorithm, a proven list of R terms
 * (u_r, v_r, w_r) multiplies matrices cut into n x n row-major blocks A_a, B_b, C_c:
 *
 *     C_c = sum_r w_r[c] * (sum_a u_r[a] * A_a) (sum_b v_r[b] * B_b)
 *
 * The two entries below are the linear halves of that formula: tg_bilinear_encode_E forms the R block combinations of
 * one operand (mode 0: u over the blocks of A; mode 1: v over the blocks of B), tg_bilinear_decode_E forms the S = n^2
 * blocks of C from the R block products.  The products themselves are the caller's (mat_mul_amd/bilinear.py hands them
 * to a batched GEMM, or encodes again: the output of one level is the input of the next).  Nothing here checks that the
 * list is a factorisation: the entries evaluate whatever coefficients they are given.  The reference has no counterpart.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.
 *
 * Lists.  tokens is int8 (K,3S) with S = n*n, as the archive stores a list; the first R rows are used and no other row is
 *   read.  The coefficient of term r, mode m (0: u, 1: v, 2: w) and index e is c_r[m][e] = tokens[r][m*S + e] - shift,
 *   taken in 32 bits.
 *
 * Matrices.  E is float (f32) or double (f64).  A strided operand is `batch` matrices of rows x cols: element (y, x) of
 *   matrix b is at X[b*batch_stride + y*ld + x] (strides in elements).  With h = rows / n and w = cols / n, block a of a
 *   matrix is its rows (a / n)*h .. (a / n)*h + h - 1 and columns (a % n)*w .. (a % n)*w + w - 1.  The block
 *   combinations are a contiguous E (batch,R,h,w).
 *
 * Encode.   Y[b][r][y][x] = sum_a c_r[mode][a] * X_b[(a / n)*h + y][(a % n)*w + x],  a = 0 .. S-1.
 * Decode.   C_b[(c / n)*h + y][(c % n)*w + x] = sum_r c_r[2][c] * M[b][r][y][x],     r = 0 .. R-1.
 *   Every element of every block of C is written, a block whose coefficients w_r[c] are all zero included: it gets +0.
 *   The same holds for an output Y[b][r] whose coefficients are all zero.
 *
 * Arithmetic rule, the same in both directions; it makes every output bit a function of the inputs alone:
 *   1. The accumulator starts at +0.
 *   2. The terms are taken in ascending a (encode) or ascending r (decode).
 *   3. A zero coefficient contributes nothing and its operand does not enter the sum: a NaN or an infinity in a block
 *      that no non-zero coefficient of an output uses does not reach that output.
 *   4. A non-zero term is t = round(c * x) in E (the coefficient converted to E exactly), then the accumulator becomes
 *      round(acc + t) in E; round is to nearest, ties to even.
 *   5. There is no fused multiply-add: the product is rounded before it is added.
 *   Denormal inputs and results are outside the rule.
 *
 * Pointers and layout.  Any element-aligned pointer and any ld >= cols are legal.  Accesses of 16 bytes are used only
 *   where both matrix pointers, ld, batch_stride (when batch > 1) and w allow them; the host decides once per call, and
 *   the result does not depend on it.  The input ranges (the matrices read, and the R rows of tokens) must not overlap
 *   the output range; the ranges are taken from the pointers and sizes and an overlap is refused.  All index arithmetic
 *   is 64-bit, and no size is bounded by a grid dimension: batch may be batch * R^(levels-1) of a recursive call.
 */
#ifndef TENSOR_GAME_BILINEAR_H_
#define TENSOR_GAME_BILINEAR_H_

#include "tensor_game_solutions.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_BILINEAR_MIN_N 2
#define TG_BILINEAR_MAX_N 5 /* S = 25: the largest matmul tensor of the project */

/* Host only, no device work: the size checks of the entries below and nothing else.  TG_BILINEAR_MIN_N <= n <=
 * TG_BILINEAR_MAX_N; 1 <= R <= TG_SOL_MAX_K; 0 <= shift <= TG_SOL_MAX_SHIFT; mode 0 or 1; batch >= 0; rows >= n and
 * cols >= n, each a multiple of n; ld >= cols; batch_stride >= rows * ld when batch > 1; elem_bytes 4 (f32) or 8 (f64);
 * and every byte offset of both operands inside int64.  (The decode entries have no mode and check with mode 0.) */
int tg_bilinear_check(int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R, int n, int mode,
                      int shift, int elem_bytes);

/* The R block combinations of `batch` strided matrices X, in ONE kernel launch.  Y: contiguous E (batch,R,rows/n,cols/n).
 * batch = 0 returns 0 at once. */
int tg_bilinear_encode_f32(const float* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride,
                           const int8_t* tokens, int R, int n, int mode, int shift, float* Y, tg_stream_t stream);
int tg_bilinear_encode_f64(const double* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride,
                           const int8_t* tokens, int R, int n, int mode, int shift, double* Y, tg_stream_t stream);

/* The S blocks of `batch` strided matrices C (rows x cols, ld, batch_stride) from the R block products M, a contiguous
 * E (batch,R,rows/n,cols/n), in ONE kernel launch.  batch = 0 returns 0 at once. */
int tg_bilinear_decode_f32(const float* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride,
                           const int8_t* tokens, int R, int n, int shift, float* C, tg_stream_t stream);
int tg_bilinear_decode_f64(const double* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride,
                           const int8_t* tokens, int R, int n, int shift, double* C, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_BILINEAR_H_ */
