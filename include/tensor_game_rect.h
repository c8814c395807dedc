/*
 * tensor_game_rect.h -- C ABI of libtensorgame.so: the rectangular matrix-multiplication tensor <n,m,p>, as a target and
 * as a bilinear algorithm.  The walks, the lift and the archive work on any S x S x S target; these entries build the
 * rectangular one and run a list proven against it, as tensor_game_bilinear.h does for <n,n,n>.
 *
 * Convention.  <n,m,p>: A is n x m, B is m x p, C is n x p, every index row-major:
 *
 *     a = i*m + j,   b = j*p + k,   c = i*p + k        (0 <= i < n, 0 <= j < m, 0 <= k < p)
 *
 *   With n = m = p this is the convention of tg_reset_matmul_i8.  The cube size is any S with max(n*m, m*p, n*p) <= S <=
 *   TG_MAX_S: the target has T[a][b][c] = 1 at those n*m*p cells and 0 everywhere else, the padding (an index at or
 *   beyond its mode's size) included.  Flips, pluses, reduction and the lift only combine vectors that exist, so a list
 *   that starts with zero padding keeps it.  A token row is 3S bytes as everywhere; mode d (0: u, 1: v, 2: w) uses its
 *   first n*m, m*p or n*p entries.  Restriction to those entries is linear: a list proven against the padded target is
 *   a factorisation of <n,m,p> after restriction, whatever its padding entries hold.
 *
 * The bilinear entries know a grid, not n, m, p: a matrix of rows x cols is cut into gr x gc row-major blocks of h x w,
 *   h = rows / gr, w = cols / gc; block e is rows (e / gc)*h .. (e / gc)*h + h - 1 and columns (e % gc)*w .. (e % gc)*w +
 *   w - 1.  A list for <n,m,p> encodes A on the grid n x m with part 0, B on m x p with part 1, and decodes C on n x p.
 *   The coefficient of term r, part d and block e is c_r[d][e] = tokens[r][d*S + e] - shift, taken in 32 bits, for
 *   e < gr*gc; no entry of a row at or beyond d*S + gr*gc is read for part d, and only the first R rows are read.
 *
 * Encode.   Y[b][r][y][x] = sum_e c_r[part][e] * X_b[(e / gc)*h + y][(e % gc)*w + x],   e = 0 .. gr*gc-1.
 * Decode.   C_b[(e / gc)*h + y][(e % gc)*w + x] = sum_r c_r[2][e] * M[b][r][y][x],      r = 0 .. R-1.
 *   Every element of every block of C is written, a block whose coefficients are all zero included: it gets +0.  The
 *   same holds for an output Y[b][r] whose coefficients are all zero.
 *
 * Arithmetic rule, the same in both directions and the same as tensor_game_bilinear.h; it makes every output bit a
 * function of the inputs alone:
 *   1. The accumulator starts at +0.
 *   2. The terms are taken in ascending e (encode) or ascending r (decode).
 *   3. A zero coefficient contributes nothing and its operand does not enter the sum: a NaN or an infinity in a block
 *      that no non-zero coefficient of an output uses does not reach that output.
 *   4. A non-zero term is t = round(c * x) in E (the coefficient converted to E exactly), then the accumulator becomes
 *      round(acc + t) in E; round is to nearest, ties to even.
 *   5. There is no fused multiply-add: the product is rounded before it is added.
 *   Denormal inputs and results are outside the rule.
 *   With gr = gc = n and S = n*n every output bit equals that of tg_bilinear_encode_E / tg_bilinear_decode_E.
 *
 * Matrices, pointers and layout: as in tensor_game_bilinear.h.  E is float (f32) or double (f64); element (y, x) of
 *   matrix b of the strided operand is at X[b*batch_stride + y*ld + x] (strides in elements), the block combinations are
 *   a contiguous E (batch,R,h,w).  Any element-aligned pointer and any ld >= cols are legal.  The input ranges (the
 *   matrices read, and the R rows of tokens, R*3S bytes) must not overlap the output range; an overlap is refused.  All
 *   index arithmetic is 64-bit, and no size is bounded by a grid dimension.
 *
 * Dispatch, decided once per call on the host, from the arguments alone; no output bit depends on it.  A thread owns one
 *   pack of consecutive x.  The pack is P bytes, P = 16 where gr*gc <= 25 and P = 8 where gr*gc > 25 (a thread holds
 *   gr*gc packs: narrower ones keep the largest grids in registers), where both matrix pointers are multiples of P bytes
 *   and ld, batch_stride (when batch > 1) and w are multiples of P / sizeof(E) elements; one element otherwise.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Every refusal happens
 * before any launch and names the argument.  The reference has no counterpart.
 */
#ifndef TENSOR_GAME_RECT_H_
#define TENSOR_GAME_RECT_H_

#include "tensor_game_solutions.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The target <n,m,p> in a cube of size S into B games of S^3 bytes, game_stride_bytes apart, in ONE kernel launch; the
 * bytes between games are not written.  n, m, p >= 1; n*m, m*p, n*p <= S <= TG_MAX_S; B >= 0 (B = 0 returns 0 at
 * once); game_stride_bytes >= S^3.  With n = m = p and S = n*n the bytes are those of tg_reset_matmul_i8. */
int tg_reset_matmul_rect_i8(int8_t* state_out, int64_t B, int n, int m, int p, int S, int64_t game_stride_bytes,
                            tg_stream_t stream);

/* Host only, no device work: the size checks of the entries below and nothing else.  gr, gc >= 1; gr*gc <= S <=
 * TG_MAX_S; 1 <= R <= TG_SOL_MAX_K; 0 <= shift <= TG_SOL_MAX_SHIFT; part 0, 1 or 2 (the encode entries take 0 or 1, the
 * decode entries check with 2); batch >= 0; rows a positive multiple of gr and cols a positive multiple of gc; ld >=
 * cols; batch_stride >= rows * ld when batch > 1; elem_bytes 4 (f32) or 8 (f64); and every byte offset of both operands
 * inside int64. */
int tg_bilinear_rect_check(int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R, int S,
                           int gr, int gc, int part, int shift, int elem_bytes);

/* The R block combinations of `batch` strided matrices X, in ONE kernel launch.  Y: contiguous E (batch,R,rows/gr,
 * cols/gc).  batch = 0 returns 0 at once. */
int tg_bilinear_rect_encode_f32(const float* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                int64_t batch_stride, const int8_t* tokens, int R, int S, int gr, int gc, int part,
                                int shift, float* Y, tg_stream_t stream);
int tg_bilinear_rect_encode_f64(const double* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                int64_t batch_stride, const int8_t* tokens, int R, int S, int gr, int gc, int part,
                                int shift, double* Y, tg_stream_t stream);

/* The gr*gc blocks of `batch` strided matrices C (rows x cols, ld, batch_stride) from the R block products M, a
 * contiguous E (batch,R,rows/gr,cols/gc), by part 2 of the list, in ONE kernel launch.  batch = 0 returns 0 at once. */
int tg_bilinear_rect_decode_f32(const float* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                int64_t batch_stride, const int8_t* tokens, int R, int S, int gr, int gc, int shift,
                                float* C, tg_stream_t stream);
int tg_bilinear_rect_decode_f64(const double* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                int64_t batch_stride, const int8_t* tokens, int R, int S, int gr, int gc, int shift,
                                double* C, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_RECT_H_ */
