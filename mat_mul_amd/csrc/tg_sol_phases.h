// tg_sol_phases.h -- the phases the kernels over an action list in LDS share (tg_solutions.hip, tg_orbits.hip): the
// workgroup sum and the exact verifier.  NT = the threads of the workgroup, t = this thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tensor_game.h"
#include "tg_device.h"

namespace tg {

constexpr int kSolWRow = TG_MAX_S;  // bytes per term of the verifier's padded copy of the w tokens

// the workgroup's sum of x (uniform result); `red` holds NT words
template <int NT>
__device__ __forceinline__ uint64_t sol_block_sum(uint64_t x, uint64_t* red, int t) {
  red[t] = x;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const uint64_t r = red[0];
  __syncthreads();
  return r;
}

// The number of non-zero entries of target - sum_r u (x) v (x) w over this thread's rows (i, j), for S <= 8 * CH.
// |p| <= 192^2 and a token is an int8, so both products are exact 24-bit multiplies; |sum p * w| <= 256 * 192^2 * 128
// and |shift * sum p| <= 64 * 256 * 192^2 stay below 2^31, and their difference is the exact sum of the terms.
template <int NT, int CH>
__device__ __forceinline__ int sol_residual_nnz(const int8_t* tok, const int8_t* wq, const int8_t* target, int L, int S,
                                                int shift, int t) {
  const int A3 = 3 * S;
  int nnz = 0;
  for (int ij = t; ij < S * S; ij += NT) {
    const int i = ij / S, j = ij - i * S;
    int acc[8 * CH] = {};
    int psum = 0;
    for (int r = 0; r < L; ++r) {
      const int8_t* row = tok + r * A3;
      const int p = mul24_pinned(row[i] - shift, row[S + j] - shift);
      psum += p;
      const uint2* w = reinterpret_cast<const uint2*>(wq + r * kSolWRow);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const uint2 q = w[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[8 * c + k] = mad24_pinned(p, sbyte(q.x, k), acc[8 * c + k]);
          acc[8 * c + 4 + k] = mad24_pinned(p, sbyte(q.y, k), acc[8 * c + 4 + k]);
        }
      }
    }
    const int off = shift * psum;
#pragma unroll
    for (int e = 0; e < 8 * CH; ++e)
      if (e < S) nnz += (target[ij * S + e] - (acc[e] - off)) != 0;
  }
  return nnz;
}

// the verifier's copy of the w tokens of L terms (the bytes beyond l = S - 1 only feed entries that are not counted)
template <int NT>
__device__ __forceinline__ void sol_stage_w(const int8_t* tok, int8_t* wq, int L, int S, int t) {
  const int A3 = 3 * S;
  for (int x = t; x < L * kSolWRow; x += NT) {
    const int r = x / kSolWRow, l = x - r * kSolWRow;
    wq[x] = l < S ? tok[r * A3 + 2 * S + l] : static_cast<int8_t>(0);
  }
}

// the exact residual's non-zero count over this thread's rows: the dispatch on S (uniform)
template <int NT>
__device__ __forceinline__ int sol_verify(const int8_t* tok, const int8_t* wq, const int8_t* target, int L, int S, int shift,
                                          int t) {
  switch ((S + 7) / 8) {
    case 1: return sol_residual_nnz<NT, 1>(tok, wq, target, L, S, shift, t);
    case 2: return sol_residual_nnz<NT, 2>(tok, wq, target, L, S, shift, t);
    case 3: return sol_residual_nnz<NT, 3>(tok, wq, target, L, S, shift, t);
    default: return sol_residual_nnz<NT, 4>(tok, wq, target, L, S, shift, t);
  }
}

}  // namespace tg
