// tg_sol_phases.h -- the phases the kernels over an action list in LDS share (tg_solutions.hip, tg_orbits.hip), each
// stated once: the workgroup sum, the exact verifier, the sort keys' byte map, the term signs, the rank sort and merge,
// the kept terms' offsets and the key of a finished image.  NT = the threads of the workgroup, t = this thread.
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

// The sort key of a term is its 3S token bytes, every byte with its sign bit flipped and every 8 bytes reversed, zero up to
// P = 3S rounded up to 8: unsigned compares of its 8-byte words order the values as signed.  Byte e of a term lies at:
__device__ __forceinline__ int sol_key_at(int e) { return (e & ~7) + 7 - (e & 7); }
// a token as its key byte, and back (the flip is its own inverse)
__device__ __forceinline__ uint8_t sol_key_flip(int v) { return static_cast<uint8_t>(v ^ 0x80); }

// Term t's sign from the codes of its three factors (per factor: 0 all zero, 1 as it was, 2 negated; | 4: a token left
// int8): tsign[t] = 0 for a null term, else sigma.  Returns whether a live term holds a token that left int8.
__device__ __forceinline__ int sol_term_sign(const uint8_t* fcode, int8_t* tsign, int L, int t) {
  if (t >= L) return 0;
  const int c0 = fcode[3 * t], c1 = fcode[3 * t + 1], c2 = fcode[3 * t + 2];
  const bool live = (c0 & 3) && (c1 & 3) && (c2 & 3);
  const int flips = ((c0 & 3) == 2) + ((c1 & 3) == 2) + ((c2 & 3) == 2);
  tsign[t] = live ? ((flips & 1) ? -1 : 1) : 0;
  return live && ((c0 | c1 | c2) & 4);
}

struct SolRank {
  bool kept;     // the term is live and one of the |c| copies its run keeps
  int place, c;  // its place among the live terms (distinct over them); its run's sum of signs
};

// The rank sort and merge, thread t = term t (K <= NT): t compares its key (P bytes, `keys` + t * P) with every other
// live term's, 8 bytes at a time with an early exit at the first differing word, and counts the lower ones, the equal
// ones before it and the run's sum of signs.  Writes keep[place] for a live term (the caller's barrier follows).
__device__ __forceinline__ SolRank sol_rank(const uint8_t* keys, const int8_t* tsign, uint8_t* keep, int L, int P, int t) {
  const bool live = t < L && tsign[t] != 0;
  int lower = 0, before = 0, c = 0;
  if (live) {
    const uint64_t* me = reinterpret_cast<const uint64_t*>(keys + t * P);
    for (int j = 0; j < L; ++j) {
      const int sj = tsign[j];
      if (sj == 0) continue;
      int d = 0;
      if (j != t) {
        const uint64_t* o = reinterpret_cast<const uint64_t*>(keys + j * P);
        for (int w = 0; w < P / 8 && d == 0; ++w) {
          const uint64_t x = o[w], y = me[w];
          d = x < y ? -1 : x > y ? 1 : 0;
        }
      }
      lower += d < 0;
      if (d == 0) {
        c += sj;
        before += j < t;
      }
    }
  }
  const bool kept = live && before < (c < 0 ? -c : c);
  const int place = lower + before;
  if (live) keep[place] = kept;
  return {kept, place, c};
}

// the kept terms at lower places: where a kept term goes in the output
__device__ __forceinline__ int sol_kept_below(const uint8_t* keep, int place) {
  int at = 0;
  for (int q = 0; q < place; ++q) at += keep[q];
  return at;
}

// The key of a finished image of n bytes (8-byte aligned, zero beyond n: the padding of the last word).  Uniform result.
template <int NT>
__device__ __forceinline__ uint64_t sol_image_key(const int8_t* img, int n, uint64_t* red, int t) {
  const int words = (n + 7) / 8;
  uint64_t h = 0;
  for (int k = t; k < words; k += NT)
    h += fmix64(reinterpret_cast<const uint64_t*>(img)[k] + static_cast<uint64_t>(k + 1) * 0x9E3779B97F4A7C15ull);
  return hash_finish(sol_block_sum<NT>(h, red, t), n);
}

}  // namespace tg
