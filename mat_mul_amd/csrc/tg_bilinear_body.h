// tg_bilinear_body.h -- the one body of the bilinear encode and decode kernels and of their host path, shared by
// tg_bilinear.hip (the n x n grid, n a template parameter) and tg_rect.hip (a gr x gc grid taken at run time).
//
// encode: Y[b][r] = sum_e c_r[part][e] * (block e of X_b);   decode: (block e of C_b) = sum_r c_r[2][e] * M[b][r].
//
// One thread owns one pack of consecutive x at a fixed (b, y).  Encode reads its operand packs once, then writes the R
// results in a loop over r; decode reads the R packs once (a few ahead of their use) into one accumulator per block and
// writes them once.  So every input byte is read once and every output byte written once.  The packs a thread holds are
// indexed by unrolled loops alone and stay in registers.
//
// What a file brings is a grid policy G, static members only:
//   G::Args                   the kernel arguments; the body reads in, out, tokens, h, w, ld, batch_stride, items, R, shift
//   G::kSlots                 packs a thread holds: blocks of the grid, or the most a bucket of grids has
//   G::live(a, e)             whether slot e is a block of this call (loaded, stored)
//   G::pitch(a)               what block() wants computed once per thread, ahead of the loop over items
//   G::block(a, pitch, p, e)  where block e of a strided matrix starts, p being where block 0 does
//   G::image(a, r, e)         byte e of row r of the coefficient image: the token, or behind the list's entries a filler
//
// The coefficient rows are the same for every thread: a workgroup copies the R rows of its part into LDS once (the
// token bytes, a row padded to whole dwords), a wavefront reads a row's dwords through readfirstlane into SGPRs, and the
// test for a zero coefficient is a scalar branch over a term's multiplies and adds.  The headers' rule 3 (a zero
// coefficient's operand does not enter the sum) is that branch, and a slot that is not live reads as coefficient zero,
// so the same branch skips it; rule 5 (no fused multiply-add) is the pragma below, which holds for every operation
// written in this file (mul_rn and add_rn name the two roundings where they happen).
#pragma once
#include <hip/hip_runtime.h>

#include "tg_lists.h"

#pragma clang fp contract(off)

namespace tg {
namespace bilinear {

constexpr int kBlock = 256;

template <typename E, int V>
struct alignas(sizeof(E) * V) Pack {
  E v[V];
};

// The two roundings of rule 4.  Plain operators on purpose: the pragma above covers the operations written in this file,
// while __fmul_rn / __fadd_rn are a `*` and a `+` inside the HIP headers, compiled with contraction on, and fuse once
// they are inlined here (seen in the assembly: v_pk_fma_f32 and v_fma_f64 with a live addend).
template <typename E>
__device__ inline E mul_rn(E a, E b) {
  return a * b;
}
template <typename E>
__device__ inline E add_rn(E a, E b) {
  return a + b;
}

// v = q * d + r; in 32 bits where both fit (the 64-bit division is a long software routine)
__device__ inline void split(int64_t v, int64_t d, int64_t& q, int64_t& r) {
  if (((static_cast<uint64_t>(v) | static_cast<uint64_t>(d)) >> 32) == 0) {
    const uint32_t q32 = static_cast<uint32_t>(v) / static_cast<uint32_t>(d);
    q = q32;
    r = static_cast<uint32_t>(v) - q32 * static_cast<uint32_t>(d);
  } else {
    q = v / d;
    r = v - q * d;
  }
}

template <typename G>
struct Coefficients {
  static constexpr int kWords = (G::kSlots + 3) / 4;  // dwords of a row's image
  int word[kWords];                                   // wave-uniform: SGPRs

  // the workgroup's copy of rows 0 .. R-1 of the call's part (any alignment) into `image`; ends with a barrier
  __device__ static void stage(int* image, const typename G::Args& a) {
    int8_t* bytes = reinterpret_cast<int8_t*>(image);
    for (int i = threadIdx.x; i < a.R * kWords * 4; i += kBlock) bytes[i] = G::image(a, i / (kWords * 4), i % (kWords * 4));
    __syncthreads();
  }

  __device__ void load(const int* image, int r) {
#pragma unroll
    for (int j = 0; j < kWords; ++j) word[j] = __builtin_amdgcn_readfirstlane(image[r * kWords + j]);
  }

  __device__ int at(int e, int shift) const { return static_cast<int8_t>(word[e / 4] >> (8 * (e % 4))) - shift; }
};

// acc += c * x by the headers' rule, for a non-zero c
template <typename E, int V>
__device__ inline void add_term(Pack<E, V>& acc, int c, const Pack<E, V>& x) {
  const E cf = static_cast<E>(c);
#pragma unroll
  for (int v = 0; v < V; ++v) acc.v[v] = add_rn(acc.v[v], mul_rn(cf, x.v[v]));
}

// item `it` of the grid-stride loop: matrix b, row y of a block, first column x of the pack
template <int V, typename A>
__device__ inline void item_position(int64_t it, const A& a, int64_t& b, int64_t& y, int64_t& x) {
  int64_t row, xv;
  split(it, a.w / V, row, xv);
  split(row, a.h, b, y);
  x = xv * V;
}

template <typename E, typename G, int V>
__global__ __launch_bounds__(kBlock) void encode_kernel(const typename G::Args a) {
  constexpr int S = G::kSlots;
  using P = Pack<E, V>;
  using Co = Coefficients<G>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a);
  const int64_t hw = a.h * a.w, pitch = G::pitch(a);
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBlock) {
    int64_t b, y, x;
    item_position<V>(it, a, b, y, x);
    const E* src = static_cast<const E*>(a.in) + b * a.batch_stride + y * a.ld + x;
    P xs[S];
#pragma unroll
    for (int e = 0; e < S; ++e)
      if (G::live(a, e)) xs[e] = *reinterpret_cast<const P*>(G::block(a, pitch, src, e));
    E* dst = static_cast<E*>(a.out) + b * a.R * hw + y * a.w + x;
    for (int r = 0; r < a.R; ++r, dst += hw) {
      Co co;
      co.load(image, r);
      P acc;
#pragma unroll
      for (int v = 0; v < V; ++v) acc.v[v] = E{0};
#pragma unroll
      for (int e = 0; e < S; ++e) {
        const int c = co.at(e, a.shift);  // zero where the slot is not live
        if (c != 0) add_term(acc, c, xs[e]);
      }
      *reinterpret_cast<P*>(dst) = acc;
    }
  }
}

template <typename E, typename G, int V>
__global__ __launch_bounds__(kBlock) void decode_kernel(const typename G::Args a) {
  constexpr int S = G::kSlots;
  constexpr int kAhead = S > 16 ? 2 : 4;  // products loaded ahead of their use; many accumulators leave less room
  using P = Pack<E, V>;
  using Co = Coefficients<G>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a);
  const int64_t hw = a.h * a.w, pitch = G::pitch(a);
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBlock) {
    int64_t b, y, x;
    item_position<V>(it, a, b, y, x);
    const E* src = static_cast<const E*>(a.in) + b * a.R * hw + y * a.w + x;
    P acc[S];
#pragma unroll
    for (int c = 0; c < S; ++c)
#pragma unroll
      for (int v = 0; v < V; ++v) acc[c].v[v] = E{0};
    for (int r0 = 0; r0 < a.R; r0 += kAhead, src += kAhead * hw) {
      P m[kAhead] = {};
#pragma unroll
      for (int j = 0; j < kAhead; ++j)
        if (r0 + j < a.R) m[j] = *reinterpret_cast<const P*>(src + j * hw);
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        if (r0 + j >= a.R) break;
        Co co;
        co.load(image, r0 + j);
#pragma unroll
        for (int c = 0; c < S; ++c) {
          const int k = co.at(c, a.shift);  // zero where the slot is not live
          if (k != 0) add_term(acc[c], k, m[j]);
        }
      }
    }
    E* dst = static_cast<E*>(a.out) + b * a.batch_stride + y * a.ld + x;
#pragma unroll
    for (int c = 0; c < S; ++c)
      if (G::live(a, c)) *reinterpret_cast<P*>(G::block(a, pitch, dst, c)) = acc[c];
  }
}

// ---- the host path of both families: each entry makes its own leading checks, then these, in this order ----

// What a call is, once its sizes passed: the element counts both operands span.
struct Extent {
  int64_t strided, dense;  // elements from the first to one past the last
};

inline bool mul_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }
inline bool add_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_add_overflow(a, b, out); }

inline int check_rank_shift(const char* fn, int R, int shift) {
  if (R < 1 || R > TG_SOL_MAX_K) return tg_internal_fail(TG_ERR_INVALID, "%s: R=%d outside [1,%d]", fn, R, TG_SOL_MAX_K);
  if (shift < 0 || shift > TG_SOL_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_SOL_MAX_SHIFT);
  return TG_OK;
}

// batch, rows, cols, ld, elem_bytes, batch_stride and the overflow chain, for a grid of gr x gc blocks whose two sizes
// the entry calls gr_name and gc_name
inline int check_sizes(const char* fn, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R,
                       int gr, const char* gr_name, int gc, const char* gc_name, int elem_bytes, Extent* ext) {
  if (batch < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld < 0", fn, (long long)batch);
  if (rows < gr || rows % gr)
    return tg_internal_fail(TG_ERR_INVALID, "%s: rows=%lld is no positive multiple of %s=%d", fn, (long long)rows, gr_name,
                            gr);
  if (cols < gc || cols % gc)
    return tg_internal_fail(TG_ERR_INVALID, "%s: cols=%lld is no positive multiple of %s=%d", fn, (long long)cols, gc_name,
                            gc);
  if (ld < cols) return tg_internal_fail(TG_ERR_INVALID, "%s: ld=%lld < cols=%lld", fn, (long long)ld, (long long)cols);
  if (elem_bytes != 4 && elem_bytes != 8)
    return tg_internal_fail(TG_ERR_INVALID, "%s: elem_bytes=%d is neither 4 nor 8", fn, elem_bytes);
  // one matrix, then the batch, then the dense operand: every byte offset inside int64
  int64_t one, matrix, span = 0, dense = 0, bytes;
  bool fits = mul_fits(rows - 1, ld, &one) && add_fits(one, cols, &one) && mul_fits(rows, ld, &matrix);
  if (fits && batch > 1 && batch_stride < matrix)
    return tg_internal_fail(TG_ERR_INVALID, "%s: batch_stride=%lld < rows*ld=%lld", fn, (long long)batch_stride,
                            (long long)matrix);
  if (fits && batch > 0) {
    fits = mul_fits(batch - 1, batch > 1 ? batch_stride : 0, &span) && add_fits(span, one, &span) &&
           mul_fits(span, elem_bytes, &bytes) && mul_fits(batch, R, &dense) && mul_fits(dense, rows / gr, &dense) &&
           mul_fits(dense, cols / gc, &dense) && mul_fits(dense, elem_bytes, &bytes);
  }
  if (!fits)
    return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld, rows=%lld, ld=%lld out of range: a byte offset leaves int64",
                            fn, (long long)batch, (long long)rows, (long long)ld);
  if (ext) *ext = {span, dense};
  return TG_OK;
}

inline bool ranges_overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + static_cast<uintptr_t>(q_bytes) && b < a + static_cast<uintptr_t>(p_bytes);
}

// The one dispatch rule (stated in the headers): packs of `pack_bytes` where every address of the call is a multiple of it.
inline bool packs_of(int pack_bytes, const void* strided, const void* dense, int64_t batch, int64_t ld,
                     int64_t batch_stride, int64_t w, int elem_bytes) {
  const int V = pack_bytes / elem_bytes;
  return aligned(strided, pack_bytes) && aligned(dense, pack_bytes) && ld % V == 0 &&
         (batch <= 1 || batch_stride % V == 0) && w % V == 0;
}

template <typename E, bool kEncode, typename G, int V>
int launch_kernel(const char* fn, const typename G::Args& a, hipStream_t st) {
  const int64_t blocks = (a.items + kBlock - 1) / kBlock;
  const unsigned grid = grid_for(blocks, static_cast<int64_t>(8) * device_cu_count());  // the loops take the rest
  if constexpr (kEncode) return launch(fn, encode_kernel<E, G, V>, grid, kBlock, 0, st, a);
  return launch(fn, decode_kernel<E, G, V>, grid, kBlock, 0, st, a);
}

// Both directions of a call whose sizes passed (`ext`): `strided` is the rows x cols operand (encode's X, decode's C),
// `dense` the (batch,R,h,w) one.  `go(V, h, w, batch_stride, items)` fills the family's arguments and launches the kernel
// for packs of V elements: pack_bytes of them where the pack rule allows, one otherwise.
template <typename E, bool kEncode, typename Go>
int entry(const char* fn, const E* in, E* out, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride,
          const int8_t* tokens, int64_t token_bytes, int gr, int gc, int pack_bytes, const Extent& ext, Go&& go) {
  constexpr int eb = sizeof(E);
  const char* in_name = kEncode ? "X" : "M";
  const char* out_name = kEncode ? "Y" : "C";
  if (batch == 0) return TG_OK;
  if (!in) return tg_internal_fail(TG_ERR_INVALID, "%s: null %s", fn, in_name);
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!out) return tg_internal_fail(TG_ERR_INVALID, "%s: null %s", fn, out_name);
  if (!aligned(in, eb)) return tg_internal_fail(TG_ERR_INVALID, "%s: %s not %d-byte aligned", fn, in_name, eb);
  if (!aligned(out, eb)) return tg_internal_fail(TG_ERR_INVALID, "%s: %s not %d-byte aligned", fn, out_name, eb);
  const int64_t in_bytes = (kEncode ? ext.strided : ext.dense) * eb, out_bytes = (kEncode ? ext.dense : ext.strided) * eb;
  if (ranges_overlap(in, in_bytes, out, out_bytes))
    return tg_internal_fail(TG_ERR_INVALID, "%s: %s and %s overlap: in-place operation is not supported", fn, in_name,
                            out_name);
  if (ranges_overlap(tokens, token_bytes, out, out_bytes))
    return tg_internal_fail(TG_ERR_INVALID, "%s: tokens and %s overlap", fn, out_name);
  const int64_t h = rows / gr, w = cols / gc;
  const void* strided = kEncode ? static_cast<const void*>(in) : out;
  const void* dense = kEncode ? static_cast<const void*>(out) : in;
  const int V = packs_of(pack_bytes, strided, dense, batch, ld, batch_stride, w, eb) ? pack_bytes / eb : 1;
  return go(V, h, w, batch > 1 ? batch_stride : 0, batch * h * (w / V));
}

}  // namespace bilinear
}  // namespace tg
