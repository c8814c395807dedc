// tg_bilinear.hip -- include/tensor_game_bilinear.h: the two linear halves of a bilinear matrix-multiplication algorithm.
//
// encode: Y[b][r] = sum_a c_r[mode][a] * (block a of X_b);   decode: (block c of C_b) = sum_r c_r[2][c] * M[b][r].
//
// One thread owns one pack of consecutive x at a fixed (b, y): 16 bytes (float4 / double2) where the host found every
// address of the call 16-byte aligned, one element otherwise.  Encode reads its S = n^2 operand packs once, then writes
// the R results in a loop over r; decode reads the R packs once (a few ahead of their use) into S accumulators and
// writes them once.  So every input byte is read once and every output byte written once, and both kernels are bound by
// HBM unless the list is dense and large.  n is a template parameter: the S packs a thread holds are indexed by unrolled
// loops alone and stay in registers.
//
// The coefficient rows are the same for every thread: a workgroup copies the R rows of its mode into LDS once (the
// token bytes, a row padded to whole dwords), a wavefront reads a row's dwords through readfirstlane into SGPRs, and the
// test for a zero coefficient is a scalar branch over a term's multiplies and adds.  The header's rule 3 (a zero
// coefficient's operand does not enter the sum) is that branch; rule 5 (no fused multiply-add) is the pragma below,
// which holds for every operation written in this file (mul_rn and add_rn name the two roundings where they happen).
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_bilinear.h"
#include "tg_lists.h"

#pragma clang fp contract(off)

namespace tg {

constexpr int kBilinearBlock = 256;

template <typename E, int V>
struct alignas(sizeof(E) * V) Pack {
  E v[V];
};

struct BilinearArgs {
  const void* in;
  void* out;
  const int8_t* tokens;
  // of the strided operand (encode's input, decode's output), in elements; the dense one is (batch,R,h,w)
  int64_t h, w, ld, batch_stride;
  int64_t items;  // batch * h * (w / V)
  int R, shift, part;
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

template <int S>
struct Coefficients {
  static constexpr int kWords = (S + 3) / 4;  // dwords of a row's image
  int word[kWords];                           // wave-uniform: SGPRs

  // the workgroup's copy of rows 0 .. R-1, part `part` of tokens (any alignment) into `image`; ends with a barrier
  __device__ static void stage(int* image, const int8_t* tokens, int R, int part) {
    int8_t* bytes = reinterpret_cast<int8_t*>(image);
    for (int i = threadIdx.x; i < R * kWords * 4; i += kBilinearBlock) {
      const int r = i / (kWords * 4), e = i % (kWords * 4);
      bytes[i] = e < S ? tokens[r * 3 * S + part * S + e] : int8_t{0};
    }
    __syncthreads();
  }

  __device__ void load(const int* image, int r) {
#pragma unroll
    for (int j = 0; j < kWords; ++j) word[j] = __builtin_amdgcn_readfirstlane(image[r * kWords + j]);
  }

  __device__ int at(int e, int shift) const { return static_cast<int8_t>(word[e / 4] >> (8 * (e % 4))) - shift; }
};

// acc += c * x by the header's rule, for a non-zero c
template <typename E, int V>
__device__ inline void add_term(Pack<E, V>& acc, int c, const Pack<E, V>& x) {
  const E cf = static_cast<E>(c);
#pragma unroll
  for (int v = 0; v < V; ++v) acc.v[v] = add_rn(acc.v[v], mul_rn(cf, x.v[v]));
}

// item `it` of the grid-stride loop: matrix b, row y of a block, first column x of the pack
template <int V>
__device__ inline void item_position(int64_t it, const BilinearArgs& a, int64_t& b, int64_t& y, int64_t& x) {
  int64_t row, xv;
  split(it, a.w / V, row, xv);
  split(row, a.h, b, y);
  x = xv * V;
}

template <typename E, int N, int V>
__global__ __launch_bounds__(kBilinearBlock) void bilinear_encode_kernel(const BilinearArgs a) {
  constexpr int S = N * N;
  using P = Pack<E, V>;
  using Co = Coefficients<S>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a.tokens, a.R, a.part);
  const int64_t hw = a.h * a.w, hl = a.h * a.ld;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBilinearBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBilinearBlock) {
    int64_t b, y, x;
    item_position<V>(it, a, b, y, x);
    const E* src = static_cast<const E*>(a.in) + b * a.batch_stride + y * a.ld + x;
    P xs[S];
#pragma unroll
    for (int e = 0; e < S; ++e) xs[e] = *reinterpret_cast<const P*>(src + (e / N) * hl + (e % N) * a.w);
    E* dst = static_cast<E*>(a.out) + b * a.R * hw + y * a.w + x;
    for (int r = 0; r < a.R; ++r, dst += hw) {
      Co co;
      co.load(image, r);
      P acc;
#pragma unroll
      for (int v = 0; v < V; ++v) acc.v[v] = E{0};
#pragma unroll
      for (int e = 0; e < S; ++e) {
        const int c = co.at(e, a.shift);
        if (c != 0) add_term(acc, c, xs[e]);
      }
      *reinterpret_cast<P*>(dst) = acc;
    }
  }
}

template <typename E, int N, int V>
__global__ __launch_bounds__(kBilinearBlock) void bilinear_decode_kernel(const BilinearArgs a) {
  constexpr int S = N * N;
  constexpr int kAhead = S > 16 ? 2 : 4;  // products loaded ahead of their use; S accumulators leave less room at n = 5
  using P = Pack<E, V>;
  using Co = Coefficients<S>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a.tokens, a.R, a.part);
  const int64_t hw = a.h * a.w, hl = a.h * a.ld;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBilinearBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBilinearBlock) {
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
          const int k = co.at(c, a.shift);
          if (k != 0) add_term(acc[c], k, m[j]);
        }
      }
    }
    E* dst = static_cast<E*>(a.out) + b * a.batch_stride + y * a.ld + x;
#pragma unroll
    for (int c = 0; c < S; ++c) *reinterpret_cast<P*>(dst + (c / N) * hl + (c % N) * a.w) = acc[c];
  }
}

}  // namespace tg

namespace {

// What a call is, once its sizes passed: the element counts both operands span.
struct BilinearExtent {
  int64_t strided, dense;  // elements from the first to one past the last
};

bool mul_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }
bool add_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_add_overflow(a, b, out); }

int bilinear_sizes(const char* fn, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R,
                   int n, int mode, int shift, int elem_bytes, BilinearExtent* ext = nullptr) {
  if (n < TG_BILINEAR_MIN_N || n > TG_BILINEAR_MAX_N)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n=%d outside [%d,%d]", fn, n, TG_BILINEAR_MIN_N, TG_BILINEAR_MAX_N);
  if (R < 1 || R > TG_SOL_MAX_K) return tg_internal_fail(TG_ERR_INVALID, "%s: R=%d outside [1,%d]", fn, R, TG_SOL_MAX_K);
  if (shift < 0 || shift > TG_SOL_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_SOL_MAX_SHIFT);
  if (mode != 0 && mode != 1) return tg_internal_fail(TG_ERR_INVALID, "%s: mode=%d is neither 0 nor 1", fn, mode);
  if (batch < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld < 0", fn, (long long)batch);
  if (rows < n || rows % n)
    return tg_internal_fail(TG_ERR_INVALID, "%s: rows=%lld is no positive multiple of n=%d", fn, (long long)rows, n);
  if (cols < n || cols % n)
    return tg_internal_fail(TG_ERR_INVALID, "%s: cols=%lld is no positive multiple of n=%d", fn, (long long)cols, n);
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
           mul_fits(span, elem_bytes, &bytes) && mul_fits(batch, R, &dense) && mul_fits(dense, rows / n, &dense) &&
           mul_fits(dense, cols / n, &dense) && mul_fits(dense, elem_bytes, &bytes);
  }
  if (!fits)
    return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld, rows=%lld, ld=%lld out of range: a byte offset leaves int64",
                            fn, (long long)batch, (long long)rows, (long long)ld);
  if (ext) *ext = {span, dense};
  return TG_OK;
}

bool ranges_overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + static_cast<uintptr_t>(q_bytes) && b < a + static_cast<uintptr_t>(p_bytes);
}

// The one dispatch rule: 16-byte packs where every address of the call is a multiple of 16 bytes.
bool packs_of_16_bytes(const void* strided, const void* dense, int64_t batch, int64_t ld, int64_t batch_stride, int64_t w,
                       int elem_bytes) {
  const int V = 16 / elem_bytes;
  return aligned(strided, 16) && aligned(dense, 16) && ld % V == 0 && (batch <= 1 || batch_stride % V == 0) && w % V == 0;
}

template <typename E, bool kEncode, int N, int V>
int launch_bilinear(const char* fn, const tg::BilinearArgs& a, hipStream_t st) {
  const int64_t blocks = (a.items + tg::kBilinearBlock - 1) / tg::kBilinearBlock;
  const unsigned grid = grid_for(blocks, static_cast<int64_t>(8) * device_cu_count());  // the loops take the rest
  if constexpr (kEncode) return launch(fn, tg::bilinear_encode_kernel<E, N, V>, grid, tg::kBilinearBlock, 0, st, a);
  return launch(fn, tg::bilinear_decode_kernel<E, N, V>, grid, tg::kBilinearBlock, 0, st, a);
}

template <typename E, bool kEncode, int V>
int launch_bilinear_n(const char* fn, int n, const tg::BilinearArgs& a, hipStream_t st) {
  switch (n) {
    case 2: return launch_bilinear<E, kEncode, 2, V>(fn, a, st);
    case 3: return launch_bilinear<E, kEncode, 3, V>(fn, a, st);
    case 4: return launch_bilinear<E, kEncode, 4, V>(fn, a, st);
    default: return launch_bilinear<E, kEncode, 5, V>(fn, a, st);
  }
}

// Both directions: `strided` is the rows x cols operand (encode's X, decode's C), `dense` the (batch,R,h,w) one.
template <typename E, bool kEncode>
int bilinear_entry(const char* fn, const E* in, E* out, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                   int64_t batch_stride, const int8_t* tokens, int R, int n, int mode, int shift, tg_stream_t stream) {
  constexpr int eb = sizeof(E);
  const char* in_name = kEncode ? "X" : "M";
  const char* out_name = kEncode ? "Y" : "C";
  BilinearExtent ext;
  if (const int rc = bilinear_sizes(fn, batch, rows, cols, ld, batch_stride, R, n, mode, shift, eb, &ext)) return rc;
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
  if (ranges_overlap(tokens, static_cast<int64_t>(R) * 3 * n * n, out, out_bytes))
    return tg_internal_fail(TG_ERR_INVALID, "%s: tokens and %s overlap", fn, out_name);
  const int64_t h = rows / n, w = cols / n;
  const void* strided = kEncode ? static_cast<const void*>(in) : out;
  const void* dense = kEncode ? static_cast<const void*>(out) : in;
  const bool wide = packs_of_16_bytes(strided, dense, batch, ld, batch_stride, w, eb);
  constexpr int V = 16 / eb;
  const tg::BilinearArgs a{in, out, tokens, h, w, ld, batch > 1 ? batch_stride : 0, batch * h * (wide ? w / V : w),
                           R, shift, kEncode ? mode : 2};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) return launch_bilinear_n<E, kEncode, V>(fn, n, a, st);
  return launch_bilinear_n<E, kEncode, 1>(fn, n, a, st);
}

}  // namespace

extern "C" int tg_bilinear_check(int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R, int n,
                                 int mode, int shift, int elem_bytes) {
  return bilinear_sizes("tg_bilinear_check", batch, rows, cols, ld, batch_stride, R, n, mode, shift, elem_bytes);
}

extern "C" int tg_bilinear_encode_f32(const float* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                      int64_t batch_stride, const int8_t* tokens, int R, int n, int mode, int shift,
                                      float* Y, tg_stream_t stream) {
  return bilinear_entry<float, true>("tg_bilinear_encode_f32", X, Y, batch, rows, cols, ld, batch_stride, tokens, R, n,
                                     mode, shift, stream);
}

extern "C" int tg_bilinear_encode_f64(const double* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                      int64_t batch_stride, const int8_t* tokens, int R, int n, int mode, int shift,
                                      double* Y, tg_stream_t stream) {
  return bilinear_entry<double, true>("tg_bilinear_encode_f64", X, Y, batch, rows, cols, ld, batch_stride, tokens, R, n,
                                      mode, shift, stream);
}

extern "C" int tg_bilinear_decode_f32(const float* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                      int64_t batch_stride, const int8_t* tokens, int R, int n, int shift, float* C,
                                      tg_stream_t stream) {
  return bilinear_entry<float, false>("tg_bilinear_decode_f32", M, C, batch, rows, cols, ld, batch_stride, tokens, R, n,
                                      0, shift, stream);
}

extern "C" int tg_bilinear_decode_f64(const double* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                      int64_t batch_stride, const int8_t* tokens, int R, int n, int shift, double* C,
                                      tg_stream_t stream) {
  return bilinear_entry<double, false>("tg_bilinear_decode_f64", M, C, batch, rows, cols, ld, batch_stride, tokens, R, n,
                                       0, shift, stream);
}
