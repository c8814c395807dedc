// tg_rect.hip -- include/tensor_game_rect.h: the rectangular target <n,m,p> and the two linear halves of a bilinear
// algorithm on a gr x gc grid of blocks.
//
// encode: Y[b][r] = sum_e c_r[part][e] * (block e of X_b);   decode: (block e of C_b) = sum_r c_r[2][e] * M[b][r].
//
// The kernels are those of tg_bilinear.hip with the grid taken at run time.  One thread owns one pack of consecutive x at
// a fixed (b, y); encode reads its gr*gc operand packs once and writes the R results in a loop over r, decode reads the
// R packs once (a few ahead of their use) into gr*gc accumulators and writes them once: every input byte is read once
// and every output byte written once.  There are about a hundred legal grids, so the kernels are not instantiated per
// grid: the template parameter is a bucket of the block count (4, 9, 16, 25, 32: the squares and TG_MAX_S), the arrays of
// packs have the bucket's size and are indexed by unrolled constants alone (registers, no scratch), and the live count
// gr*gc and the blocks' element offsets (computed once on the host, read from the kernel arguments) are wave-uniform.
// A block at or beyond the live count is neither loaded nor stored, and its coefficient reads as zero: the image of a
// row in LDS holds `shift` there, so the zero test that skips a term skips it too.
//
// The coefficient rows, the zero test (rule 3 of the header) and the two roundings (rules 4 and 5) are as in
// tg_bilinear.hip: the rows of the part in LDS once per workgroup, a row's dwords through readfirstlane into SGPRs, a
// scalar branch over a term's multiplies and adds, and plain `*` and `+` under the pragma below (__fmul_rn / __fadd_rn
// are a `*` and a `+` inside the HIP headers, compiled with contraction on, and fuse once they are inlined here).
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_rect.h"
#include "tg_lists.h"

#pragma clang fp contract(off)

namespace tg {
namespace rect {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = TG_MAX_S;  // of a grid: gr * gc <= S <= TG_MAX_S
constexpr int kWidePacksUpTo = 25;    // the header's dispatch rule: packs of 16 bytes up to here, of 8 bytes above

template <typename E, int V>
struct alignas(sizeof(E) * V) Pack {
  E v[V];
};

struct Args {
  const void* in;
  void* out;
  const int8_t* tokens;
  // of the strided operand (encode's input, decode's output), in elements; the dense one is (batch,R,h,w)
  int64_t h, w, ld, batch_stride;
  int64_t items;  // batch * h * (w / V)
  int R, S, shift, part;
  int live;                  // gr * gc
  int64_t at[kMaxBlocks];    // block e of a strided matrix starts (e / gc) * h * ld + (e % gc) * w elements in
};

struct ResetArgs {
  int8_t* out;
  int64_t B, stride;
  int n, m, p, S;
};

// T[a][b][c] of <n,m,p> for every byte of B games; the bytes between games are not touched
__global__ __launch_bounds__(kBlock) void reset_kernel(const ResetArgs a) {
  const int N = a.S * a.S * a.S;
  const int64_t total = a.B * N;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
       idx += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t g = idx / N;
    const int e = static_cast<int>(idx - g * N);
    const int x = e / (a.S * a.S), rem = e - x * a.S * a.S, y = rem / a.S, z = rem - y * a.S;
    // x = i*m + j, y = j*p + k, z = i*p + k; an index at or beyond its mode's size is padding
    const bool inside = x < a.n * a.m && y < a.m * a.p && z < a.n * a.p;
    a.out[g * a.stride + e] = inside && (x / a.m == z / a.p) && (x % a.m == y / a.p) && (y % a.p == z % a.p);
  }
}

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

template <int MAXB>
struct Coefficients {
  static constexpr int kWords = (MAXB + 3) / 4;  // dwords of a row's image
  int word[kWords];                              // wave-uniform: SGPRs

  // the workgroup's copy of entries 0 .. live-1 of part `part` of rows 0 .. R-1 (any alignment) into `image`, `shift`
  // (a zero coefficient) behind them; ends with a barrier
  __device__ static void stage(int* image, const Args& a) {
    int8_t* bytes = reinterpret_cast<int8_t*>(image);
    for (int i = threadIdx.x; i < a.R * kWords * 4; i += kBlock) {
      const int r = i / (kWords * 4), e = i % (kWords * 4);
      bytes[i] = e < a.live ? a.tokens[r * 3 * a.S + a.part * a.S + e] : static_cast<int8_t>(a.shift);
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
__device__ inline void item_position(int64_t it, const Args& a, int64_t& b, int64_t& y, int64_t& x) {
  int64_t row, xv;
  split(it, a.w / V, row, xv);
  split(row, a.h, b, y);
  x = xv * V;
}

// MINB: the smallest live count the host sends to this bucket; blocks below it are live without a test
template <typename E, int MINB, int MAXB, int V>
__global__ __launch_bounds__(kBlock) void encode_kernel(const Args a) {
  using P = Pack<E, V>;
  using Co = Coefficients<MAXB>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a);
  const int64_t hw = a.h * a.w;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBlock) {
    int64_t b, y, x;
    item_position<V>(it, a, b, y, x);
    const E* src = static_cast<const E*>(a.in) + b * a.batch_stride + y * a.ld + x;
    P xs[MAXB];
#pragma unroll
    for (int e = 0; e < MAXB; ++e)
      if (e < MINB || e < a.live) xs[e] = *reinterpret_cast<const P*>(src + a.at[e]);
    E* dst = static_cast<E*>(a.out) + b * a.R * hw + y * a.w + x;
    for (int r = 0; r < a.R; ++r, dst += hw) {
      Co co;
      co.load(image, r);
      P acc;
#pragma unroll
      for (int v = 0; v < V; ++v) acc.v[v] = E{0};
#pragma unroll
      for (int e = 0; e < MAXB; ++e) {
        const int c = co.at(e, a.shift);  // zero at and beyond a.live
        if (c != 0) add_term(acc, c, xs[e]);
      }
      *reinterpret_cast<P*>(dst) = acc;
    }
  }
}

template <typename E, int MINB, int MAXB, int V>
__global__ __launch_bounds__(kBlock) void decode_kernel(const Args a) {
  constexpr int kAhead = MAXB > 16 ? 2 : 4;  // products loaded ahead of their use; many accumulators leave less room
  using P = Pack<E, V>;
  using Co = Coefficients<MAXB>;
  __shared__ int image[TG_SOL_MAX_K * Co::kWords];
  Co::stage(image, a);
  const int64_t hw = a.h * a.w;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; it < a.items;
       it += static_cast<int64_t>(gridDim.x) * kBlock) {
    int64_t b, y, x;
    item_position<V>(it, a, b, y, x);
    const E* src = static_cast<const E*>(a.in) + b * a.R * hw + y * a.w + x;
    P acc[MAXB];
#pragma unroll
    for (int c = 0; c < MAXB; ++c)
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
        for (int c = 0; c < MAXB; ++c) {
          const int k = co.at(c, a.shift);  // zero at and beyond a.live
          if (k != 0) add_term(acc[c], k, m[j]);
        }
      }
    }
    E* dst = static_cast<E*>(a.out) + b * a.batch_stride + y * a.ld + x;
#pragma unroll
    for (int c = 0; c < MAXB; ++c)
      if (c < MINB || c < a.live) *reinterpret_cast<P*>(dst + a.at[c]) = acc[c];
  }
}

}  // namespace rect
}  // namespace tg

namespace {

namespace R = tg::rect;

// What a call is, once its sizes passed: the element counts both operands span.
struct Extent {
  int64_t strided, dense;  // elements from the first to one past the last
};

bool mul_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }
bool add_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_add_overflow(a, b, out); }

int rect_sizes(const char* fn, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int Rk, int S,
               int gr, int gc, int part, int max_part, int shift, int elem_bytes, Extent* ext = nullptr) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (gr < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: gr=%d < 1", fn, gr);
  if (gc < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: gc=%d < 1", fn, gc);
  if (gr > S || gc > S || gr * gc > S)
    return tg_internal_fail(TG_ERR_INVALID, "%s: gr*gc=%lld above S=%d", fn, (long long)gr * gc, S);
  if (Rk < 1 || Rk > TG_SOL_MAX_K) return tg_internal_fail(TG_ERR_INVALID, "%s: R=%d outside [1,%d]", fn, Rk, TG_SOL_MAX_K);
  if (shift < 0 || shift > TG_SOL_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_SOL_MAX_SHIFT);
  if (part < 0 || part > max_part) return tg_internal_fail(TG_ERR_INVALID, "%s: part=%d outside [0,%d]", fn, part, max_part);
  if (batch < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld < 0", fn, (long long)batch);
  if (rows < gr || rows % gr)
    return tg_internal_fail(TG_ERR_INVALID, "%s: rows=%lld is no positive multiple of gr=%d", fn, (long long)rows, gr);
  if (cols < gc || cols % gc)
    return tg_internal_fail(TG_ERR_INVALID, "%s: cols=%lld is no positive multiple of gc=%d", fn, (long long)cols, gc);
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
           mul_fits(span, elem_bytes, &bytes) && mul_fits(batch, Rk, &dense) && mul_fits(dense, rows / gr, &dense) &&
           mul_fits(dense, cols / gc, &dense) && mul_fits(dense, elem_bytes, &bytes);
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

// The one dispatch rule (stated in the header): packs of `pack_bytes` where every address of the call is a multiple of it.
bool packs_of(int pack_bytes, const void* strided, const void* dense, int64_t batch, int64_t ld, int64_t batch_stride,
              int64_t w, int elem_bytes) {
  const int V = pack_bytes / elem_bytes;
  return aligned(strided, pack_bytes) && aligned(dense, pack_bytes) && ld % V == 0 &&
         (batch <= 1 || batch_stride % V == 0) && w % V == 0;
}

template <typename E, bool kEncode, int MINB, int MAXB, int V>
int launch_rect(const char* fn, const R::Args& a, hipStream_t st) {
  const int64_t blocks = (a.items + R::kBlock - 1) / R::kBlock;
  const unsigned grid = grid_for(blocks, static_cast<int64_t>(8) * device_cu_count());  // the loops take the rest
  if constexpr (kEncode) return launch(fn, R::encode_kernel<E, MINB, MAXB, V>, grid, R::kBlock, 0, st, a);
  return launch(fn, R::decode_kernel<E, MINB, MAXB, V>, grid, R::kBlock, 0, st, a);
}

// the bucket of the live count, for packs of V elements where the bucket's pack rule allows them (else single elements)
template <typename E, bool kEncode>
int launch_bucket(const char* fn, bool packs, const R::Args& a, hipStream_t st) {
  constexpr int V16 = 16 / sizeof(E), V8 = 8 / sizeof(E);
#define TG_RECT_BUCKET(lo, hi, V)                                                \
  if (a.live <= hi)                                                              \
    return packs && V > 1 ? launch_rect<E, kEncode, lo, hi, V>(fn, a, st)        \
                          : launch_rect<E, kEncode, lo, hi, 1>(fn, a, st)
  TG_RECT_BUCKET(1, 4, V16);
  TG_RECT_BUCKET(5, 9, V16);
  TG_RECT_BUCKET(10, 16, V16);
  TG_RECT_BUCKET(17, R::kWidePacksUpTo, V16);
  TG_RECT_BUCKET(R::kWidePacksUpTo + 1, R::kMaxBlocks, V8);
#undef TG_RECT_BUCKET
  return tg_internal_fail(TG_ERR_INVALID, "%s: gr*gc=%d above %d", fn, a.live, R::kMaxBlocks);
}

// Both directions: `strided` is the rows x cols operand (encode's X, decode's C), `dense` the (batch,R,h,w) one.
template <typename E, bool kEncode>
int rect_entry(const char* fn, const E* in, E* out, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
               int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc, int part, int shift,
               tg_stream_t stream) {
  constexpr int eb = sizeof(E);
  const char* in_name = kEncode ? "X" : "M";
  const char* out_name = kEncode ? "Y" : "C";
  Extent ext;
  if (const int rc = rect_sizes(fn, batch, rows, cols, ld, batch_stride, Rk, S, gr, gc, part, kEncode ? 1 : 2, shift, eb,
                                &ext))
    return rc;
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
  if (ranges_overlap(tokens, static_cast<int64_t>(Rk) * 3 * S, out, out_bytes))
    return tg_internal_fail(TG_ERR_INVALID, "%s: tokens and %s overlap", fn, out_name);
  const int64_t h = rows / gr, w = cols / gc;
  const void* strided = kEncode ? static_cast<const void*>(in) : out;
  const void* dense = kEncode ? static_cast<const void*>(out) : in;
  const int live = gr * gc;
  const int pack_bytes = live <= R::kWidePacksUpTo ? 16 : 8;
  const bool packs = packs_of(pack_bytes, strided, dense, batch, ld, batch_stride, w, eb);
  const int V = packs ? pack_bytes / eb : 1;
  R::Args a{in, out, tokens, h, w, ld, batch > 1 ? batch_stride : 0, batch * h * (w / V), Rk, S, shift, part, live, {}};
  for (int e = 0; e < live; ++e) a.at[e] = (e / gc) * h * ld + (e % gc) * w;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return launch_bucket<E, kEncode>(fn, packs, a, st);
}

}  // namespace

extern "C" int tg_reset_matmul_rect_i8(int8_t* state_out, int64_t B, int n, int m, int p, int S, int64_t game_stride_bytes,
                                       tg_stream_t stream) {
  const char* fn = "tg_reset_matmul_rect_i8";
  if (n < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: n=%d < 1", fn, n);
  if (m < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: m=%d < 1", fn, m);
  if (p < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: p=%d < 1", fn, p);
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  const int64_t nm = static_cast<int64_t>(n) * m, mp = static_cast<int64_t>(m) * p, np = static_cast<int64_t>(n) * p;
  if (nm > S) return tg_internal_fail(TG_ERR_INVALID, "%s: n*m=%lld above S=%d", fn, (long long)nm, S);
  if (mp > S) return tg_internal_fail(TG_ERR_INVALID, "%s: m*p=%lld above S=%d", fn, (long long)mp, S);
  if (np > S) return tg_internal_fail(TG_ERR_INVALID, "%s: n*p=%lld above S=%d", fn, (long long)np, S);
  if (int rc = check_state(fn, B, S, game_stride_bytes)) return rc;
  if (B > INT64_MAX / game_stride_bytes) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld out of range", fn, (long long)B);
  if (B == 0) return TG_OK;
  if (!state_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null state_out", fn);
  const int64_t total = B * S * S * S;
  const R::ResetArgs a{state_out, B, game_stride_bytes, n, m, p, S};
  return launch(fn, R::reset_kernel, grid_for((total + R::kBlock - 1) / R::kBlock, 8192), R::kBlock, 0,
                static_cast<hipStream_t>(stream), a);
}

extern "C" int tg_bilinear_rect_check(int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int Rk,
                                      int S, int gr, int gc, int part, int shift, int elem_bytes) {
  return rect_sizes("tg_bilinear_rect_check", batch, rows, cols, ld, batch_stride, Rk, S, gr, gc, part, 2, shift,
                    elem_bytes);
}

extern "C" int tg_bilinear_rect_encode_f32(const float* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                           int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc,
                                           int part, int shift, float* Y, tg_stream_t stream) {
  return rect_entry<float, true>("tg_bilinear_rect_encode_f32", X, Y, batch, rows, cols, ld, batch_stride, tokens, Rk, S,
                                 gr, gc, part, shift, stream);
}

extern "C" int tg_bilinear_rect_encode_f64(const double* X, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                           int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc,
                                           int part, int shift, double* Y, tg_stream_t stream) {
  return rect_entry<double, true>("tg_bilinear_rect_encode_f64", X, Y, batch, rows, cols, ld, batch_stride, tokens, Rk, S,
                                  gr, gc, part, shift, stream);
}

extern "C" int tg_bilinear_rect_decode_f32(const float* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                           int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc,
                                           int shift, float* C, tg_stream_t stream) {
  return rect_entry<float, false>("tg_bilinear_rect_decode_f32", M, C, batch, rows, cols, ld, batch_stride, tokens, Rk, S,
                                  gr, gc, 2, shift, stream);
}

extern "C" int tg_bilinear_rect_decode_f64(const double* M, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                                           int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc,
                                           int shift, double* C, tg_stream_t stream) {
  return rect_entry<double, false>("tg_bilinear_rect_decode_f64", M, C, batch, rows, cols, ld, batch_stride, tokens, Rk,
                                   S, gr, gc, 2, shift, stream);
}
