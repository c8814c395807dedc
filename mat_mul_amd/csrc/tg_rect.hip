// tg_rect.hip -- include/tensor_game_rect.h: the rectangular target <n,m,p> and the two linear halves of a bilinear
// algorithm on a gr x gc grid of blocks.
//
// encode: Y[b][r] = sum_e c_r[part][e] * (block e of X_b);   decode: (block e of C_b) = sum_r c_r[2][e] * M[b][r].
//
// The kernels and the host path are those of tg_bilinear_body.h; this file holds the grid taken at run time, the entries'
// own checks and the dispatch on the block count.  There are about a hundred legal grids, so the kernels are not
// instantiated per grid: the policy's parameter is a bucket of the block count (4, 9, 16, 25, 32: the squares and
// TG_MAX_S), the arrays of packs have the bucket's size and are indexed by unrolled constants alone (registers, no
// scratch), and the live count gr*gc and the blocks' element offsets (computed once on the host, read from the kernel
// arguments) are wave-uniform.  A block at or beyond the live count is neither loaded nor stored, and its coefficient
// reads as zero: the image of a row in LDS holds `shift` there, so the zero test that skips a term skips it too.  The
// arithmetic rule of the header holds under the pragma below as in the body.
#include "../../include/tensor_game_rect.h"
#include "tg_bilinear_body.h"

#pragma clang fp contract(off)

namespace tg {
namespace rect {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = TG_MAX_S;  // of a grid: gr * gc <= S <= TG_MAX_S
constexpr int kWidePacksUpTo = 25;    // the header's dispatch rule: packs of 16 bytes up to here, of 8 bytes above

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

// MINB: the smallest live count the host sends to this bucket; blocks below it are live without a test
template <int MINB, int MAXB>
struct RunTimeGrid {
  using Args = rect::Args;
  static constexpr int kSlots = MAXB;
  __device__ static bool live(const Args& a, int e) { return e < MINB || e < a.live; }
  __device__ static int64_t pitch(const Args&) { return 0; }  // at[] holds whole offsets
  template <typename T>
  __device__ static T* block(const Args& a, int64_t, T* p, int e) {
    return p + a.at[e];
  }
  // `shift` (a zero coefficient) behind the live entries
  __device__ static int8_t image(const Args& a, int r, int e) {
    return e < a.live ? a.tokens[r * 3 * a.S + a.part * a.S + e] : static_cast<int8_t>(a.shift);
  }
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

}  // namespace rect
}  // namespace tg

namespace {

namespace B = tg::bilinear;
namespace R = tg::rect;

int rect_sizes(const char* fn, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int Rk, int S,
               int gr, int gc, int part, int max_part, int shift, int elem_bytes, B::Extent* ext = nullptr) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (gr < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: gr=%d < 1", fn, gr);
  if (gc < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: gc=%d < 1", fn, gc);
  if (gr > S || gc > S || gr * gc > S)
    return tg_internal_fail(TG_ERR_INVALID, "%s: gr*gc=%lld above S=%d", fn, (long long)gr * gc, S);
  if (const int rc = B::check_rank_shift(fn, Rk, shift)) return rc;
  if (part < 0 || part > max_part) return tg_internal_fail(TG_ERR_INVALID, "%s: part=%d outside [0,%d]", fn, part, max_part);
  return B::check_sizes(fn, batch, rows, cols, ld, batch_stride, Rk, gr, "gr", gc, "gc", elem_bytes, ext);
}

// the bucket of the live count, for packs of V elements where the bucket's pack rule allows them (else single elements)
template <typename E, bool kEncode>
int launch_bucket(const char* fn, bool packs, const R::Args& a, hipStream_t st) {
  constexpr int V16 = 16 / sizeof(E), V8 = 8 / sizeof(E);
#define TG_RECT_BUCKET(lo, hi, V)                                                                \
  if (a.live <= hi)                                                                              \
    return packs && V > 1 ? B::launch_kernel<E, kEncode, R::RunTimeGrid<lo, hi>, V>(fn, a, st)   \
                          : B::launch_kernel<E, kEncode, R::RunTimeGrid<lo, hi>, 1>(fn, a, st)
  TG_RECT_BUCKET(1, 4, V16);
  TG_RECT_BUCKET(5, 9, V16);
  TG_RECT_BUCKET(10, 16, V16);
  TG_RECT_BUCKET(17, R::kWidePacksUpTo, V16);
  TG_RECT_BUCKET(R::kWidePacksUpTo + 1, R::kMaxBlocks, V8);
#undef TG_RECT_BUCKET
  return tg_internal_fail(TG_ERR_INVALID, "%s: gr*gc=%d above %d", fn, a.live, R::kMaxBlocks);
}

template <typename E, bool kEncode>
int rect_entry(const char* fn, const E* in, E* out, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
               int64_t batch_stride, const int8_t* tokens, int Rk, int S, int gr, int gc, int part, int shift,
               tg_stream_t stream) {
  B::Extent ext;
  if (const int rc = rect_sizes(fn, batch, rows, cols, ld, batch_stride, Rk, S, gr, gc, part, kEncode ? 1 : 2, shift,
                                sizeof(E), &ext))
    return rc;
  const int live = gr * gc;
  return B::entry<E, kEncode>(
      fn, in, out, batch, rows, cols, ld, batch_stride, tokens, static_cast<int64_t>(Rk) * 3 * S, gr, gc,
      live <= R::kWidePacksUpTo ? 16 : 8, ext, [&](int V, int64_t h, int64_t w, int64_t stride, int64_t items) {
        R::Args a{in, out, tokens, h, w, ld, stride, items, Rk, S, shift, part, live, {}};
        for (int e = 0; e < live; ++e) a.at[e] = (e / gc) * h * ld + (e % gc) * w;
        return launch_bucket<E, kEncode>(fn, V > 1, a, static_cast<hipStream_t>(stream));
      });
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
