// tg_bilinear.hip -- include/tensor_game_bilinear.h: the two linear halves of a bilinear matrix-multiplication algorithm
// on the n x n grid of blocks.
//
// encode: Y[b][r] = sum_a c_r[mode][a] * (block a of X_b);   decode: (block c of C_b) = sum_r c_r[2][c] * M[b][r].
//
// The kernels and the host path are those of tg_bilinear_body.h; this file holds the square grid (n is a template
// parameter, so every one of the S = n^2 slots is live and a block's offset is two multiplications), the entries' own
// checks and the dispatch on n.  A pack is 16 bytes (float4 / double2) where the host found every address of the call
// 16-byte aligned, one element otherwise.  The arithmetic rule of the header holds under the pragma below as in the body.
#include "../../include/tensor_game_bilinear.h"
#include "tg_bilinear_body.h"

#pragma clang fp contract(off)

namespace tg {

struct BilinearArgs {
  const void* in;
  void* out;
  const int8_t* tokens;
  // of the strided operand (encode's input, decode's output), in elements; the dense one is (batch,R,h,w)
  int64_t h, w, ld, batch_stride;
  int64_t items;  // batch * h * (w / V)
  int R, shift, part;
};

template <int N>
struct SquareGrid {
  using Args = BilinearArgs;
  static constexpr int kSlots = N * N;
  __device__ static bool live(const Args&, int) { return true; }
  __device__ static int64_t pitch(const Args& a) { return a.h * a.ld; }  // from one row of blocks to the next
  template <typename T>
  __device__ static T* block(const Args& a, int64_t pitch, T* p, int e) {
    return p + (e / N) * pitch + (e % N) * a.w;
  }
  // zero behind the S entries: never read as a coefficient
  __device__ static int8_t image(const Args& a, int r, int e) {
    return e < kSlots ? a.tokens[r * 3 * kSlots + a.part * kSlots + e] : int8_t{0};
  }
};

}  // namespace tg

namespace {

namespace B = tg::bilinear;

int bilinear_sizes(const char* fn, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t batch_stride, int R,
                   int n, int mode, int shift, int elem_bytes, B::Extent* ext = nullptr) {
  if (n < TG_BILINEAR_MIN_N || n > TG_BILINEAR_MAX_N)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n=%d outside [%d,%d]", fn, n, TG_BILINEAR_MIN_N, TG_BILINEAR_MAX_N);
  if (const int rc = B::check_rank_shift(fn, R, shift)) return rc;
  if (mode != 0 && mode != 1) return tg_internal_fail(TG_ERR_INVALID, "%s: mode=%d is neither 0 nor 1", fn, mode);
  return B::check_sizes(fn, batch, rows, cols, ld, batch_stride, R, n, "n", n, "n", elem_bytes, ext);
}

template <typename E, bool kEncode, int V>
int launch_bilinear_n(const char* fn, int n, const tg::BilinearArgs& a, hipStream_t st) {
  switch (n) {
    case 2: return B::launch_kernel<E, kEncode, tg::SquareGrid<2>, V>(fn, a, st);
    case 3: return B::launch_kernel<E, kEncode, tg::SquareGrid<3>, V>(fn, a, st);
    case 4: return B::launch_kernel<E, kEncode, tg::SquareGrid<4>, V>(fn, a, st);
    default: return B::launch_kernel<E, kEncode, tg::SquareGrid<5>, V>(fn, a, st);
  }
}

template <typename E, bool kEncode>
int bilinear_entry(const char* fn, const E* in, E* out, int64_t batch, int64_t rows, int64_t cols, int64_t ld,
                   int64_t batch_stride, const int8_t* tokens, int R, int n, int mode, int shift, tg_stream_t stream) {
  B::Extent ext;
  if (const int rc = bilinear_sizes(fn, batch, rows, cols, ld, batch_stride, R, n, mode, shift, sizeof(E), &ext)) return rc;
  return B::entry<E, kEncode>(
      fn, in, out, batch, rows, cols, ld, batch_stride, tokens, static_cast<int64_t>(R) * 3 * n * n, n, n, 16, ext,
      [&](int V, int64_t h, int64_t w, int64_t stride, int64_t items) {
        const tg::BilinearArgs a{in, out, tokens, h, w, ld, stride, items, R, shift, kEncode ? mode : 2};
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (V > 1) return launch_bilinear_n<E, kEncode, 16 / sizeof(E)>(fn, n, a, st);
        return launch_bilinear_n<E, kEncode, 1>(fn, n, a, st);
      });
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
