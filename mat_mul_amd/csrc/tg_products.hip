// tg_products.hip -- include/tensor_game_products.h: the R block products of a bilinear algorithm on bfloat16 / float16
// operands, the block combinations formed while the product loads its tiles.
//
//   M[b][r] = Ahat_r * Bhat_r,   Ahat_r = rn_H(sum_e u_r[e] * (block e of A_b)),   Bhat_r = rn_H(sum_e v_r[e] * (block e of B_b))
//
// One workgroup of 256 threads owns one TM x TM tile of one M[b][r] at a time (TM = 64, or 128 where both h and w are
// above 64) and takes tiles by a grid-stride loop; r is the innermost digit of the tile number, so workgroups that run
// together read the same blocks of A and B.  Per step of 32 in k:
//   1. a thread owns packs of 8 consecutive elements of a row of the A tile (8 k) and of the B tile (8 x).  For every
//      block with a non-zero coefficient it loads the pack (one 16-byte load, or 8 elements where the operand's
//      addresses do not allow it: the host decides per operand) and accumulates in float32 by the header's rule 2.  The
//      coefficient rows are those of tg_bilinear_body.h: an image in LDS, a row in SGPRs, the zero test a scalar branch, a
//      block behind the grid reading as coefficient zero.  A pack outside the block (the tails in h, w and q) is not
//      loaded and is zero;
//   2. the sums are rounded to H by the hardware's round-to-nearest-even conversion and stored to LDS, A as [y][k], B
//      transposed as [x][k], so that both MFMA fragments (8 consecutive k of a row / of a column) are one 16-byte read;
//   3. after a barrier each of the four wavefronts multiplies its quarter of the tile with v_mfma_f32_32x32x16_{bf16,f16}.
// The results leave from the accumulators by plain stores: a lane holds a column, so 32 lanes write 128 consecutive bytes.
#include "../../include/tensor_game_products.h"
#include "tg_bilinear_body.h"

#pragma clang fp contract(off)

namespace tg {
namespace products {

constexpr int kBlock = 256;
constexpr int kSlots = TG_MAX_S;   // blocks of a grid at most
constexpr int kStep = 32;          // k per step: two MFMAs deep
constexpr int kPitch = kStep + 8;  // elements of an LDS row: 80 bytes, so every fragment is 16-byte aligned

struct Args {
  const uint16_t* A;
  const uint16_t* B;
  const int8_t* tokens;
  float* M;
  int64_t h, q, w;  // the blocks: A's are h x q, B's q x w, M's h x w
  int64_t lda, stride_a, ldb, stride_b;
  int64_t tiles_y, tiles_x, tiles;  // tiles = batch * tiles_y * tiles_x * R
  int R, S, shift;
  int live_a, live_b;  // n * m, m * p: the blocks of A's grid and of B's
  int cols_a, cols_b;  // m, p: the columns of the two grids
};

// what Coefficients (tg_bilinear_body.h) wants of a grid: the image of part PART, `shift` behind the grid's blocks
template <int PART>
struct Part {
  using Args = products::Args;
  static constexpr int kSlots = products::kSlots;
  __device__ static int8_t image(const Args& a, int r, int e) {
    return e < (PART ? a.live_b : a.live_a) ? a.tokens[static_cast<int64_t>(r) * 3 * a.S + PART * a.S + e]
                                            : static_cast<int8_t>(a.shift);
  }
};

using Acc = __attribute__((ext_vector_type(16))) float;

struct Bf16 {
  using Frag = __attribute__((ext_vector_type(8))) __bf16;
  __device__ static float widen(uint16_t v) { return __uint_as_float(static_cast<uint32_t>(v) << 16); }
  __device__ static uint16_t narrow(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
  __device__ static Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

struct F16 {
  using Frag = __attribute__((ext_vector_type(8))) _Float16;
  __device__ static float widen(uint16_t v) { return static_cast<float>(__builtin_bit_cast(_Float16, v)); }
  __device__ static uint16_t narrow(float f) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f)); }
  __device__ static Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

using Raw = bilinear::Pack<uint16_t, 8>;  // 8 elements of H, 16 bytes

// the first `count` (0 .. 8) elements at p, zeros behind them; a 16-byte load where the host found every pack aligned
// and whole (count is then 0 or 8)
template <bool VEC>
__device__ inline Raw load_raw(const uint16_t* p, int count) {
  Raw x;
  if constexpr (VEC) {
    x = Raw{};
    if (count == 8) x = *reinterpret_cast<const Raw*>(p);
  } else {
#pragma unroll
    for (int v = 0; v < 8; ++v) x.v[v] = v < count ? p[v] : uint16_t{0};
  }
  return x;
}

__device__ inline int64_t uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
  return static_cast<int64_t>(static_cast<uint64_t>(hi) << 32 | lo);
}

// out[i] = rn_H of the block combination of pack i (rule 2 of the header) by row r of `image`: pack i is `count[i]`
// elements at base + at[e] + off[i] of every block e.  Loads of a few blocks are issued together, then their terms are
// added in ascending e.  The row and the blocks' offsets are read from LDS here, at every step in k, on purpose: read
// once per tile they are loop invariants, and the compiler then carries every slot's zero test, its coefficient as a
// float and its address across the loop in VGPRs (several hundred of them, seen as scratch).
template <typename H, bool VEC, int NP, typename Co>
__device__ inline void combine(const int* image, int r, int shift, const int64_t* at, int live, const uint16_t* base,
                               const int64_t (&off)[NP], const int (&count)[NP], Raw (&out)[NP]) {
  constexpr int kAhead = 8 / NP;
  Co co;
  co.load(image, r);
  float acc[NP][8];
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[i][v] = 0.0f;
#pragma unroll
  for (int e0 = 0; e0 < kSlots; e0 += kAhead) {
    if (e0 < live) {  // wave-uniform
      Raw xs[kAhead][NP];
#pragma unroll
      for (int j = 0; j < kAhead; ++j)
        if (co.at(e0 + j, shift) != 0) {
          const int64_t block = uniform(at[e0 + j]);
#pragma unroll
          for (int i = 0; i < NP; ++i) xs[j][i] = load_raw<VEC>(base + off[i] + block, count[i]);
        }
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        const int c = co.at(e0 + j, shift);  // zero where the slot is no block of the grid
        if (c != 0) {
          const float cf = static_cast<float>(c);
#pragma unroll
          for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int v = 0; v < 8; ++v)
              acc[i][v] = bilinear::add_rn(acc[i][v], bilinear::mul_rn(cf, H::widen(xs[j][i].v[v])));
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int v = 0; v < 8; ++v) out[i].v[v] = v < count[i] ? H::narrow(acc[i][v]) : uint16_t{0};
}

__device__ inline int clamp8(int64_t v) { return v < 0 ? 0 : (v > 8 ? 8 : static_cast<int>(v)); }

template <typename H, int SUB, bool VA, bool VB>
__global__ __launch_bounds__(kBlock, 2) void products_kernel(const Args a) {
  constexpr int TM = 64 * SUB;  // rows and columns of a tile; a wavefront owns SUB x SUB squares of 32 x 32
  using CoA = bilinear::Coefficients<Part<0>>;
  using CoB = bilinear::Coefficients<Part<1>>;
  using Frag = typename H::Frag;
  __shared__ int image_a[TG_SOL_MAX_K * CoA::kWords];
  __shared__ int image_b[TG_SOL_MAX_K * CoB::kWords];
  __shared__ __attribute__((aligned(16))) uint16_t As[TM * kPitch];  // [y][k]
  __shared__ __attribute__((aligned(16))) uint16_t Bs[TM * kPitch];  // [x][k]
  __shared__ int64_t at_a[kSlots], at_b[kSlots];  // where block e starts inside a matrix, in elements
  if (threadIdx.x < a.live_a) at_a[threadIdx.x] = (threadIdx.x / a.cols_a) * a.h * a.lda + (threadIdx.x % a.cols_a) * a.q;
  if (threadIdx.x < a.live_b) at_b[threadIdx.x] = (threadIdx.x / a.cols_b) * a.q * a.ldb + (threadIdx.x % a.cols_b) * a.w;
  CoA::stage(image_a, a);
  CoB::stage(image_b, a);  // ends with a barrier
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, col = lane & 31, half = lane >> 5;
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    int64_t rest, r64, pos, tx, b, ty;
    bilinear::split(t, a.R, rest, r64);
    bilinear::split(rest, a.tiles_x, pos, tx);
    bilinear::split(pos, a.tiles_y, b, ty);
    const int r = static_cast<int>(r64);
    const int64_t y0 = ty * TM, x0 = tx * TM;
    const uint16_t* Ab = a.A + b * a.stride_a;
    const uint16_t* Bb = a.B + b * a.stride_b;
    Acc acc[SUB][SUB];
#pragma unroll
    for (int i = 0; i < SUB; ++i)
#pragma unroll
      for (int j = 0; j < SUB; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.0f;
    for (int64_t k0 = 0; k0 < a.q; k0 += kStep) {
      Raw pa[SUB], pb[SUB];
      {  // the A tile is TM rows of 4 packs
        int64_t off[SUB];
        int count[SUB];
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          const int pack = tid + kBlock * i;
          const int64_t y = y0 + (pack >> 2), k = k0 + 8 * (pack & 3);
          count[i] = y < a.h ? clamp8(a.q - k) : 0;
          off[i] = y * a.lda + k;
        }
        combine<H, VA, SUB, CoA>(image_a, r, a.shift, at_a, a.live_a, Ab, off, count, pa);
      }
      {  // the B tile is 32 rows (k) of TM / 8 packs
        int64_t off[SUB];
        int count[SUB];
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          const int pack = tid + kBlock * i;
          const int64_t k = k0 + pack / (TM / 8), x = x0 + 8 * (pack % (TM / 8));
          count[i] = k < a.q ? clamp8(a.w - x) : 0;
          off[i] = k * a.ldb + x;
        }
        combine<H, VB, SUB, CoB>(image_b, r, a.shift, at_b, a.live_b, Bb, off, count, pb);
      }
      __syncthreads();  // the fragments of the step before are read
#pragma unroll
      for (int i = 0; i < SUB; ++i) {
        const int pack = tid + kBlock * i;
        *reinterpret_cast<Raw*>(&As[(pack >> 2) * kPitch + 8 * (pack & 3)]) = pa[i];
        const int kl = pack / (TM / 8), xl = 8 * (pack % (TM / 8));
#pragma unroll
        for (int v = 0; v < 8; ++v) Bs[(xl + v) * kPitch + kl] = pb[i].v[v];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < kStep / 16; ++ks) {
        // lane (col, half) holds A[row col][k = 8 half + j] and B[k = 8 half + j][column col], j = 0 .. 7
        Frag fa[SUB], fb[SUB];
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          fa[i] = *reinterpret_cast<const Frag*>(&As[((wm * SUB + i) * 32 + col) * kPitch + 16 * ks + 8 * half]);
          fb[i] = *reinterpret_cast<const Frag*>(&Bs[((wn * SUB + i) * 32 + col) * kPitch + 16 * ks + 8 * half]);
        }
#pragma unroll
        for (int i = 0; i < SUB; ++i)
#pragma unroll
          for (int j = 0; j < SUB; ++j) acc[i][j] = H::mfma(fa[i], fb[j], acc[i][j]);
      }
    }
    // result g of a lane: row (g & 3) + 8 (g >> 2) + 4 half, column col of its square
    float* Mb = a.M + (b * a.R + r) * a.h * a.w;
#pragma unroll
    for (int i = 0; i < SUB; ++i)
#pragma unroll
      for (int j = 0; j < SUB; ++j) {
        const int64_t x = x0 + (wn * SUB + j) * 32 + col;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int64_t y = y0 + (wm * SUB + i) * 32 + (g & 3) + 8 * (g >> 2) + 4 * half;
          if (y < a.h && x < a.w) Mb[y * a.w + x] = acc[i][j][g];
        }
      }
  }
}

}  // namespace products
}  // namespace tg

namespace {

namespace B = tg::bilinear;
namespace P = tg::products;

struct Extents {
  int64_t a, b, m;  // elements from the first to one past the last of A, B and M
};

// ld, the batch stride and the span of one operand: `rows` x `cols`, called rows_name x cols_name
int operand_span(const char* fn, const char* name, const char* rows_name, const char* cols_name, int64_t batch,
                 int64_t rows, int64_t cols, int64_t ld, int64_t stride, int64_t* span) {
  if (ld < cols)
    return tg_internal_fail(TG_ERR_INVALID, "%s: ld%s=%lld < %s=%lld", fn, name, (long long)ld, cols_name, (long long)cols);
  int64_t one, matrix, bytes;
  *span = 0;
  bool fits = B::mul_fits(rows - 1, ld, &one) && B::add_fits(one, cols, &one) && B::mul_fits(rows, ld, &matrix);
  if (fits && batch > 1 && stride < matrix)
    return tg_internal_fail(TG_ERR_INVALID, "%s: stride_%s=%lld < %s*ld%s=%lld", fn, name, (long long)stride, rows_name,
                            name, (long long)matrix);
  if (fits && batch > 0)
    fits = B::mul_fits(batch - 1, batch > 1 ? stride : 0, span) && B::add_fits(*span, one, span) &&
           B::mul_fits(*span, 2, &bytes);
  if (!fits)
    return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld, %s=%lld, ld%s=%lld out of range: a byte offset leaves int64",
                            fn, (long long)batch, rows_name, (long long)rows, name, (long long)ld);
  return TG_OK;
}

int products_sizes(const char* fn, int64_t batch, int64_t Pr, int64_t Q, int64_t T, int64_t lda, int64_t stride_a,
                   int64_t ldb, int64_t stride_b, int R, int S, int n, int m, int p, int shift, Extents* ext = nullptr) {
  if (n < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: n=%d < 1", fn, n);
  if (m < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: m=%d < 1", fn, m);
  if (p < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: p=%d < 1", fn, p);
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  const int64_t nm = static_cast<int64_t>(n) * m, mp = static_cast<int64_t>(m) * p, np = static_cast<int64_t>(n) * p;
  if (nm > S) return tg_internal_fail(TG_ERR_INVALID, "%s: n*m=%lld above S=%d", fn, (long long)nm, S);
  if (mp > S) return tg_internal_fail(TG_ERR_INVALID, "%s: m*p=%lld above S=%d", fn, (long long)mp, S);
  if (np > S) return tg_internal_fail(TG_ERR_INVALID, "%s: n*p=%lld above S=%d", fn, (long long)np, S);
  if (const int rc = B::check_rank_shift(fn, R, shift)) return rc;
  if (batch < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld < 0", fn, (long long)batch);
  if (Pr < n || Pr % n)
    return tg_internal_fail(TG_ERR_INVALID, "%s: P=%lld is no positive multiple of n=%d", fn, (long long)Pr, n);
  if (Q < m || Q % m)
    return tg_internal_fail(TG_ERR_INVALID, "%s: Q=%lld is no positive multiple of m=%d", fn, (long long)Q, m);
  if (T < p || T % p)
    return tg_internal_fail(TG_ERR_INVALID, "%s: T=%lld is no positive multiple of p=%d", fn, (long long)T, p);
  Extents e{};
  if (const int rc = operand_span(fn, "a", "P", "Q", batch, Pr, Q, lda, stride_a, &e.a)) return rc;
  if (const int rc = operand_span(fn, "b", "Q", "T", batch, Q, T, ldb, stride_b, &e.b)) return rc;
  int64_t bytes;
  if (!(B::mul_fits(batch, R, &e.m) && B::mul_fits(e.m, Pr / n, &e.m) && B::mul_fits(e.m, T / p, &e.m) &&
        B::mul_fits(e.m, 4, &bytes)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: batch=%lld, R=%d, P=%lld, T=%lld out of range: a byte offset of M leaves "
                            "int64", fn, (long long)batch, R, (long long)Pr, (long long)T);
  if (ext) *ext = e;
  return TG_OK;
}

// 16-byte loads for an operand: the header's load path
bool wide_loads(const void* ptr, int64_t batch, int64_t ld, int64_t stride, int64_t width) {
  return aligned(ptr, 16) && ld % 8 == 0 && (batch <= 1 || stride % 8 == 0) && width % 8 == 0;
}

template <typename H, int SUB>
int launch_loads(const char* fn, bool va, bool vb, const P::Args& a, unsigned grid, hipStream_t st) {
  if (va && vb) return launch(fn, P::products_kernel<H, SUB, true, true>, grid, P::kBlock, 0, st, a);
  if (va) return launch(fn, P::products_kernel<H, SUB, true, false>, grid, P::kBlock, 0, st, a);
  if (vb) return launch(fn, P::products_kernel<H, SUB, false, true>, grid, P::kBlock, 0, st, a);
  return launch(fn, P::products_kernel<H, SUB, false, false>, grid, P::kBlock, 0, st, a);
}

template <typename H>
int products_entry(const char* fn, const uint16_t* A, const uint16_t* Bm, int64_t batch, int64_t Pr, int64_t Q, int64_t T,
                   int64_t lda, int64_t stride_a, int64_t ldb, int64_t stride_b, const int8_t* tokens, int R, int S, int n,
                   int m, int p, int shift, float* M, tg_stream_t stream) {
  Extents ext;
  if (const int rc = products_sizes(fn, batch, Pr, Q, T, lda, stride_a, ldb, stride_b, R, S, n, m, p, shift, &ext)) return rc;
  if (batch == 0) return TG_OK;
  if (!A) return tg_internal_fail(TG_ERR_INVALID, "%s: null A", fn);
  if (!Bm) return tg_internal_fail(TG_ERR_INVALID, "%s: null B", fn);
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!M) return tg_internal_fail(TG_ERR_INVALID, "%s: null M", fn);
  if (!aligned(A, 2)) return tg_internal_fail(TG_ERR_INVALID, "%s: A not 2-byte aligned", fn);
  if (!aligned(Bm, 2)) return tg_internal_fail(TG_ERR_INVALID, "%s: B not 2-byte aligned", fn);
  if (!aligned(M, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: M not 4-byte aligned", fn);
  if (B::ranges_overlap(A, ext.a * 2, M, ext.m * 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: A and M overlap: in-place operation is not supported", fn);
  if (B::ranges_overlap(Bm, ext.b * 2, M, ext.m * 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: B and M overlap: in-place operation is not supported", fn);
  if (B::ranges_overlap(tokens, static_cast<int64_t>(R) * 3 * S, M, ext.m * 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: tokens and M overlap", fn);
  const int64_t h = Pr / n, q = Q / m, w = T / p;
  const bool big = h > 64 && w > 64;
  const int64_t tm = big ? 128 : 64;
  P::Args a{};
  a.A = A, a.B = Bm, a.tokens = tokens, a.M = M;
  a.h = h, a.q = q, a.w = w;
  a.lda = lda, a.stride_a = batch > 1 ? stride_a : 0, a.ldb = ldb, a.stride_b = batch > 1 ? stride_b : 0;
  a.tiles_y = (h + tm - 1) / tm, a.tiles_x = (w + tm - 1) / tm;
  a.tiles = ext.m / (h * w) * a.tiles_y * a.tiles_x;  // below batch * R * h * w, which fits
  a.R = R, a.S = S, a.shift = shift;
  a.live_a = n * m, a.live_b = m * p, a.cols_a = m, a.cols_b = p;
  const bool va = wide_loads(A, batch, lda, stride_a, q), vb = wide_loads(Bm, batch, ldb, stride_b, w);
  const unsigned grid = grid_for(a.tiles, static_cast<int64_t>(8) * device_cu_count());  // the loop takes the rest
  const hipStream_t st = static_cast<hipStream_t>(stream);
  return big ? launch_loads<H, 2>(fn, va, vb, a, grid, st) : launch_loads<H, 1>(fn, va, vb, a, grid, st);
}

}  // namespace

extern "C" int tg_bilinear_products_check(int64_t batch, int64_t Pr, int64_t Q, int64_t T, int64_t lda, int64_t stride_a,
                                          int64_t ldb, int64_t stride_b, int R, int S, int n, int m, int p, int shift) {
  return products_sizes("tg_bilinear_products_check", batch, Pr, Q, T, lda, stride_a, ldb, stride_b, R, S, n, m, p, shift);
}

extern "C" int tg_bilinear_products_bf16(const uint16_t* A, const uint16_t* Bm, int64_t batch, int64_t Pr, int64_t Q,
                                         int64_t T, int64_t lda, int64_t stride_a, int64_t ldb, int64_t stride_b,
                                         const int8_t* tokens, int R, int S, int n, int m, int p, int shift, float* M,
                                         tg_stream_t stream) {
  return products_entry<P::Bf16>("tg_bilinear_products_bf16", A, Bm, batch, Pr, Q, T, lda, stride_a, ldb, stride_b, tokens,
                                 R, S, n, m, p, shift, M, stream);
}

extern "C" int tg_bilinear_products_f16(const uint16_t* A, const uint16_t* Bm, int64_t batch, int64_t Pr, int64_t Q,
                                        int64_t T, int64_t lda, int64_t stride_a, int64_t ldb, int64_t stride_b,
                                        const int8_t* tokens, int R, int S, int n, int m, int p, int shift, float* M,
                                        tg_stream_t stream) {
  return products_entry<P::F16>("tg_bilinear_products_f16", A, Bm, batch, Pr, Q, T, lda, stride_a, ldb, stride_b, tokens, R,
                                S, n, m, p, shift, M, stream);
}
