// The way back from a changed basis (include/tensor_game_bases.h): the exact inverse of a sampled basis and the
// application of a matrix triple to the factors of an action list.  gfx950 only; part of libtensorgame.so.
//
// basis_inverse_kernel   a workgroup of three wavefronts per triple, wavefront x = mode x, lane c = column c of both
//              substitutions (columns are independent: a lane only ever reads back what it wrote itself).  X = L^-1 and
//              Y = U^-1 go to LDS as int32 (an accepted entry is below 2^28), zeros of their empty triangles included;
//              after a barrier lane c forms column c of Y * X in int64: Y[r][k] is one address for the wavefront, X[k][c]
//              is stride 1.  The product waits in LDS until the workgroup has ORed its flags, because one bad matrix
//              zeroes all three; then each wavefront stores its own matrix, row-major and coalesced.
// solution_rebase_kernel   a wavefront per list.  The L * 3S token bytes and the row's three matrices are staged into LDS
//              once (matrix rows an odd number of words apart: the lanes of one term read 3S different rows at the same
//              column); lane p owns output byte p of the list: row p mod 3S of the staged triple times the S factor
//              values of its mode, in int64.  The bytes go into a zeroed LDS image of the output row; the range flag is
//              ORed across the wavefront BEFORE the image (or zeros) leaves, 16 bytes at a time where the row is aligned.
// Every output is a function of its own triple / row; the one atomic is the OR of the sticky bits into *status.  No
// floating point.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_bases.h"
#include "tg_lists.h"
#include "tg_sol_copy.h"

namespace tg {

constexpr int kInvThreads = 3 * 64;        // a wavefront per mode
constexpr int kInvPitch = TG_MAX_S;        // words per LDS row of a matrix
constexpr int64_t kInvLimit = 1ll << 28;   // an entry of L^-1 or U^-1 is accepted below this magnitude
constexpr int kRebaseThreads = 64;

struct InvArgs {
  const int8_t* lower;  // (N, 3, S, S)
  const int8_t* upper;
  int64_t N;
  int32_t* inv;         // (N, 3, S, S)
  uint8_t* bad;         // (N) or null
  uint32_t* status;     // or null
  int S;
};

// d * acc for a diagonal entry d = +-1 (the division by it), checked against the accepted range
__device__ __forceinline__ int32_t inv_entry(int64_t acc, int d, int& flags) {
  if (d != 1 && d != -1) {
    flags |= TG_BASIS_BAD_DIAGONAL;
    return 0;
  }
  acc *= d;
  if (acc >= kInvLimit || acc <= -kInvLimit) {  // replaced by 0: what follows stays exact in int64 and is discarded
    flags |= TG_BASIS_BAD_RANGE;
    return 0;
  }
  return static_cast<int32_t>(acc);
}

__global__ __launch_bounds__(kInvThreads) void basis_inverse_kernel(InvArgs a) {
  __shared__ int32_t mats[3][3][TG_MAX_S * kInvPitch];  // per mode: X = L^-1, Y = U^-1, Y * X
  const int x = threadIdx.x >> 6, c = threadIdx.x & 63, S = a.S, SS = S * S;
  int32_t* const X = mats[x][0];
  int32_t* const Y = mats[x][1];
  int32_t* const O = mats[x][2];

  for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
    const int8_t* L = a.lower + (n * 3 + x) * SS;
    const int8_t* U = a.upper + (n * 3 + x) * SS;
    int flags = 0;
    if (c < S) {
      // forward: column c of X, rows c .. S-1; only the diagonal and the strictly lower triangle of L are read
      for (int r = 0; r < c; ++r) X[r * kInvPitch + c] = 0;
      for (int r = c; r < S; ++r) {
        int64_t acc = r == c;
        for (int k = c; k < r; ++k) acc -= static_cast<int64_t>(L[r * S + k]) * X[k * kInvPitch + c];
        X[r * kInvPitch + c] = inv_entry(acc, L[r * S + r], flags);
      }
      // backward: column c of Y, rows c .. 0; only the diagonal and the strictly upper triangle of U are read
      for (int r = c + 1; r < S; ++r) Y[r * kInvPitch + c] = 0;
      for (int r = c; r >= 0; --r) {
        int64_t acc = r == c;
        for (int k = r + 1; k <= c; ++k) acc -= static_cast<int64_t>(U[r * S + k]) * Y[k * kInvPitch + c];
        Y[r * kInvPitch + c] = inv_entry(acc, U[r * S + r], flags);
      }
    }
    __syncthreads();  // X and Y are complete
    if (c < S) {
      for (int r = 0; r < S; ++r) {
        int64_t acc = 0;
        for (int k = 0; k < S; ++k) acc += static_cast<int64_t>(Y[r * kInvPitch + k]) * X[k * kInvPitch + c];
        if (acc != static_cast<int32_t>(acc)) {
          flags |= TG_BASIS_BAD_RANGE;
          acc = 0;
        }
        O[r * kInvPitch + c] = static_cast<int32_t>(acc);
      }
    }
    // (the OR of a predicate, not of the bits; also: the products are complete)
    const bool diagonal = __syncthreads_or(flags & TG_BASIS_BAD_DIAGONAL);
    const bool any = __syncthreads_or(flags);
    int32_t* out = a.inv + (n * 3 + x) * SS;
    for (int e = c; e < SS; e += 64) out[e] = any ? 0 : O[(e / S) * kInvPitch + e % S];
    if (threadIdx.x == 0) {
      if (a.bad) a.bad[n] = any;
      if (any && a.status)  // the range of a triple with a bad diagonal is not looked at
        atomicOr(a.status, static_cast<uint32_t>(diagonal ? TG_BASIS_BAD_DIAGONAL : TG_BASIS_BAD_RANGE));
    }
    __syncthreads();  // the matrices are free for the next triple
  }
}

struct RebaseArgs {
  const int8_t* tokens;    // (M, K, 3S)
  const int64_t* lengths;  // (M)
  const int32_t* mats;     // (G, 3, S, S)
  const int64_t* index;    // (M) or null
  int64_t M, G;
  int8_t* out;             // (M, K, 3S)
  int64_t* lengths_out;    // (M)
  uint8_t* bad;            // (M) or null
  uint32_t* status;        // or null
  int K, S, shift;
  int img;                 // bytes of one LDS image: K * 3S rounded up to 16
  int pitch;               // words per staged matrix row: S | 1
};

__global__ __launch_bounds__(kRebaseThreads) void solution_rebase_kernel(RebaseArgs a) {
  // two images of a.img bytes (the terms, the output row), then 3S matrix rows of a.pitch words
  extern __shared__ __attribute__((aligned(16))) uint8_t rebase_lds[];
  int8_t* const tok = reinterpret_cast<int8_t*>(rebase_lds);
  int8_t* const out = tok + a.img;
  int32_t* const mat = reinterpret_cast<int32_t*>(out + a.img);
  const int t = threadIdx.x, S = a.S, A3 = 3 * S, K = a.K, shift = a.shift, P = a.pitch;
  const int n_row = K * A3;

  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    // uniform, and checked before they address anything
    const int64_t L64 = a.lengths[m];
    const int64_t g = a.index ? a.index[m] : m;
    uint32_t bits = (L64 < 0 || L64 > K ? TG_REBASE_BAD_LENGTH : 0) | (g < 0 || g >= a.G ? TG_REBASE_BAD_INDEX : 0);
    if (!bits) {
      const int L = static_cast<int>(L64);
      sol_copy_in<kRebaseThreads>(a.tokens + m * n_row, tok, L * A3, t);
      const int32_t* src = a.mats + g * 3 * S * S;
      for (int e = t; e < A3 * S; e += kRebaseThreads) mat[(e / S) * P + e % S] = src[e];  // row x * S + a of the triple
      for (int q = t; q < a.img / 16; q += kRebaseThreads) reinterpret_cast<uint4*>(out)[q] = uint4{0, 0, 0, 0};
      __syncthreads();
      int over = 0;
      for (int p = t; p < L * A3; p += kRebaseThreads) {
        const int term = p / A3, e = p - term * A3;        // e = x * S + a: the matrix row, and the byte within the term
        const int8_t* f = tok + term * A3 + (e / S) * S;   // the factor of mode x
        const int32_t* row = mat + e * P;
        int64_t acc = shift;
        for (int b = 0; b < S; ++b) acc += static_cast<int64_t>(row[b]) * (f[b] - shift);
        over |= acc < -128 || acc > 127;
        out[p] = static_cast<int8_t>(acc);
      }
      if (__syncthreads_or(over)) bits = TG_REBASE_BAD_RANGE;  // (also: the image is complete)
    }
    sol_copy_out<kRebaseThreads>(a.out + m * n_row, bits ? nullptr : out, n_row, t);
    if (t == 0) {
      a.lengths_out[m] = bits ? 0 : L64;
      if (a.bad) a.bad[m] = bits != 0;
      if (bits && a.status) atomicOr(a.status, bits);
    }
    __syncthreads();  // the images and the matrices are free for the next list
  }
}

}  // namespace tg

namespace {

constexpr int64_t kTripleMax = 3ll * TG_MAX_S * TG_MAX_S * 4;  // bytes of one int32 triple at the largest S

int inverse_sizes(const char* fn, int64_t N, int S) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (N < 0 || N > INT64_MAX / kTripleMax) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)N);
  return TG_OK;
}

int rebase_sizes(const char* fn, int64_t M, int K, int S, int64_t G, int shift) {
  if (const int rc = check_lists(fn, K, S, shift, TG_SOL_MAX_K)) return rc;
  if (const int rc = check_list_count(fn, M)) return rc;
  if (G < 0 || G > INT64_MAX / kTripleMax || (G == 0 && M != 0))
    return tg_internal_fail(TG_ERR_INVALID, "%s: G=%lld out of range (G >= 1 unless M = 0)", fn, (long long)G);
  return TG_OK;
}

}  // namespace

extern "C" int tg_basis_inverse_check(int64_t N, int S) { return inverse_sizes("tg_basis_inverse_check", N, S); }

extern "C" int tg_solution_rebase_check(int64_t M, int K, int S, int64_t G, int shift) {
  return rebase_sizes("tg_solution_rebase_check", M, K, S, G, shift);
}

extern "C" int tg_basis_inverse_i32(const int8_t* lower, const int8_t* upper, int64_t N, int S, int32_t* inv_out,
                                    uint8_t* bad, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_basis_inverse_i32";
  if (const int rc = inverse_sizes(fn, N, S)) return rc;
  if (N == 0) return TG_OK;
  if (!lower) return tg_internal_fail(TG_ERR_INVALID, "%s: null lower", fn);
  if (!upper) return tg_internal_fail(TG_ERR_INVALID, "%s: null upper", fn);
  if (!inv_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null inv_out", fn);
  if (!aligned(inv_out, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: inv_out not 4-byte aligned", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const tg::InvArgs a{lower, upper, N, inv_out, bad, status, S};
  // 36 KiB of LDS per workgroup: four per CU
  return launch_resident(fn, tg::basis_inverse_kernel, N, 4, tg::kInvThreads, 0, static_cast<hipStream_t>(stream), a);
}

extern "C" int tg_solution_rebase(const int8_t* tokens, const int64_t* lengths, const int32_t* mats, const int64_t* index,
                                  int64_t M, int K, int S, int64_t G, int shift, int8_t* tokens_out, int64_t* lengths_out,
                                  uint8_t* bad, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_solution_rebase";
  if (const int rc = rebase_sizes(fn, M, K, S, G, shift)) return rc;
  if (M == 0) return TG_OK;
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!lengths) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths", fn);
  if (!mats) return tg_internal_fail(TG_ERR_INVALID, "%s: null mats", fn);
  if (!index && G != M)
    return tg_internal_fail(TG_ERR_INVALID, "%s: index is NULL (row m uses triple m), which needs G == M: G=%lld, M=%lld", fn,
                            (long long)G, (long long)M);
  if (!tokens_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens_out", fn);
  if (!lengths_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths_out", fn);
  if (tokens_out == tokens)
    return tg_internal_fail(TG_ERR_INVALID, "%s: tokens_out == tokens: in-place operation is not supported", fn);
  if (!aligned(lengths, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: lengths not 8-byte aligned", fn);
  if (!aligned(index, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: index not 8-byte aligned", fn);
  if (!aligned(lengths_out, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: lengths_out not 8-byte aligned", fn);
  if (!aligned(mats, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: mats not 4-byte aligned", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const int img = list_image_bytes(K, S);  // with 3S rows of S | 1 words the LDS stays below 64 KiB
  const int pitch = S | 1;
  const tg::RebaseArgs a{tokens, lengths, mats, index, M, G, tokens_out, lengths_out, bad, status, K, S, shift, img, pitch};
  return launch_resident(fn, tg::solution_rebase_kernel, M, 16, tg::kRebaseThreads,
                         2 * static_cast<size_t>(img) + static_cast<size_t>(3 * S) * pitch * 4, static_cast<hipStream_t>(stream), a);
}
