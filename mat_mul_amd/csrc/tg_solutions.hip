// Exact verification and the canonical form of a factorisation (include/tensor_game_solutions.h).  gfx950 only; part of
// libtensorgame.so.
//
// One kernel, one list per workgroup at a time: NT = 64 threads (a wavefront) while K <= 64, NT = 256 above, so thread t
// owns term t in the per-term phases.  The list's L * 3S token bytes are staged into LDS once and everything works there:
//   verify     the S^2 rows (i, j) of the residual are spread over the threads: a thread walks the L terms with
//              p = u_i * v_j and one multiply-add per l into int32 registers, the w tokens of a term read as 8-byte words
//              from a padded copy (32 bytes per term, the same address for the whole wavefront) and the shift taken
//              out of the loop: sum p * (w - shift) = sum p * w - shift * sum p;
//   normalise  one thread per factor (3L of them) finds the first non-zero value and negates the S bytes in place;
//   order      a rank sort: thread t compares its term with every other live term (8 bytes at a time, through a copy
//              whose unsigned word order is the signed lexicographic order; early exit at the first differing word) and counts the lower ones, the equal ones before it, and the run's sum of signs c.  Its place among
//              the live terms is lower + equal-before, it is kept iff equal-before < |c|, and its place in the output is
//              the number of kept terms at lower places (a flag per place, summed).  No loop count depends on the data
//              beyond the early exit, and there is no per-thread array indexed at run time;
//   emit       the kept terms go into a zeroed LDS image of the canon row, the key is summed over its 8-byte words and
//              the image leaves with 16-byte stores where the row is 16-byte aligned, byte stores otherwise.
// Every output word is a function of its own list; the one atomic is the OR of the sticky bad-row bits into *status,
// whose value does not depend on the order of the ORs.  No floating point.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_solutions.h"
#include "tg_host.h"
#include "tg_sol_copy.h"
#include "tg_sol_phases.h"

namespace tg {

struct SolArgs {
  const int8_t* targets;   // (M, S, S, S) or null
  const int8_t* tokens;    // (M, K, 3S)
  const int64_t* lengths;  // (M)
  int64_t M;
  int8_t* canon;           // (M, K, 3S)
  int32_t* rank;
  uint64_t* key;
  int32_t* residual;       // or null
  uint32_t* status;        // or null
  int K, S, shift;
  int img;                 // bytes of one LDS image: K * 3S rounded up to 16
};

// a bad row: zero canon row, rank 0, key 0, residual -1, the status bit
template <int NT>
__device__ __forceinline__ void sol_bad_row(const SolArgs& a, int64_t m, int n_row, uint32_t bit, int t) {
  sol_copy_out<NT>(a.canon + m * n_row, nullptr, n_row, t);
  if (t == 0) {
    a.rank[m] = 0;
    a.key[m] = 0;
    if (a.residual) a.residual[m] = -1;
    if (a.status) atomicOr(a.status, bit);
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void solution_canon_kernel(SolArgs a) {
  // two images of a.img bytes (the terms, the canon row), then K rows of kSolWRow bytes (the verifier's w tokens)
  extern __shared__ __attribute__((aligned(16))) uint8_t sol_lds[];
  __shared__ uint64_t red[NT];
  __shared__ uint8_t fcode[3 * TG_SOL_MAX_K];  // per factor: 0 all zero, 1 as it was, 2 negated; | 4: the negation left int8
  __shared__ int8_t tsign[TG_SOL_MAX_K];       // per term: 0 null, else sigma
  __shared__ uint8_t keep[TG_SOL_MAX_K];       // per place among the live terms: the term there is kept
  int8_t* const tok = reinterpret_cast<int8_t*>(sol_lds);
  int8_t* const out = tok + a.img;
  int8_t* const wq = out + a.img;
  const int t = threadIdx.x, S = a.S, A3 = 3 * S, K = a.K, shift = a.shift;
  const int n_row = K * A3, N3 = S * S * S;

  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    const int64_t L64 = a.lengths[m];  // uniform: every barrier below is reached by the whole workgroup or by none
    if (L64 < 0 || L64 > K) {          // checked before it addresses anything
      sol_bad_row<NT>(a, m, n_row, TG_SOL_BAD_LENGTH, t);
      continue;
    }
    const int L = static_cast<int>(L64);
    sol_copy_in<NT>(a.tokens + m * n_row, tok, L * A3, t);
    if (t < K) keep[t] = 0;
    __syncthreads();

    // ---- verify, from the original terms
    int nnz = 0;
    if (a.residual) {  // (the host refuses residual_nnz without targets)
      for (int x = t; x < L * kSolWRow; x += NT) {  // (the bytes beyond l = S - 1 only feed entries that are not counted)
        const int r = x / kSolWRow, l = x - r * kSolWRow;
        wq[x] = l < S ? tok[r * A3 + 2 * S + l] : static_cast<int8_t>(0);
      }
      __syncthreads();
      const int8_t* target = a.targets + m * N3;
      switch ((S + 7) / 8) {  // uniform
        case 1: nnz = sol_residual_nnz<NT, 1>(tok, wq, target, L, S, shift, t); break;
        case 2: nnz = sol_residual_nnz<NT, 2>(tok, wq, target, L, S, shift, t); break;
        case 3: nnz = sol_residual_nnz<NT, 3>(tok, wq, target, L, S, shift, t); break;
        default: nnz = sol_residual_nnz<NT, 4>(tok, wq, target, L, S, shift, t); break;
      }
    }
    __syncthreads();  // the verifier is done with the original bytes

    // ---- normalise: factor q = 3 * term + x lies at tok + q * S
    for (int q = t; q < 3 * L; q += NT) {
      int8_t* f = tok + q * S;
      int first = 0;
      for (int e = 0; e < S && first == 0; ++e) first = f[e] - shift;
      uint8_t code = first == 0 ? 0 : first > 0 ? 1 : 2;
      if (first < 0) {
        for (int e = 0; e < S; ++e) {
          const int v = 2 * shift - f[e];
          if (v < -128 || v > 127) code |= 4;
          f[e] = static_cast<int8_t>(v);
        }
      }
      fcode[q] = code;
    }
    __syncthreads();
    int bad = 0;
    if (t < L) {
      const int c0 = fcode[3 * t], c1 = fcode[3 * t + 1], c2 = fcode[3 * t + 2];
      const bool live = (c0 & 3) && (c1 & 3) && (c2 & 3);
      const int flips = ((c0 & 3) == 2) + ((c1 & 3) == 2) + ((c2 & 3) == 2);
      tsign[t] = live ? ((flips & 1) ? -1 : 1) : 0;
      bad = live && ((c0 | c1 | c2) & 4);
    }
    // The sort keys: the normalised terms again, P = 3S rounded up to 8 bytes apart in the canon image and the w rows
    // behind it (both idle here: K * P <= img + K * kSolWRow), every byte with its sign bit flipped and every 8 bytes
    // reversed, so that comparing the 8-byte words as unsigned integers compares the values as signed, in order.
    const int P = (A3 + 7) & ~7;
    for (int x = t; x < L * P; x += NT) {
      const int r = x / P, e = x - r * P;
      out[r * P + (e & ~7) + 7 - (e & 7)] = e < A3 ? static_cast<int8_t>(tok[r * A3 + e] ^ 0x80) : static_cast<int8_t>(0);
    }
    __syncthreads();

    // ---- order and merge: thread t = term t (K <= NT)
    const bool live = t < L && tsign[t] != 0;
    int lower = 0, before = 0, c = 0;
    if (live) {
      const uint64_t* me = reinterpret_cast<const uint64_t*>(out + t * P);
      for (int j = 0; j < L; ++j) {
        const int sj = tsign[j];
        if (sj == 0) continue;
        int d = 0;
        if (j != t) {
          const uint64_t* o = reinterpret_cast<const uint64_t*>(out + j * P);
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
    const int place = lower + before;  // distinct over the live terms
    if (live) keep[place] = kept;
    __syncthreads();  // the sort keys are read
    for (int q = t; q < (a.img + K * kSolWRow) / 16; q += NT) reinterpret_cast<uint4*>(out)[q] = uint4{0, 0, 0, 0};
    __syncthreads();
    if (kept) {
      int at = 0;
      for (int q = 0; q < place; ++q) at += keep[q];
      const int8_t* me = tok + t * A3;
      int8_t* dst = out + at * A3;
      for (int e = 0; e < 2 * S; ++e) dst[e] = me[e];
      for (int e = 2 * S; e < A3; ++e) {
        const int v = c < 0 ? 2 * shift - me[e] : me[e];
        bad |= v < -128 || v > 127;
        dst[e] = static_cast<int8_t>(v);
      }
    }
    const int rank = __syncthreads_count(kept);  // (also: the image is complete, the flags are read)
    if (__syncthreads_or(bad)) {
      sol_bad_row<NT>(a, m, n_row, TG_SOL_BAD_NEGATION, t);
      continue;
    }

    // ---- key, outputs
    const int n = rank * A3, words = (n + 7) / 8;  // the image is zero beyond n: the padding of the last word
    uint64_t h = 0;
    for (int k = t; k < words; k += NT)
      h += fmix64(reinterpret_cast<const uint64_t*>(out)[k] + static_cast<uint64_t>(k + 1) * 0x9E3779B97F4A7C15ull);
    h = sol_block_sum<NT>(h, red, t);
    const uint64_t total = sol_block_sum<NT>(static_cast<uint64_t>(nnz), red, t);
    sol_copy_out<NT>(a.canon + m * n_row, out, n_row, t);
    if (t == 0) {
      a.rank[m] = rank;
      a.key[m] = hash_finish(h, n);
      if (a.residual) a.residual[m] = static_cast<int32_t>(total);
    }
    __syncthreads();  // the images, the w rows and the flags are free for the next list
  }
}

}  // namespace tg

namespace {

int solution_sizes(const char* fn, int64_t M, int K, int S, int shift) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (K < 1 || K > TG_SOL_MAX_K) return tg_internal_fail(TG_ERR_INVALID, "%s: K=%d outside [1,%d]", fn, K, TG_SOL_MAX_K);
  if (shift < 0 || shift > TG_SOL_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_SOL_MAX_SHIFT);
  if (M < 0 || M > INT64_MAX / (static_cast<int64_t>(TG_SOL_MAX_K) * 3 * TG_MAX_S * TG_MAX_S))
    return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M);
  return TG_OK;
}

template <int NT>
int launch_solution(const tg::SolArgs& a, int per_cu, hipStream_t st) {
  const int64_t resident = static_cast<int64_t>(per_cu) * device_cu_count();
  return launch("tg_solution_canon", tg::solution_canon_kernel<NT>, static_cast<unsigned>(a.M < resident ? a.M : resident),
                NT, 2 * static_cast<size_t>(a.img) + static_cast<size_t>(a.K) * tg::kSolWRow, st, a);
}

}  // namespace

extern "C" int tg_solution_check(int64_t M, int K, int S, int shift) {
  return solution_sizes("tg_solution_check", M, K, S, shift);
}

extern "C" int tg_solution_canon(const int8_t* targets, const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int S,
                                 int shift, int8_t* canon, int32_t* rank, uint64_t* key, int32_t* residual_nnz,
                                 uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_solution_canon";
  if (const int rc = solution_sizes(fn, M, K, S, shift)) return rc;
  if (M == 0) return TG_OK;
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!lengths) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths", fn);
  if (!canon) return tg_internal_fail(TG_ERR_INVALID, "%s: null canon", fn);
  if (!rank) return tg_internal_fail(TG_ERR_INVALID, "%s: null rank", fn);
  if (!key) return tg_internal_fail(TG_ERR_INVALID, "%s: null key", fn);
  if (!targets && residual_nnz)
    return tg_internal_fail(TG_ERR_INVALID, "%s: residual_nnz needs targets (both NULL: no verification)", fn);
  if (canon == tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: canon == tokens: in-place operation is not supported", fn);
  if (!aligned(lengths, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: lengths not 8-byte aligned", fn);
  if (!aligned(key, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: key not 8-byte aligned", fn);
  if (!aligned(rank, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: rank not 4-byte aligned", fn);
  if (!aligned(residual_nnz, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: residual_nnz not 4-byte aligned", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const int img = (K * 3 * S + 15) & ~15;  // at most 24 KiB: two images, 8 KiB of w rows and the static LDS stay below 64 KiB
  const tg::SolArgs a{targets, tokens, lengths, M, canon, rank, key, residual_nnz, status, K, S, shift, img};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_solution<64>(a, 32, st);  // a wavefront per list
  return launch_solution<256>(a, 8, st);               // a 256-thread workgroup per list
}
