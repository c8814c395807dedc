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
// The verifier, the keys' byte map, the term signs, the rank sort and merge, the kept terms' offsets and the key are the
// functions of tg_sol_phases.h, which tg_orbits.hip calls too; the host checks the list entries share are tg_lists.h.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_solutions.h"
#include "tg_lists.h"
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
      sol_stage_w<NT>(tok, wq, L, S, t);
      __syncthreads();
      nnz = sol_verify<NT>(tok, wq, a.targets + m * N3, L, S, shift, t);
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
    int bad = sol_term_sign(fcode, tsign, L, t);
    // The sort keys (tg_sol_phases.h): the normalised terms again, P = 3S rounded up to 8 bytes apart in the canon image
    // and the w rows behind it (both idle here: K * P <= img + K * kSolWRow).
    const int P = (A3 + 7) & ~7;
    for (int x = t; x < L * P; x += NT) {
      const int r = x / P, e = x - r * P;
      out[r * P + sol_key_at(e)] = static_cast<int8_t>(e < A3 ? sol_key_flip(tok[r * A3 + e]) : 0);
    }
    __syncthreads();

    // ---- order and merge: thread t = term t (K <= NT)
    const SolRank o = sol_rank(reinterpret_cast<const uint8_t*>(out), tsign, keep, L, P, t);
    __syncthreads();  // the sort keys are read
    for (int q = t; q < (a.img + K * kSolWRow) / 16; q += NT) reinterpret_cast<uint4*>(out)[q] = uint4{0, 0, 0, 0};
    __syncthreads();
    if (o.kept) {
      const int8_t* me = tok + t * A3;
      int8_t* dst = out + sol_kept_below(keep, o.place) * A3;
      for (int e = 0; e < 2 * S; ++e) dst[e] = me[e];
      for (int e = 2 * S; e < A3; ++e) {
        const int v = o.c < 0 ? 2 * shift - me[e] : me[e];
        bad |= v < -128 || v > 127;
        dst[e] = static_cast<int8_t>(v);
      }
    }
    const int rank = __syncthreads_count(o.kept);  // (also: the image is complete, the flags are read)
    if (__syncthreads_or(bad)) {
      sol_bad_row<NT>(a, m, n_row, TG_SOL_BAD_NEGATION, t);
      continue;
    }

    // ---- key, outputs
    const uint64_t key = sol_image_key<NT>(out, rank * A3, red, t);
    const uint64_t total = sol_block_sum<NT>(static_cast<uint64_t>(nnz), red, t);
    sol_copy_out<NT>(a.canon + m * n_row, out, n_row, t);
    if (t == 0) {
      a.rank[m] = rank;
      a.key[m] = key;
      if (a.residual) a.residual[m] = static_cast<int32_t>(total);
    }
    __syncthreads();  // the images, the w rows and the flags are free for the next list
  }
}

}  // namespace tg

namespace {

int solution_sizes(const char* fn, int64_t M, int K, int S, int shift) {
  if (const int rc = check_lists(fn, K, S, shift, TG_SOL_MAX_K)) return rc;
  return check_list_count(fn, M);
}

template <int NT>
int launch_solution(const tg::SolArgs& a, int per_cu, hipStream_t st) {
  return launch_resident("tg_solution_canon", tg::solution_canon_kernel<NT>, a.M, per_cu, NT,
                         2 * static_cast<size_t>(a.img) + static_cast<size_t>(a.K) * tg::kSolWRow, st, a);
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
  if (const int rc = check_canon_pointers(fn, {targets, tokens, lengths, canon, rank, key, residual_nnz, status})) return rc;
  const int img = list_image_bytes(K, S);  // two images, 8 KiB of w rows and the static LDS stay below 64 KiB
  const tg::SolArgs a{targets, tokens, lengths, M, canon, rank, key, residual_nnz, status, K, S, shift, img};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_solution<64>(a, 32, st);  // a wavefront per list
  return launch_solution<256>(a, 8, st);               // a 256-thread workgroup per list
}
