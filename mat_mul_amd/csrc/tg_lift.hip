// The sign lift of Z_2 lists to the integers (include/tensor_game_lift.h).  gfx950 only; part of libtensorgame.so.
//
// ONE workgroup of 256 threads per list (a grid-stride loop over the lists; no workgroup waits for another):
//   system  cells x (N + 1) bits, bit-packed in dwords and stored WORD-major: word k of cell r at sys[k * cells + r].
//           Thread t owns the cells t, t + 256, ...: a lane's neighbours own the neighbouring dwords, so every access
//           of a wavefront to its own cells is contiguous (coalesced in the workspace, conflict-free in LDS), and the
//           pivot row is one address for all lanes (a broadcast).  The system lives in LDS where the largest list of
//           that (K, S) fits (tg_lift2_workspace_bytes == 0), otherwise in the caller's workspace, a slice per
//           workgroup; the two kernels are one template.
//   build   a cell's row holds three bits per term that covers the cell; the owner writes them, no atomics.
//   pivots  Gauss-Jordan over the columns in ascending order: the lowest unused cell with the bit set is the pivot row
//           (a block-wide min), every other cell with the bit set XORs the pivot row in, from the pivot's word on (an
//           unused row is zero in every earlier column).  A column without such a cell is free.  That is the header's
//           rule: the pivot columns of the reduced form are the columns outside the span of the earlier ones.
//           Which cells are used is kept by their owner alone.
//   tries   factored once: per try the free values (Philox), x_c of a pivot column = the parity of its pivot row
//           against the free values and the right-hand side's bit, collected by ballots into a mask of the -1s per
//           term and mode; then the exact check, a cell per thread in int32, and a block-wide sum.  The first exact
//           try ends the loop.
// Every loop is bounded by K, S, N, tries or the number of lists.  No floating point, no atomics, plain vector stores.
// The exact check is the arithmetic of tg_solution_canon's verification (target - sum of the terms in int32, count the
// non-zero cells), but over mask terms with a sign mask, a cell per thread: it shares no code with the token form.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/tensor_game_lift.h"
#include "tg_lists.h"

namespace tg {

constexpr int kLiftThreads = 256;
constexpr int kLiftWaves = kLiftThreads / 64;
constexpr int kLiftMaxRd = 3 * TG_FLIP_MAX_K;                                          // (term, mode) pairs: 384
constexpr int kLiftMaxWords = (kLiftMaxRd * TG_MAX_S + 32) / 32;                       // words of a row: 385
constexpr int kLiftOwned = TG_MAX_S * TG_MAX_S * TG_MAX_S / kLiftThreads;              // cells per thread: 128
// the fixed part of the dynamic LDS, in dwords (every offset a multiple of 4)
constexpr int kOffMasks = 0;
constexpr int kOffColbase = kOffMasks + kLiftMaxRd;
constexpr int kOffNeg = kOffColbase + ((kLiftMaxRd + 1 + 3) & ~3);
constexpr int kOffXfree = kOffNeg + kLiftMaxRd;
constexpr int kOffUsed = kOffXfree + ((kLiftMaxWords + 3) & ~3);
constexpr int kOffRed = kOffUsed + kLiftOwned / 32 * kLiftThreads;
constexpr int kLiftFixedWords = kOffRed + 8;

struct Lift2Args {
  const int8_t* targets;  // (W, S, S, S)
  const int32_t* lists;   // (W, K, 3)
  const int32_t* ranks;   // (W)
  int8_t* tokens;         // (W, K, 3S)
  int32_t* status;
  int32_t* try_used;
  int32_t* unknowns;
  int32_t* sys_rank;
  int32_t* miss;
  uint32_t* workspace;
  int64_t W, ws_words;    // dwords of one workspace slice
  uint64_t seed, list0;
  int K, S, shift, tries;
  int sys_words;          // S^3 * the words of the widest row of this (K, S)
};

// the sum / the minimum of v over the workgroup; red: kLiftWaves dwords nobody else uses
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ int block_min(int v, int* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = red[0] < red[1] ? red[0] : red[1], b = red[2] < red[3] ? red[2] : red[3];
  return a < b ? a : b;
}
static_assert(kLiftWaves == 4, "block_sum and block_min read four partial results");

template <bool kLds>
__global__ __launch_bounds__(kLiftThreads) void lift2_kernel(Lift2Args a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lift_smem[];
  uint32_t* masks = lift_smem + kOffMasks;                      // [3R] the list
  int* colbase = reinterpret_cast<int*>(lift_smem + kOffColbase);  // [3R + 1] the first column of (term, mode)
  uint32_t* neg = lift_smem + kOffNeg;                          // [3R] the candidate: bit e set where the value is -1
  uint32_t* xfree = lift_smem + kOffXfree;                      // [nw] the free values of a try, and bit N = 1
  uint32_t* usedw = lift_smem + kOffUsed;                       // [j >> 5][tid]: my j-th cell is a pivot row
  int* red = reinterpret_cast<int*>(lift_smem + kOffRed);
  uint32_t* sys = kLds ? lift_smem + kLiftFixedWords : a.workspace + static_cast<int64_t>(blockIdx.x) * a.ws_words;
  int* piv = reinterpret_cast<int*>(sys + a.sys_words);         // [N] the pivot row of a column, or -1 - f

  const int tid = threadIdx.x, lane = tid & 63;
  const int K = a.K, S = a.S, SS = S * S, rows = SS * S, row_bytes = K * 3 * S;
  const uint32_t smask = S >= 32 ? ~0u : (1u << S) - 1u;
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);

  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    __syncthreads();  // the list before this one is done with the LDS
    int8_t* tok = a.tokens + w * row_bytes;
    const int8_t* target = a.targets + w * rows;
    const int R = a.ranks[w];
    int status = -1, try_used = -1, N = 0, P = 0, miss = -1;
    bool lifted = false;
    if (R >= 0 && R <= K) {  // checked before it addresses anything
      const int32_t* list = a.lists + w * K * 3;
      for (int q = tid; q < 3 * R; q += kLiftThreads) masks[q] = static_cast<uint32_t>(list[q]) & smask;
#pragma unroll
      for (int j = 0; j < kLiftOwned / 32; ++j) usedw[j * kLiftThreads + tid] = 0u;
      __syncthreads();
      if (tid == 0) {
        int acc = 0;
        for (int q = 0; q < 3 * R; ++q) {
          colbase[q] = acc;
          acc += __popc(masks[q]);
        }
        colbase[3 * R] = acc;
      }
      __syncthreads();
      N = colbase[3 * R];
      const int nw = (N >> 5) + 1;  // N + 1 bits
      // ---- build: my cells' rows, D's parity and the right-hand side
      int odd = 0;
      for (int r = tid; r < rows; r += kLiftThreads) {
        const int i = r / SS, j = (r - i * SS) / S, k = r - i * SS - j * S;
        for (int kk = 0; kk < nw; ++kk) sys[kk * rows + r] = 0u;
        int cover = 0;
        for (int t = 0; t < R; ++t) {
          const uint32_t m0 = masks[3 * t], m1 = masks[3 * t + 1], m2 = masks[3 * t + 2];
          if ((m0 >> i) & (m1 >> j) & (m2 >> k) & 1u) {
            ++cover;
            const int c0 = colbase[3 * t] + __popc(m0 & ((1u << i) - 1u));
            const int c1 = colbase[3 * t + 1] + __popc(m1 & ((1u << j) - 1u));
            const int c2 = colbase[3 * t + 2] + __popc(m2 & ((1u << k) - 1u));
            sys[(c0 >> 5) * rows + r] |= 1u << (c0 & 31);
            sys[(c1 >> 5) * rows + r] |= 1u << (c1 & 31);
            sys[(c2 >> 5) * rows + r] |= 1u << (c2 & 31);
          }
        }
        const int D = static_cast<int>(target[r]) - cover;
        odd += D & 1;
        if ((D >> 1) & 1) sys[(N >> 5) * rows + r] |= 1u << (N & 31);
      }
      odd = block_sum(odd, red);
      if (odd) {
        status = TG_LIFT2_NOT_MOD2;
        miss = odd;
        N = 0;
      } else {
        // ---- pivots: Gauss-Jordan, the columns in ascending order
        int nfree = 0;
        for (int c = 0; c < N; ++c) {
          const int kc = c >> 5;
          const uint32_t bit = 1u << (c & 31);
          int cand = INT_MAX;
          for (int j = 0, r = tid; r < rows; ++j, r += kLiftThreads)
            if ((sys[kc * rows + r] & bit) && !((usedw[(j >> 5) * kLiftThreads + tid] >> (j & 31)) & 1u)) {
              cand = r;
              break;
            }
          const int p = block_min(cand, red);
          if (p == INT_MAX) {
            if (tid == 0) piv[c] = -1 - nfree;
            ++nfree;
            continue;
          }
          if (tid == 0) piv[c] = p;
          ++P;
          for (int j = 0, r = tid; r < rows; ++j, r += kLiftThreads) {
            if (r == p)
              usedw[(j >> 5) * kLiftThreads + tid] |= 1u << (j & 31);
            else if (sys[kc * rows + r] & bit)
              for (int kk = kc; kk < nw; ++kk) sys[kk * rows + r] ^= sys[kk * rows + p];
          }
        }
        // ---- consistent iff no unused row is left with the right-hand side's bit
        int bad = 0;
        for (int j = 0, r = tid; r < rows; ++j, r += kLiftThreads)
          bad |= static_cast<int>((sys[(N >> 5) * rows + r] >> (N & 31)) & ~(usedw[(j >> 5) * kLiftThreads + tid] >> (j & 31)) & 1u);
        bad = block_sum(bad, red);
        if (bad) {
          status = TG_LIFT2_INCONSISTENT;
        } else {
          // ---- tries
          const uint64_t g = a.list0 + static_cast<uint64_t>(w);
          int best = INT_MAX;
          for (int t = 0; t < a.tries; ++t) {
            for (int c0 = 0; c0 < nw * 32; c0 += kLiftThreads) {
              const int c = c0 + tid;
              uint32_t v = c == N ? 1u : 0u;
              if (c < N && t > 0) {
                const int pv = piv[c];
                if (pv < 0) {
                  const uint32_t f = static_cast<uint32_t>(-1 - pv);
                  const U4 o = philox4x32_10(U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32),
                                                static_cast<uint32_t>(t), TG_LIFT2_DOMAIN + (f >> 7)}, k0, k1);
                  const uint32_t sel = (f >> 5) & 3u;
                  const uint32_t word = sel == 0 ? o.x : sel == 1 ? o.y : sel == 2 ? o.z : o.w;
                  v = (word >> (f & 31u)) & 1u;
                }
              }
              const uint64_t ball = __ballot(v != 0u);
              if ((lane & 31) == 0 && (c >> 5) < nw) xfree[c >> 5] = static_cast<uint32_t>(ball >> (lane & 32));
            }
            __syncthreads();
            for (int q0 = 0; q0 < 3 * R * 32; q0 += kLiftThreads) {
              const int q = q0 + tid, rd = q >> 5, e = q & 31;
              uint32_t xb = 0u;
              if (rd < 3 * R) {
                const uint32_t m = masks[rd];
                if ((m >> e) & 1u) {
                  const int c = colbase[rd] + __popc(m & ((1u << e) - 1u));
                  const int pv = piv[c];
                  if (pv < 0) {
                    xb = (xfree[c >> 5] >> (c & 31)) & 1u;
                  } else {
                    uint32_t par = 0u;
                    for (int kk = c >> 5; kk < nw; ++kk) par ^= sys[kk * rows + pv] & xfree[kk];
                    xb = static_cast<uint32_t>(__popc(par)) & 1u;
                  }
                }
              }
              const uint64_t ball = __ballot(xb != 0u);
              if (e == 0 && rd < 3 * R) neg[rd] = static_cast<uint32_t>(ball >> (lane & 32));
            }
            __syncthreads();
            int cnt = 0;
            for (int r = tid; r < rows; r += kLiftThreads) {
              const int i = r / SS, j = (r - i * SS) / S, k = r - i * SS - j * S;
              int val = 0;
              for (int u = 0; u < R; ++u) {
                const uint32_t m0 = masks[3 * u], m1 = masks[3 * u + 1], m2 = masks[3 * u + 2];
                if ((m0 >> i) & (m1 >> j) & (m2 >> k) & 1u)
                  val += ((neg[3 * u] >> i) ^ (neg[3 * u + 1] >> j) ^ (neg[3 * u + 2] >> k)) & 1u ? -1 : 1;
              }
              cnt += static_cast<int>(target[r]) - val != 0;
            }
            cnt = block_sum(cnt, red);
            best = cnt < best ? cnt : best;
            if (cnt == 0) {
              try_used = t;
              break;
            }
          }
          miss = best;
          lifted = try_used >= 0;
          status = lifted ? TG_LIFT2_OK : TG_LIFT2_NOT_EXACT;
        }
      }
    }
    if (lifted) {
      for (int q = tid; q < row_bytes; q += kLiftThreads) {
        const int r = q / (3 * S), rem = q - r * 3 * S, d = rem / S, e = rem - d * S;
        int v = 0;
        if (r < R) {
          const int on = (masks[3 * r + d] >> e) & 1u, minus = (neg[3 * r + d] >> e) & 1u;
          v = on ? (minus ? -1 : 1) + a.shift : a.shift;
        }
        tok[q] = static_cast<int8_t>(v);
      }
    } else {
      for (int q = tid; q < row_bytes; q += kLiftThreads) tok[q] = 0;
    }
    if (tid == 0) {
      a.status[w] = status;
      a.try_used[w] = try_used;
      a.unknowns[w] = N;
      a.sys_rank[w] = P;
      a.miss[w] = miss;
    }
  }
}

}  // namespace tg

namespace {

struct Lift2Layout {
  int sys_words;     // S^3 * words of the widest row
  int64_t words;     // ... and the pivot table behind it
  int64_t lds_bytes;  // the dynamic LDS of the kernel that keeps all of it there
};

Lift2Layout lift2_layout(int K, int S) {
  const int n_max = 3 * K * S, nw_max = (n_max + 32) / 32;
  Lift2Layout l;
  l.sys_words = S * S * S * nw_max;
  l.words = static_cast<int64_t>(l.sys_words) + n_max;
  l.lds_bytes = ((tg::kLiftFixedWords + l.words) * 4 + 15) & ~int64_t{15};
  return l;
}

bool lift2_in_lds(const Lift2Layout& l) { return l.lds_bytes <= tg::kMaxDynamicLds; }

int64_t lift2_ws_bytes(const Lift2Layout& l) { return lift2_in_lds(l) ? 0 : (l.words * 4 + 255) & ~int64_t{255}; }

int lift2_sizes(const char* fn, int64_t W, int K, int S, int shift, int64_t tries, int64_t ws_lists) {
  if (const int rc = check_lists(fn, K, S, shift, TG_FLIP_MAX_K)) return rc;
  const int64_t most = INT64_MAX / (static_cast<int64_t>(TG_FLIP_MAX_K) * 3 * TG_MAX_S * TG_MAX_S);
  if (W < 0 || W > most) return tg_internal_fail(TG_ERR_INVALID, "%s: W=%lld out of range", fn, (long long)W);
  if (tries < 1 || tries > TG_LIFT2_MAX_TRIES)
    return tg_internal_fail(TG_ERR_INVALID, "%s: tries=%lld outside [1,%d]", fn, (long long)tries, TG_LIFT2_MAX_TRIES);
  if (ws_lists < 0 || ws_lists > TG_LIFT2_MAX_WS_LISTS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: ws_lists=%lld outside [0,%d]", fn, (long long)ws_lists, TG_LIFT2_MAX_WS_LISTS);
  if (ws_lists < 1 && lift2_ws_bytes(lift2_layout(K, S)) > 0)
    return tg_internal_fail(TG_ERR_INVALID, "%s: ws_lists=%lld < 1, and K=%d, S=%d need a workspace", fn, (long long)ws_lists, K, S);
  return TG_OK;
}

}  // namespace

extern "C" int64_t tg_lift2_workspace_bytes(int K, int S) {
  if (const int rc = check_lists("tg_lift2_workspace_bytes", K, S, 0, TG_FLIP_MAX_K)) return rc;
  return lift2_ws_bytes(lift2_layout(K, S));
}

extern "C" int tg_lift2_check(int64_t W, int K, int S, int shift, int64_t tries, int64_t ws_lists) {
  return lift2_sizes("tg_lift2_check", W, K, S, shift, tries, ws_lists);
}

extern "C" int tg_lift2_signs(const int8_t* targets, const int32_t* lists, const int32_t* ranks, int64_t W, int K, int S,
                              int shift, uint64_t seed, uint64_t list0, int64_t tries, int8_t* tokens, int32_t* status,
                              int32_t* try_used, int32_t* unknowns, int32_t* sys_rank, int32_t* miss, void* workspace,
                              int64_t ws_lists, tg_stream_t stream) {
  const char* fn = "tg_lift2_signs";
  if (const int rc = lift2_sizes(fn, W, K, S, shift, tries, ws_lists)) return rc;
  if (W == 0) return TG_OK;
  const struct { const void* p; const char* name; int align; } all[] = {
      {targets, "targets", 1}, {lists, "lists", 4}, {ranks, "ranks", 4}, {tokens, "tokens", 1}, {status, "status", 4},
      {try_used, "try_used", 4}, {unknowns, "unknowns", 4}, {sys_rank, "sys_rank", 4}, {miss, "miss", 4}};
  for (const auto& x : all)
    if (!x.p) return tg_internal_fail(TG_ERR_INVALID, "%s: null %s", fn, x.name);
  for (const auto& x : all)
    if (!aligned(x.p, x.align)) return tg_internal_fail(TG_ERR_INVALID, "%s: %s not %d-byte aligned", fn, x.name, x.align);
  const Lift2Layout l = lift2_layout(K, S);
  const int64_t ws_bytes = lift2_ws_bytes(l);
  if (ws_bytes > 0 && !workspace) return tg_internal_fail(TG_ERR_INVALID, "%s: null workspace (K=%d, S=%d need one)", fn, K, S);
  if (ws_bytes > 0 && !aligned(workspace, 16)) return tg_internal_fail(TG_ERR_INVALID, "%s: workspace not 16-byte aligned", fn);
  const tg::Lift2Args a{targets, lists, ranks, tokens, status, try_used, unknowns, sys_rank, miss,
                        static_cast<uint32_t*>(workspace), W, ws_bytes / 4, seed, list0, K, S, shift,
                        static_cast<int>(tries), l.sys_words};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ws_bytes == 0) {
    if (const int rc = lds_opt_in<tg::lift2_kernel<true>>(fn, static_cast<size_t>(l.lds_bytes))) return rc;
    return launch_resident(fn, tg::lift2_kernel<true>, W, 8, tg::kLiftThreads, static_cast<size_t>(l.lds_bytes), st, a);
  }
  const int64_t resident = int64_t{8} * device_cu_count();
  const int64_t grid = W < ws_lists ? (W < resident ? W : resident) : (ws_lists < resident ? ws_lists : resident);
  return launch(fn, tg::lift2_kernel<false>, static_cast<unsigned>(grid), tg::kLiftThreads, tg::kLiftFixedWords * 4, st, a);
}
