// Random walks on the flip graph (include/tensor_game_flips.h), and the same walks with plus transitions
// (include/tensor_game_flips_plus.h).  gfx950 only; part of libtensorgame.so.
//
// A walk is sequential, so the parallelism is across walks and, inside a step, across terms: ONE wavefront (a 64-thread
// workgroup of its own, so nothing ever waits for another wavefront) per walk, lane l owning terms l and l + 64.
//   list    in LDS, in the header's normalised form: per term the three vectors n_0, n_1, n_2 as int8 values, each padded
//           with zero bytes to whole dwords so that two vectors compare dword by dword, and the sign s.  The term stride is
//           an odd number of dwords (the lanes of a wavefront reading "their" term fall into different banks).
//   masks   per owned term and mode, a K-bit mask (one or two 64-bit words in VGPRs) of the terms that share that
//           normalised vector.  A flip changes two terms, a merge one, a removal moves one: per changed slot p every lane
//           compares its own terms with term p on the values (6 vector compares) and the 6 ballots ARE term p's new masks;
//           the K^2 compares are done once per launch, not per step.
//   matches C = the popcounts of the masks above the diagonal, summed by a wavefront prefix sum; the lane whose prefix
//           interval holds the drawn number walks its own masks in (j, m) order to the match and broadcasts it.
//   reduce  candidates are the pairs whose masks agree in two modes; they are visited in ascending (i, j) order with
//           ballots, a pair that would leave the bound is passed over, and after a merge the scan starts again: what the
//           header's full scans give, because a pair that does not involve a changed term is either no candidate or
//           passed over again.
//   draws   Philox for 64 consecutive steps at a time, one step per lane.
//   plus    (flip_advance_plus_kernel only) two terms become three: the pair number is located with the same prefix sum
//           over L - 1 - t pairs per term, the three new vectors are tested before anything is written, the third term
//           is appended in slot L, and the three slots are refreshed like any changed term; then the reduce above.
//           flip_begin_kernel and flip_advance_kernel do not see any of it: FlipWalk::step is as it was.
// Every loop is bounded by n_steps, K, S or the number of walks; none waits on memory another wavefront writes.  No
// floating point, no atomics but the OR of the sticky bad-row bits.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_flips_plus.h"
#include "tg_lists.h"

namespace tg {

struct FlipArgs {
  const int8_t* tokens;    // begin: (M, K, 3S)
  const int64_t* lengths;  // begin: (M)
  const int64_t* src;      // begin: (W) or null
  int64_t M, W;
  int8_t* cur;             // (W, K, 3S)
  int32_t* cur_rank;
  int8_t* best;
  int32_t* best_rank;
  int64_t* best_step;
  int64_t* flips;
  int32_t* state;
  uint32_t* status;        // begin: or null
  uint64_t seed, walk0;
  int64_t step0;
  int n_steps;
  int K, S, shift, bound;
};

__device__ __forceinline__ uint64_t bits_above(int t, int w) {  // of word w: the bits of the terms > t
  const int r = t - 64 * w;
  return r < 0 ? ~0ull : r >= 63 ? 0ull : (~0ull << (r + 1));
}
__device__ __forceinline__ uint64_t bits_below(int n, int w) {  // of word w: the bits of the terms < n
  const int r = n - 64 * w;
  return r <= 0 ? 0ull : r >= 64 ? ~0ull : ((1ull << r) - 1);
}
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// NW = 64-bit words per mask = terms per lane: 1 while K <= 64, 2 up to TG_FLIP_MAX_K
template <int NW>
struct FlipWalk {
  uint32_t* vec;  // LDS: n_m of term t at vec + t * TS + m * SW (SW dwords, zero beyond S bytes)
  int8_t* sgn;    // LDS: s of term t (0 while the term is being loaded and is null)
  int S, SW, TS, K, L, lane, bound, shift;
  uint64_t eq[NW][3][NW];  // eq[s][m][w]: word w of the terms that share n_m with my term lane + 64 s

  __device__ __forceinline__ int8_t* bytes(int t, int m) const { return reinterpret_cast<int8_t*>(vec + t * TS + m * SW); }

  __device__ __forceinline__ bool same(int t, int p, int m) const {  // n_m(t) == n_m(p), on the values
    const uint32_t* a = vec + t * TS + m * SW;
    const uint32_t* b = vec + p * TS + m * SW;
    uint32_t x = 0;
    for (int e = 0; e < SW; ++e) x |= a[e] ^ b[e];
    return x == 0;
  }

  // term p (uniform, < L) has changed or is new in its slot: bit p of every mask, and the masks of term p
  __device__ __forceinline__ void refresh(int p) {
    const int ps = p >> 6, pl = p & 63;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int t = lane + 64 * s;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const bool e = t < L && same(t, p, m);
        const uint64_t b = __ballot(e);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          if (w == ps) eq[s][m][w] = (eq[s][m][w] & ~(1ull << pl)) | (static_cast<uint64_t>(e) << pl);
          if (w == ps && lane == pl) eq[w][m][s] = b;
        }
      }
    }
  }

  __device__ __forceinline__ void refresh_all() {
#pragma unroll
    for (int s = 0; s < NW; ++s)
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int w = 0; w < NW; ++w) eq[s][m][w] = 0;
    for (int p = 0; p < L; ++p) refresh(p);
  }

  // Removing slot p (uniform): the last live term moves into it.
  __device__ __forceinline__ void remove(int p) {
    const int last = L - 1;
    if (p != last) {
      if (lane < TS) vec[p * TS + lane] = vec[last * TS + lane];
      if (lane == 0) sgn[p] = sgn[last];
    }
    L = last;
    __syncthreads();
    if (p != last) refresh(p);
  }

  // lane e < S holds x[e]: the vector goes to n_m of term t normalised; returns the sign taken out (0: all zero, and
  // nothing is written)
  __device__ __forceinline__ int put_normalised(int t, int m, int x) {
    const uint64_t nz = __ballot(lane < S && x != 0);
    if (nz == 0) return 0;
    const int first = __shfl(x, static_cast<int>(__builtin_ctzll(nz)));
    const int sg = first > 0 ? 1 : -1;
    if (lane < S) bytes(t, m)[lane] = static_cast<int8_t>(sg * x);
    return sg;
  }

  // One pair of a reduce scan (i < j, uniform, a candidate).  True if it merged.
  __device__ __forceinline__ bool try_merge(int i, int j) {
    const bool s0 = same(i, j, 0), s1 = same(i, j, 1), s2 = same(i, j, 2);
    const int d = uniform(s0 && s1 && s2 ? 2 : !s0 ? 0 : !s1 ? 1 : 2);
    const int si = sgn[i], sj = sgn[j];
    const int z = lane < S ? si * bytes(i, d)[lane] + sj * bytes(j, d)[lane] : 0;
    if (__any(z > bound || z < -bound)) return false;
    const int sg = put_normalised(i, d, z);
    if (sg == 0) {
      remove(j);
      remove(i);
      return true;
    }
    if (lane == 0) sgn[i] = static_cast<int8_t>(sg);
    __syncthreads();
    remove(j);
    refresh(i);
    return true;
  }

  __device__ __forceinline__ void reduce() {
    bool again = true;
    for (int pass = 0; pass <= K && again; ++pass) {  // every pass but the last lowers L
      again = false;
      uint64_t cand[NW][NW];
#pragma unroll
      for (int s = 0; s < NW; ++s) {
        const int t = lane + 64 * s;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const uint64_t e0 = eq[s][0][w], e1 = eq[s][1][w], e2 = eq[s][2][w];
          cand[s][w] = t < L ? ((e0 & e1) | (e0 & e2) | (e1 & e2)) & bits_above(t, w) & bits_below(L, w) : 0ull;
        }
      }
#pragma unroll
      for (int s = 0; s < NW; ++s) {
        uint64_t any = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) any |= cand[s][w];
        uint64_t has = __ballot(any != 0);
        while (has != 0 && !again) {  // the terms i of this slot that have a candidate, ascending
          const int il = static_cast<int>(__builtin_ctzll(has));
          has &= has - 1;
#pragma unroll
          for (int w = 0; w < NW; ++w) {
            uint64_t cw = __shfl(static_cast<unsigned long long>(cand[s][w]), il);
            while (cw != 0 && !again) {  // its partners j, ascending
              const int j = 64 * w + static_cast<int>(__builtin_ctzll(cw));
              cw &= cw - 1;
              again = try_merge(il + 64 * s, j);
            }
          }
        }
      }
    }
  }

  // my matches (i = my terms, j > i), per slot
  __device__ __forceinline__ int count(int s) const {
    const int t = lane + 64 * s;
    int c = 0;
    if (t < L) {
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int w = 0; w < NW; ++w) c += __popcll(eq[s][m][w] & bits_above(t, w) & bits_below(L, w));
    }
    return c;
  }

  // the kk-th match of my term of slot s in (j, m) order, as j * 4 + m
  __device__ __forceinline__ int locate(int s, int kk) const {
    const int t = lane + 64 * s;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const uint64_t keep = bits_above(t, w) & bits_below(L, w);
      const uint64_t a0 = eq[s][0][w] & keep, a1 = eq[s][1][w] & keep, a2 = eq[s][2][w] & keep;
      uint64_t un = a0 | a1 | a2;
      while (un != 0) {
        const int b = static_cast<int>(__builtin_ctzll(un));
        un &= un - 1;
        const int h0 = (a0 >> b) & 1, h1 = (a1 >> b) & 1, h2 = (a2 >> b) & 1;
        const int n = h0 + h1 + h2;
        if (kk < n) {
          const int m = kk == 0 ? (h0 ? 0 : h1 ? 1 : 2) : kk == 1 ? (h0 && h1 ? 1 : 2) : 2;
          return (64 * w + b) * 4 + m;
        }
        kk -= n;
      }
    }
    return 0;  // (not reached: kk is below my count)
  }

  __device__ __forceinline__ int scan(int v) const {  // inclusive prefix sum over the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(v, d);
      if (lane >= d) v += u;
    }
    return v;
  }

  // One step with the draw ox.  0: no match (stuck), 1: the flip was refused, 2: accepted.
  __device__ __forceinline__ int step(uint32_t ox) {
    int cnt[NW], inc[NW], tot[NW], C = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      cnt[s] = count(s);
      inc[s] = scan(cnt[s]);
      tot[s] = uniform(__shfl(inc[s], 63));
      C += tot[s];
    }
    if (C == 0) return 0;
    const uint32_t c = static_cast<uint32_t>((static_cast<uint64_t>(ox) * (8u * static_cast<uint32_t>(C))) >> 32);
    int k = static_cast<int>(c >> 3);
    const int variant = static_cast<int>(c & 7);
    int i = 0, jm = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      if (k >= 0 && k < tot[s]) {
        const int il = static_cast<int>(__builtin_ctzll(__ballot(inc[s] > k)));
        int found = 0;
        if (lane == il) found = locate(s, k - (inc[s] - cnt[s]));
        jm = uniform(__shfl(found, il));
        i = il + 64 * s;
        k = -1;
      } else if (k >= 0) {
        k -= tot[s];
      }
    }
    const int j = jm >> 2, m = jm & 3;
    const int eps = (variant & 1) ? -1 : 1;
    int q = m == 0 ? 1 : 0, r = m == 2 ? 1 : 2;
    if (variant & 2) { const int x = q; q = r; r = x; }
    const int a = (variant & 4) ? j : i, b = (variant & 4) ? i : j;
    const int sa = sgn[a], sb = sgn[b];
    int nq = 0, nr = 0;
    if (lane < S) {
      nq = bytes(a, q)[lane] + eps * bytes(b, q)[lane];
      nr = sb * bytes(b, r)[lane] - eps * sa * bytes(a, r)[lane];
    }
    if (__any(nq > bound || nq < -bound || nr > bound || nr < -bound)) return 1;
    const int sq = put_normalised(a, q, nq);  // a' = x, nq, s_a n_r(a);  b' = x, n_q(b), nr
    const int sr = put_normalised(b, r, nr);
    if (lane == 0) {
      if (sq != 0) sgn[a] = static_cast<int8_t>(sa * sq);
      if (sr != 0) sgn[b] = static_cast<int8_t>(sr);
    }
    __syncthreads();
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const bool null_hi = (a > b ? sq : sr) == 0, null_lo = (a > b ? sr : sq) == 0;
    if (null_hi) remove(hi);  // the higher slot first
    if (null_lo) remove(lo);
    if (!null_hi && hi < L) refresh(hi);  // (hi >= L: it was the last term and has moved into lo, refreshed there)
    if (!null_lo) refresh(lo);
    reduce();
    return 2;
  }

  // The plus (tensor_game_flips_plus.h step 4) the draws oy, oz choose; needs 2 <= L < K.  1: refused, 2: accepted.
  __device__ __forceinline__ int plus(uint32_t oy, uint32_t oz) {
    const uint32_t P = static_cast<uint32_t>(L * (L - 1) / 2);
    int k = static_cast<int>((static_cast<uint64_t>(oy) * P) >> 32);
    const int v = static_cast<int>((static_cast<uint64_t>(oz) * 24u) >> 32);
    // pair number k: term t owns the L - 1 - t pairs (t, j > t); the slots in turn, a prefix sum over each
    int i = 0, j = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int t = lane + 64 * s;
      const int own = t < L - 1 ? L - 1 - t : 0;
      const int inc = scan(own);
      const int tot = uniform(__shfl(inc, 63));
      if (k >= 0 && k < tot) {
        const int il = static_cast<int>(__builtin_ctzll(__ballot(inc > k)));
        const int before = uniform(__shfl(inc - own, il));
        i = il + 64 * s;
        j = i + 1 + (k - before);
        k = -1;
      } else if (k >= 0) {
        k -= tot;
      }
    }
    const int a = (v & 1) ? j : i, b = (v & 1) ? i : j;
    const int eps = (v & 2) ? -1 : 1;
    const int perm = v >> 2;  // 012, 021, 102, 120, 201, 210
    const int p = perm >> 1, q = perm == 0 || perm == 5 ? 1 : perm == 1 || perm == 3 ? 2 : 0, r = 3 - p - q;
    const int sa = sgn[a], sb = sgn[b];
    int d1 = 0, d2 = 0, d3 = 0;  // A_p - B_p, A_r + B_r, B_q - A_q
    if (lane < S) {
      d1 = bytes(a, p)[lane] - eps * bytes(b, p)[lane];
      d2 = sa * bytes(a, r)[lane] + eps * sb * bytes(b, r)[lane];
      d3 = bytes(b, q)[lane] - bytes(a, q)[lane];
    }
    if (__any(d1 > bound || d1 < -bound || d2 > bound || d2 < -bound || d3 > bound || d3 < -bound)) return 1;
    const int n = L;  // the new slot: t2 = B_p, A_q, d2 (its copies first: slot a keeps mode q and slot b mode p)
    const uint32_t cp = lane < SW ? vec[b * TS + p * SW + lane] : 0u, cq = lane < SW ? vec[a * TS + q * SW + lane] : 0u;
    const int s1 = put_normalised(a, p, d1);  // t1 = d1, A_q, A_r
    const int s3 = put_normalised(b, q, d3);  // t3 = B_p, d3, B_r: eps twice
    const int s2 = put_normalised(n, r, d2);
    if (s2 != 0 && lane < SW) {
      vec[n * TS + p * SW + lane] = cp;
      vec[n * TS + q * SW + lane] = cq;
    }
    if (lane == 0) {
      if (s1 != 0) sgn[a] = static_cast<int8_t>(sa * s1);
      if (s3 != 0) sgn[b] = static_cast<int8_t>(sb * s3);
      if (s2 != 0) sgn[n] = static_cast<int8_t>(eps * s2);
    }
    __syncthreads();
    if (s2 != 0) L = n + 1;  // (a null t2 would be removed first, from the last slot: it is not appended)
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const bool null_hi = (a > b ? s1 : s3) == 0, null_lo = (a > b ? s3 : s1) == 0;
    if (null_hi) remove(hi);  // the higher slot first; the last term moves in and is refreshed there
    if (null_lo) remove(lo);
    if (s2 != 0 && n < L) refresh(n);  // bit n of every mask and all of n's masks: nothing of an earlier tenant stays
    if (!null_hi && hi < L) refresh(hi);
    if (!null_lo && lo < L) refresh(lo);
    reduce();
    return 2;
  }

  // ---- global <-> LDS
  __device__ __forceinline__ void clear() {
    for (int x = lane; x < K * TS; x += 64) vec[x] = 0;
    for (int x = lane; x < K; x += 64) sgn[x] = 0;
    __syncthreads();
  }

  // rows[0:n] (tokens) -> values in LDS; true if some value is outside [-bound, bound]
  __device__ __forceinline__ bool stage(const int8_t* rows, int n) {
    const int A3 = 3 * S;
    bool out = false;
    for (int x = lane; x < n * A3; x += 64) {
      const int t = x / A3, e = x - t * A3, m = e / S;
      const int f = rows[x] - shift;
      out |= f > bound || f < -bound;
      bytes(t, m)[e - m * S] = static_cast<int8_t>(f);
    }
    __syncthreads();
    return __any(out);
  }

  // the staged terms [0:n] to the normalised form, each by its owner; sgn = 0 marks a null term
  __device__ __forceinline__ void normalise(int n) {
    for (int t = lane; t < n; t += 64) {
      int sg = 1;
      for (int m = 0; m < 3; ++m) {
        int8_t* f = bytes(t, m);
        int first = 0;
        for (int e = 0; e < S && first == 0; ++e) first = f[e];
        if (first < 0)
          for (int e = 0; e < S; ++e) f[e] = static_cast<int8_t>(-f[e]);
        sg = first == 0 ? 0 : first < 0 ? -sg : sg;
      }
      sgn[t] = static_cast<int8_t>(sg);
    }
    __syncthreads();
  }

  // Drop the null terms of [0:n], keeping the order; sets L.
  __device__ __forceinline__ void compact(int n) {
    int dst = 0;
    for (int t = 0; t < n; ++t) {
      const int sg = sgn[t];  // uniform
      if (sg == 0) continue;
      if (dst != t) {
        if (lane < TS) vec[dst * TS + lane] = vec[t * TS + lane];
        if (lane == 0) sgn[dst] = static_cast<int8_t>(sg);
        __syncthreads();
      }
      ++dst;
    }
    L = dst;
    __syncthreads();
  }

  // the list in stored form as tokens, zero bytes at and beyond L (n_live < 0: zero bytes everywhere)
  __device__ __forceinline__ void store(int8_t* rows, int n_live) const {
    const int A3 = 3 * S;
    for (int x = lane; x < K * A3; x += 64) {
      const int t = x / A3, e = x - t * A3, m = e / S;
      int8_t v = 0;
      if (t < n_live) {
        const int f = bytes(t, m)[e - m * S];
        v = static_cast<int8_t>((m == 2 ? sgn[t] * f : f) + shift);
      }
      rows[x] = v;
    }
  }
};

template <int NW>
__device__ __forceinline__ FlipWalk<NW> flip_walk(const FlipArgs& a, uint32_t* lds) {
  FlipWalk<NW> w;
  w.S = a.S;
  w.SW = (a.S + 3) / 4;
  w.TS = (3 * w.SW) | 1;
  w.K = a.K;
  w.L = 0;
  w.lane = threadIdx.x;
  w.bound = a.bound;
  w.shift = a.shift;
  w.vec = lds;
  w.sgn = reinterpret_cast<int8_t*>(lds + a.K * w.TS);
  return w;
}

template <int NW>
__global__ __launch_bounds__(64) void flip_begin_kernel(FlipArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t flip_lds[];
  FlipWalk<NW> wk = flip_walk<NW>(a, flip_lds);
  const int64_t n_row = static_cast<int64_t>(a.K) * 3 * a.S;
  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    uint32_t bad = 0;
    int64_t m = a.src ? a.src[w] : w;
    int64_t L0 = 0;
    if (m < 0 || m >= a.M) {  // checked before it addresses anything
      bad = TG_FLIP_BAD_SRC;
    } else {
      L0 = a.lengths[m];
      if (L0 < 0 || L0 > a.K) bad = TG_FLIP_BAD_LENGTH;
    }
    wk.clear();
    if (!bad && wk.stage(a.tokens + m * n_row, static_cast<int>(L0))) bad = TG_FLIP_BAD_RANGE;
    int rank = 0;
    if (!bad) {
      wk.normalise(static_cast<int>(L0));
      wk.compact(static_cast<int>(L0));
      wk.refresh_all();
      wk.reduce();
      rank = wk.L;
    }
    wk.store(a.cur + w * n_row, bad ? -1 : rank);
    wk.store(a.best + w * n_row, bad ? -1 : rank);
    if (wk.lane == 0) {
      a.cur_rank[w] = rank;
      a.best_rank[w] = rank;
      a.best_step[w] = 0;
      a.flips[w] = 0;
      a.state[w] = bad ? -1 : 0;
      if (bad && a.status) atomicOr(a.status, bad);
    }
    __syncthreads();  // the list is free for the next walk
  }
}

template <int NW>
__global__ __launch_bounds__(64) void flip_advance_kernel(FlipArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t flip_lds[];
  FlipWalk<NW> wk = flip_walk<NW>(a, flip_lds);
  const int64_t n_row = static_cast<int64_t>(a.K) * 3 * a.S;
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);
  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    const int L0 = a.cur_rank[w];
    if (a.state[w] != 0 || L0 < 0 || L0 > a.K) continue;  // left exactly as it is (uniform)
    const uint64_t g = a.walk0 + static_cast<uint64_t>(w);
    wk.clear();
    wk.stage(a.cur + w * n_row, L0);
    wk.normalise(L0);
    wk.L = L0;
    wk.refresh_all();
    int best = a.best_rank[w];
    int64_t accepted = 0;
    int stuck = 0;
    uint32_t ox64 = 0;
    for (int k = 0; k < a.n_steps; ++k) {
      if ((k & 63) == 0) {  // the draws of steps k .. k + 63, one per lane
        const uint32_t t = static_cast<uint32_t>(static_cast<uint64_t>(a.step0) + static_cast<uint64_t>(k + wk.lane));
        ox64 = philox4x32_10(U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), t, TG_FLIP_DOMAIN}, k0, k1).x;
      }
      const uint32_t ox = static_cast<uint32_t>(uniform(static_cast<int>(__shfl(ox64, k & 63))));
      const int what = wk.step(ox);
      if (what == 0) {
        stuck = 1;
        break;
      }
      accepted += what == 2;
      if (wk.L < best) {
        best = wk.L;
        wk.store(a.best + w * n_row, best);
        if (wk.lane == 0) {
          a.best_rank[w] = best;
          a.best_step[w] = a.step0 + k + 1;
        }
      }
    }
    wk.store(a.cur + w * n_row, wk.L);
    if (wk.lane == 0) {
      a.cur_rank[w] = wk.L;
      a.flips[w] += accepted;
      if (stuck) a.state[w] = 1;
    }
    __syncthreads();  // the list is free for the next walk
  }
}

struct FlipPlusArgs {
  FlipArgs f;
  int32_t* since;   // (W)
  int64_t* pluses;  // (W)
  int plus_after, plus_slack;
};

// tg_flip_advance_plus: flip_advance_kernel's walk with the choice of tensor_game_flips_plus.h in front of every step.
// since, pluses and the cap are wavefront-uniform scalars, read once per walk and written once, by lane 0.
template <int NW>
__global__ __launch_bounds__(64) void flip_advance_plus_kernel(FlipPlusArgs pa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t flip_lds[];
  const FlipArgs& a = pa.f;
  FlipWalk<NW> wk = flip_walk<NW>(a, flip_lds);
  const int64_t n_row = static_cast<int64_t>(a.K) * 3 * a.S;
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);
  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    const int L0 = a.cur_rank[w];
    if (a.state[w] != 0 || L0 < 0 || L0 > a.K) continue;  // left exactly as it is (uniform)
    const uint64_t g = a.walk0 + static_cast<uint64_t>(w);
    wk.clear();
    wk.stage(a.cur + w * n_row, L0);
    wk.normalise(L0);
    wk.L = L0;
    wk.refresh_all();
    int best = a.best_rank[w];
    int since = uniform(pa.since[w]);
    int64_t accepted = 0, plused = 0;
    int stuck = 0;
    U4 o64{0, 0, 0, 0};
    for (int k = 0; k < a.n_steps; ++k) {
      if ((k & 63) == 0) {  // the draws of steps k .. k + 63, one per lane
        const uint32_t t = static_cast<uint32_t>(static_cast<uint64_t>(a.step0) + static_cast<uint64_t>(k + wk.lane));
        o64 = philox4x32_10(U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), t, TG_FLIP_DOMAIN}, k0, k1);
      }
      const int before = wk.L;
      const int64_t cap64 = static_cast<int64_t>(best) + pa.plus_slack;
      const bool can = before >= 2 && before < (cap64 < a.K ? cap64 : a.K);
      // a flip step unless the walk is due for a plus and may take one; step() returns 0 for C == 0
      int what = 0;
      if (!(can && since >= pa.plus_after)) {
        const uint32_t ox = static_cast<uint32_t>(uniform(static_cast<int>(__shfl(o64.x, k & 63))));
        what = wk.step(ox);
        accepted += what == 2;
      }
      bool progress = wk.L < before;
      if (what == 0) {
        if (!can) {
          stuck = 1;
          break;
        }
        const uint32_t oy = static_cast<uint32_t>(uniform(static_cast<int>(__shfl(o64.y, k & 63))));
        const uint32_t oz = static_cast<uint32_t>(uniform(static_cast<int>(__shfl(o64.z, k & 63))));
        progress = wk.plus(oy, oz) == 2;
        plused += progress;
      }
      since = progress ? 0 : since == INT32_MAX ? since : since + 1;
      if (wk.L < best) {
        best = wk.L;
        wk.store(a.best + w * n_row, best);
        if (wk.lane == 0) {
          a.best_rank[w] = best;
          a.best_step[w] = a.step0 + k + 1;
        }
      }
    }
    wk.store(a.cur + w * n_row, wk.L);
    if (wk.lane == 0) {
      a.cur_rank[w] = wk.L;
      a.flips[w] += accepted;
      pa.since[w] = since;
      pa.pluses[w] += plused;
      if (stuck) a.state[w] = 1;
    }
    __syncthreads();  // the list is free for the next walk
  }
}

}  // namespace tg

namespace {

int flip_sizes(const char* fn, int64_t M, int64_t W, int K, int S, int shift, int bound) {
  if (const int rc = check_lists(fn, K, S, shift, TG_FLIP_MAX_K)) return rc;
  if (bound < 1 || bound > TG_FLIP_MAX_BOUND)
    return tg_internal_fail(TG_ERR_INVALID, "%s: bound=%d outside [1,%d]", fn, bound, TG_FLIP_MAX_BOUND);
  const int64_t most = INT64_MAX / (static_cast<int64_t>(TG_FLIP_MAX_K) * 3 * TG_MAX_S);
  if (M < 0 || M > most) return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M);
  if (W < 0 || W > most) return tg_internal_fail(TG_ERR_INVALID, "%s: W=%lld out of range", fn, (long long)W);
  return TG_OK;
}

int flip_steps(const char* fn, int64_t step0, int64_t n_steps) {
  if (n_steps < 1 || n_steps > TG_FLIP_MAX_STEPS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_steps=%lld outside [1,%d]", fn, (long long)n_steps, TG_FLIP_MAX_STEPS);
  if (step0 < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: step0=%lld < 0", fn, (long long)step0);
  if (step0 + n_steps > (int64_t{1} << 32))
    return tg_internal_fail(TG_ERR_INVALID, "%s: step0 + n_steps=%lld beyond 2^32", fn, (long long)(step0 + n_steps));
  return TG_OK;
}

int flip_state_pointers(const char* fn, const int8_t* cur, const int32_t* cur_rank, const int8_t* best,
                        const int32_t* best_rank, const int64_t* best_step, const int64_t* flips, const int32_t* state) {
  if (!cur) return tg_internal_fail(TG_ERR_INVALID, "%s: null cur", fn);
  if (!cur_rank) return tg_internal_fail(TG_ERR_INVALID, "%s: null cur_rank", fn);
  if (!best) return tg_internal_fail(TG_ERR_INVALID, "%s: null best", fn);
  if (!best_rank) return tg_internal_fail(TG_ERR_INVALID, "%s: null best_rank", fn);
  if (!best_step) return tg_internal_fail(TG_ERR_INVALID, "%s: null best_step", fn);
  if (!flips) return tg_internal_fail(TG_ERR_INVALID, "%s: null flips", fn);
  if (!state) return tg_internal_fail(TG_ERR_INVALID, "%s: null state", fn);
  if (cur == best) return tg_internal_fail(TG_ERR_INVALID, "%s: cur == best: the two lists must be distinct", fn);
  if (!aligned(cur_rank, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: cur_rank not 4-byte aligned", fn);
  if (!aligned(best_rank, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: best_rank not 4-byte aligned", fn);
  if (!aligned(state, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: state not 4-byte aligned", fn);
  if (!aligned(best_step, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: best_step not 8-byte aligned", fn);
  if (!aligned(flips, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: flips not 8-byte aligned", fn);
  return TG_OK;
}

int flip_plus_sizes(const char* fn, int64_t plus_after, int64_t plus_slack) {
  if (plus_after < 1 || plus_after > TG_FLIP_MAX_PLUS_AFTER)
    return tg_internal_fail(TG_ERR_INVALID, "%s: plus_after=%lld outside [1,%d]", fn, (long long)plus_after, TG_FLIP_MAX_PLUS_AFTER);
  if (plus_slack < 0 || plus_slack > TG_FLIP_MAX_K)
    return tg_internal_fail(TG_ERR_INVALID, "%s: plus_slack=%lld outside [0,%d]", fn, (long long)plus_slack, TG_FLIP_MAX_K);
  return TG_OK;
}

// a wavefront per walk: as many workgroups as walks, up to what the device holds a few times over; `args` is what the
// kernel takes (FlipArgs `a` itself, or a struct that holds it)
template <typename Kern, typename Args>
int launch_flip(const char* fn, Kern kernel, const tg::FlipArgs& a, const Args& args, hipStream_t st) {
  const int SW = (a.S + 3) / 4, TS = (3 * SW) | 1;
  const size_t lds = static_cast<size_t>(a.K) * TS * 4 + ((static_cast<size_t>(a.K) + 15) & ~size_t{15});  // <= 12.7 KiB
  return launch_resident(fn, kernel, a.W, 32, 64, lds, st, args);
}

template <typename Kern>
int launch_flip(const char* fn, Kern kernel, const tg::FlipArgs& a, hipStream_t st) {
  return launch_flip(fn, kernel, a, a, st);
}

}  // namespace

extern "C" int tg_flip_check(int64_t M, int64_t W, int K, int S, int shift, int bound, int64_t step0, int64_t n_steps) {
  if (const int rc = flip_sizes("tg_flip_check", M, W, K, S, shift, bound)) return rc;
  return flip_steps("tg_flip_check", step0, n_steps);
}

extern "C" int tg_flip_begin(const int8_t* tokens, const int64_t* lengths, int64_t M, const int64_t* src, int64_t W, int K,
                             int S, int shift, int bound, int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank,
                             int64_t* best_step, int64_t* flips, int32_t* state, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_flip_begin";
  if (const int rc = flip_sizes(fn, M, W, K, S, shift, bound)) return rc;
  if (!src && W != M) return tg_internal_fail(TG_ERR_INVALID, "%s: W=%lld != M=%lld without src", fn, (long long)W, (long long)M);
  if (W == 0) return TG_OK;
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!lengths) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths", fn);
  if (const int rc = flip_state_pointers(fn, cur, cur_rank, best, best_rank, best_step, flips, state)) return rc;
  if (cur == tokens || best == tokens)
    return tg_internal_fail(TG_ERR_INVALID, "%s: cur or best == tokens: in-place operation is not supported", fn);
  if (!aligned(lengths, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: lengths not 8-byte aligned", fn);
  if (!aligned(src, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: src not 8-byte aligned", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const tg::FlipArgs a{tokens, lengths, src, M, W, cur, cur_rank, best, best_rank, best_step, flips, state, status,
                       0, 0, 0, 0, K, S, shift, bound};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_flip(fn, tg::flip_begin_kernel<1>, a, st);
  return launch_flip(fn, tg::flip_begin_kernel<2>, a, st);
}

extern "C" int tg_flip_advance(int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank, int64_t* best_step,
                               int64_t* flips, int32_t* state, int64_t W, int K, int S, int shift, int bound, uint64_t seed,
                               uint64_t walk0, int64_t step0, int64_t n_steps, tg_stream_t stream) {
  const char* fn = "tg_flip_advance";
  if (const int rc = flip_sizes(fn, 0, W, K, S, shift, bound)) return rc;
  if (const int rc = flip_steps(fn, step0, n_steps)) return rc;
  if (W == 0) return TG_OK;
  if (const int rc = flip_state_pointers(fn, cur, cur_rank, best, best_rank, best_step, flips, state)) return rc;
  const tg::FlipArgs a{nullptr, nullptr, nullptr, 0, W, cur, cur_rank, best, best_rank, best_step, flips, state, nullptr,
                       seed, walk0, step0, static_cast<int>(n_steps), K, S, shift, bound};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_flip(fn, tg::flip_advance_kernel<1>, a, st);
  return launch_flip(fn, tg::flip_advance_kernel<2>, a, st);
}

extern "C" int tg_flip_plus_check(int64_t W, int K, int S, int shift, int bound, int64_t step0, int64_t n_steps,
                                  int64_t plus_after, int64_t plus_slack) {
  const char* fn = "tg_flip_plus_check";
  if (const int rc = flip_sizes(fn, 0, W, K, S, shift, bound)) return rc;
  if (const int rc = flip_steps(fn, step0, n_steps)) return rc;
  return flip_plus_sizes(fn, plus_after, plus_slack);
}

extern "C" int tg_flip_advance_plus(int8_t* cur, int32_t* cur_rank, int8_t* best, int32_t* best_rank, int64_t* best_step,
                                    int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses, int64_t W, int K, int S,
                                    int shift, int bound, uint64_t seed, uint64_t walk0, int64_t step0, int64_t n_steps,
                                    int64_t plus_after, int64_t plus_slack, tg_stream_t stream) {
  const char* fn = "tg_flip_advance_plus";
  if (const int rc = flip_sizes(fn, 0, W, K, S, shift, bound)) return rc;
  if (const int rc = flip_steps(fn, step0, n_steps)) return rc;
  if (const int rc = flip_plus_sizes(fn, plus_after, plus_slack)) return rc;
  if (W == 0) return TG_OK;
  if (const int rc = flip_state_pointers(fn, cur, cur_rank, best, best_rank, best_step, flips, state)) return rc;
  if (!since) return tg_internal_fail(TG_ERR_INVALID, "%s: null since", fn);
  if (!pluses) return tg_internal_fail(TG_ERR_INVALID, "%s: null pluses", fn);
  if (!aligned(since, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: since not 4-byte aligned", fn);
  if (!aligned(pluses, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: pluses not 8-byte aligned", fn);
  const tg::FlipArgs a{nullptr, nullptr, nullptr, 0, W, cur, cur_rank, best, best_rank, best_step, flips, state, nullptr,
                       seed, walk0, step0, static_cast<int>(n_steps), K, S, shift, bound};
  const tg::FlipPlusArgs pa{a, since, pluses, static_cast<int>(plus_after), static_cast<int>(plus_slack)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_flip(fn, tg::flip_advance_plus_kernel<1>, a, pa, st);
  return launch_flip(fn, tg::flip_advance_plus_kernel<2>, a, pa, st);
}
