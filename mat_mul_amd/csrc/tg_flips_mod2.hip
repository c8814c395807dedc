// Flip-graph walks over Z_2 and their proof (include/tensor_game_flips_mod2.h).  gfx950 only; part of libtensorgame.so.
//
// Over Z_2 a factor of S <= 32 values is one dword, so a walk's whole list fits in its wavefront's registers: ONE
// wavefront (a 64-thread workgroup of its own) per walk, lane l owning terms l and l + 64, as in tg_flips.hip -- but
//   list    in VGPRs: 3 x NW dwords per lane.  No LDS, no __syncthreads(): the only traffic between lanes is v_readlane
//           of a uniform slot, ballots and the prefix sum's shuffles.
//   same    n_d(t) == n_d(p) is the lane's own word against a v_readlane of slot p's word (p is wavefront-uniform).
//   masks   per owned term and mode, a K-bit mask of the terms that share that word (tg_flips.hip's eq): per changed slot
//           3 x NW compares and ballots; the K^2 compares are done once per launch.
//   matches C = the popcounts of the masks above the diagonal, summed by a wavefront prefix sum; the lane whose prefix
//           interval holds the drawn number walks its own masks in (j, d) order to the match.
//   reduce  the first pair in (i, j) order whose masks agree in two modes merges or cancels, until there is none: over
//           Z_2 no pair is ever passed over, so this is the header's full scan.
//   draws   Philox for 64 consecutive steps at a time, one step per lane.
//   memory  a list is read once and written once per launch as 12-byte rows, lane after lane; best only when the rank
//           falls.
// Registers are indexed by compile-time constants only (a slot or mode known at run time selects among them), so
// nothing goes to scratch.  Every loop is bounded by n_steps, K, S or the number of walks.  No floating point, no
// atomics but the OR of the sticky bad-row bits.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_flips_mod2.h"
#include "tg_lists.h"

namespace tg {

struct Flip2Args {
  const int8_t* tokens;    // begin: (M, K, 3S)
  const int64_t* lengths;  // begin: (M)
  const int64_t* src;      // begin: (W) or null
  int64_t M, W;
  int32_t* cur;            // (W, K, 3)
  int32_t* cur_rank;
  int32_t* best;
  int32_t* best_rank;
  int64_t* best_step;
  int64_t* flips;
  int32_t* state;
  int32_t* since;
  int64_t* pluses;
  uint32_t* status;        // begin: or null
  uint64_t seed, walk0;
  int64_t step0;
  int n_steps;
  int K, S, shift;
  int plus_after, plus_slack;
};

__device__ __forceinline__ uint64_t above2(int t, int w) {  // of word w: the bits of the terms > t
  const int r = t - 64 * w;
  return r < 0 ? ~0ull : r >= 63 ? 0ull : (~0ull << (r + 1));
}
__device__ __forceinline__ uint64_t below2(int n, int w) {  // of word w: the bits of the terms < n
  const int r = n - 64 * w;
  return r <= 0 ? 0ull : r >= 64 ? ~0ull : ((1ull << r) - 1);
}
// (readfirstlane and readlane return a SIGNED int: through uint32_t before anything widens them)
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), l));
}
__device__ __forceinline__ uint64_t lane_of64(uint64_t v, int l) {
  return (static_cast<uint64_t>(lane_of(static_cast<uint32_t>(v >> 32), l)) << 32) | lane_of(static_cast<uint32_t>(v), l);
}

// NW = 64-bit words per mask = terms per lane: 1 while K <= 64, 2 up to TG_FLIP_MAX_K
template <int NW>
struct Walk2 {
  uint32_t m[NW][3];       // my terms lane + 64 s: the three masks
  uint64_t eq[NW][3][NW];  // eq[s][d][w]: word w of the terms that share m_d with my term lane + 64 s
  int K, L, lane;

  // m_d of slot p (both uniform)
  __device__ __forceinline__ uint32_t word(int p, int d) const {
    uint32_t v = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s)
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (s == (p >> 6) && x == d) v = m[s][x];
    return lane_of(v, p & 63);
  }

  __device__ __forceinline__ void put(int p, int d, uint32_t v) {
#pragma unroll
    for (int s = 0; s < NW; ++s)
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (s == (p >> 6) && x == d && lane == (p & 63)) m[s][x] = v;
  }

  // term p (uniform, < L) has changed or is new in its slot: bit p of every mask, and the masks of term p
  __device__ __forceinline__ void refresh(int p) {
    const int ps = p >> 6, pl = p & 63;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const uint32_t wp = word(p, d);
#pragma unroll
      for (int s = 0; s < NW; ++s) {
        const bool e = lane + 64 * s < L && m[s][d] == wp;
        const uint64_t b = __ballot(e);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          if (w == ps) eq[s][d][w] = (eq[s][d][w] & ~(1ull << pl)) | (static_cast<uint64_t>(e) << pl);
          if (w == ps && lane == pl) eq[w][d][s] = b;
        }
      }
    }
  }

  __device__ __forceinline__ void refresh_all() {
#pragma unroll
    for (int s = 0; s < NW; ++s)
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int w = 0; w < NW; ++w) eq[s][d][w] = 0;
    for (int p = 0; p < L; ++p) refresh(p);
  }

  // Removing slot p (uniform): the last live term moves into it.
  __device__ __forceinline__ void remove(int p) {
    const int last = L - 1;
    if (p != last) {
#pragma unroll
      for (int d = 0; d < 3; ++d) put(p, d, word(last, d));
    }
    L = last;
    if (p != last) refresh(p);
  }

  // the pair (i < j, uniform) agrees in two modes: it cancels or merges
  __device__ __forceinline__ void merge(int i, int j) {
    const uint32_t x0 = word(i, 0) ^ word(j, 0), x1 = word(i, 1) ^ word(j, 1), x2 = word(i, 2) ^ word(j, 2);
    if ((x0 | x1 | x2) == 0) {
      remove(j);
      remove(i);
      return;
    }
    const int d = x0 ? 0 : x1 ? 1 : 2;
    put(i, d, word(i, d) ^ word(j, d));
    remove(j);
    refresh(i);
  }

  __device__ __forceinline__ void reduce() {
    for (int pass = 0; pass <= K; ++pass) {  // every pass but the last lowers L
      int i = -1, j = -1;
#pragma unroll
      for (int s = 0; s < NW; ++s) {
        if (i < 0) {
          const int t = lane + 64 * s;
          uint64_t cand[NW], any = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) {
            const uint64_t e0 = eq[s][0][w], e1 = eq[s][1][w], e2 = eq[s][2][w];
            cand[w] = t < L ? ((e0 & e1) | (e0 & e2) | (e1 & e2)) & above2(t, w) & below2(L, w) : 0ull;
            any |= cand[w];
          }
          const uint64_t has = __ballot(any != 0);
          if (has != 0) {  // the lowest term i of this slot that has a partner, and its lowest partner j
            const int il = static_cast<int>(__builtin_ctzll(has));
            i = il + 64 * s;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
              const uint64_t cw = lane_of64(cand[w], il);
              if (j < 0 && cw != 0) j = 64 * w + static_cast<int>(__builtin_ctzll(cw));
            }
          }
        }
      }
      if (i < 0) return;
      merge(i, j);
    }
  }

  // my matches (i = my terms, j > i), per slot
  __device__ __forceinline__ int count(int s) const {
    const int t = lane + 64 * s;
    int c = 0;
    if (t < L) {
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int w = 0; w < NW; ++w) c += __popcll(eq[s][d][w] & above2(t, w) & below2(L, w));
    }
    return c;
  }

  // the kk-th match of my term of slot s in (j, d) order, as j * 4 + d
  __device__ __forceinline__ int locate(int s, int kk) const {
    const int t = lane + 64 * s;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const uint64_t keep = above2(t, w) & below2(L, w);
      const uint64_t a0 = eq[s][0][w] & keep, a1 = eq[s][1][w] & keep, a2 = eq[s][2][w] & keep;
      uint64_t un = a0 | a1 | a2;
      while (un != 0) {
        const int b = static_cast<int>(__builtin_ctzll(un));
        un &= un - 1;
        const int h0 = (a0 >> b) & 1, h1 = (a1 >> b) & 1, h2 = (a2 >> b) & 1;
        const int n = h0 + h1 + h2;
        if (kk < n) {
          const int d = kk == 0 ? (h0 ? 0 : h1 ? 1 : 2) : kk == 1 ? (h0 && h1 ? 1 : 2) : 2;
          return (64 * w + b) * 4 + d;
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

  // number k of the items of which term lane + 64 s owns own[s]: its term and its index among that term's items
  __device__ __forceinline__ void find(const int (&own)[NW], const int (&inc)[NW], const int (&tot)[NW], int k, int& i,
                                       int& within) const {
    i = 0;
    within = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      if (k >= 0 && k < tot[s]) {
        const int il = static_cast<int>(__builtin_ctzll(__ballot(inc[s] > k)));
        within = k - static_cast<int>(lane_of(static_cast<uint32_t>(inc[s] - own[s]), il));
        i = il + 64 * s;
        k = -1;
      } else if (k >= 0) {
        k -= tot[s];
      }
    }
  }

  // step 1: the number of matches (cnt, inc, tot: per slot, for flip)
  __device__ __forceinline__ int matches(int (&cnt)[NW], int (&inc)[NW], int (&tot)[NW]) const {
    int C = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      cnt[s] = count(s);
      inc[s] = scan(cnt[s]);
      tot[s] = static_cast<int>(lane_of(static_cast<uint32_t>(inc[s]), 63));
      C += tot[s];
    }
    return C;
  }

  // slots hi > lo were written (null: the term there is null), and slot `fresh` (or -1) was appended: the removals, the
  // higher slot first, and the masks of what stayed
  __device__ __forceinline__ void settle(int a, bool null_a, int b, bool null_b, int fresh) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const bool null_hi = a > b ? null_a : null_b, null_lo = a > b ? null_b : null_a;
    if (null_hi) remove(hi);  // the last term moves in and is refreshed there
    if (null_lo) remove(lo);
    if (fresh >= 0 && fresh < L) refresh(fresh);  // bit `fresh` of every mask: nothing of an earlier tenant stays
    if (!null_hi && hi < L) refresh(hi);          // (hi >= L: it was the last term and has moved into lo)
    if (!null_lo && lo < L) refresh(lo);
    reduce();
  }

  // step 4 with the draw ox, C > 0
  __device__ __forceinline__ void flip(uint32_t ox, int C, const int (&cnt)[NW], const int (&inc)[NW], const int (&tot)[NW]) {
    const uint32_t c = static_cast<uint32_t>((static_cast<uint64_t>(ox) * (4u * static_cast<uint32_t>(C))) >> 32);
    int i, within;
    find(cnt, inc, tot, static_cast<int>(c >> 2), i, within);
    int found = 0;
#pragma unroll
    for (int s = 0; s < NW; ++s)
      if (s == (i >> 6) && lane == (i & 63)) found = locate(s, within);
    const int jd = static_cast<int>(lane_of(static_cast<uint32_t>(found), i & 63));
    const int j = jd >> 2, d = jd & 3;
    int q = d == 0 ? 1 : 0, r = d == 2 ? 1 : 2;
    if (c & 1) { const int x = q; q = r; r = x; }
    const int a = (c & 2) ? j : i, b = (c & 2) ? i : j;
    const uint32_t nq = word(a, q) ^ word(b, q), nr = word(b, r) ^ word(a, r);
    put(a, q, nq);  // a' = x, nq, m_r(a);  b' = x, m_q(b), nr
    put(b, r, nr);
    settle(a, nq == 0, b, nr == 0, -1);
  }

  // step 5 with the draws oy, oz; needs 2 <= L < K
  __device__ __forceinline__ void plus(uint32_t oy, uint32_t oz) {
    const uint32_t P = static_cast<uint32_t>(L * (L - 1) / 2);
    const int k = static_cast<int>((static_cast<uint64_t>(oy) * P) >> 32);
    const int v = static_cast<int>((static_cast<uint64_t>(oz) * 12u) >> 32);
    int own[NW], inc[NW], tot[NW];  // term t owns the L - 1 - t pairs (t, j > t)
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int t = lane + 64 * s;
      own[s] = t < L - 1 ? L - 1 - t : 0;
      inc[s] = scan(own[s]);
      tot[s] = static_cast<int>(lane_of(static_cast<uint32_t>(inc[s]), 63));
    }
    int i, within;
    find(own, inc, tot, k, i, within);
    const int j = i + 1 + within;
    const int a = (v & 1) ? j : i, b = (v & 1) ? i : j;
    const int perm = v >> 1;  // 012, 021, 102, 120, 201, 210
    const int p = perm >> 1, q = perm == 0 || perm == 5 ? 1 : perm == 1 || perm == 3 ? 2 : 0, r = 3 - p - q;
    const uint32_t ap = word(a, p), aq = word(a, q), ar = word(a, r);
    const uint32_t bp = word(b, p), bq = word(b, q), br = word(b, r);
    const int n = L;
    put(a, p, ap ^ bp);  // t1 = ap ^ bp, aq, ar
    put(b, q, bq ^ aq);  // t3 = bp, bq ^ aq, br
    const bool null2 = ar == br;  // t2 = bp, aq, ar ^ br: a null one would be removed first, from the last slot
    if (!null2) {
      put(n, p, bp);
      put(n, q, aq);
      put(n, r, ar ^ br);
      L = n + 1;
    }
    settle(a, ap == bp, b, aq == bq, null2 ? -1 : n);
  }

  // ---- global <-> registers: 12-byte rows, lane after lane
  __device__ __forceinline__ void load(const int32_t* rows, int n) {
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int t = lane + 64 * s;
#pragma unroll
      for (int d = 0; d < 3; ++d) m[s][d] = t < n ? static_cast<uint32_t>(rows[t * 3 + d]) : 0u;
    }
    L = n;
  }

  // zero rows at and beyond n_live
  __device__ __forceinline__ void store(int32_t* rows, int n_live) const {
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int t = lane + 64 * s;
      if (t < K) {
#pragma unroll
        for (int d = 0; d < 3; ++d) rows[t * 3 + d] = t < n_live ? static_cast<int32_t>(m[s][d]) : 0;
      }
    }
  }
};

template <int NW>
__global__ __launch_bounds__(64) void flip2_begin_kernel(Flip2Args a) {
  Walk2<NW> wk;
  wk.K = a.K;
  wk.lane = threadIdx.x;
#pragma unroll
  for (int s = 0; s < NW; ++s)
#pragma unroll
    for (int d = 0; d < 3; ++d) wk.m[s][d] = 0;
  const int A3 = 3 * a.S;
  const int64_t n_tok = static_cast<int64_t>(a.K) * A3, n_row = static_cast<int64_t>(a.K) * 3;
  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    uint32_t bad = 0;
    const int64_t src = a.src ? a.src[w] : w;
    int64_t L0 = 0;
    if (src < 0 || src >= a.M) {  // checked before it addresses anything
      bad = TG_FLIP_BAD_SRC;
    } else {
      L0 = a.lengths[src];
      if (L0 < 0 || L0 > a.K) bad = TG_FLIP_BAD_LENGTH;
    }
    wk.L = 0;
    if (!bad) {
      const int n = uni(static_cast<int>(L0));
      const int8_t* rows = a.tokens + src * n_tok;
      uint64_t live[NW];
#pragma unroll
      for (int s = 0; s < NW; ++s) {
        const int t = wk.lane + 64 * s;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          uint32_t mask = 0;
          if (t < n)
            for (int e = 0; e < a.S; ++e) mask |= static_cast<uint32_t>((rows[t * A3 + d * a.S + e] ^ a.shift) & 1) << e;
          wk.m[s][d] = mask;
        }
        live[s] = __ballot(wk.m[s][0] != 0 && wk.m[s][1] != 0 && wk.m[s][2] != 0);
      }
      int dst = 0;  // drop the null terms, the others keep their order (dst <= t: nothing unread is overwritten)
      for (int t = 0; t < n; ++t) {
        uint64_t lw = live[0];
#pragma unroll
        for (int s = 1; s < NW; ++s)
          if (s == (t >> 6)) lw = live[s];
        if (((lw >> (t & 63)) & 1) == 0) continue;
        if (dst != t) {
#pragma unroll
          for (int d = 0; d < 3; ++d) wk.put(dst, d, wk.word(t, d));
        }
        ++dst;
      }
      wk.L = dst;
      wk.refresh_all();
      wk.reduce();
    }
    const int rank = wk.L;
    wk.store(a.cur + w * n_row, rank);
    wk.store(a.best + w * n_row, rank);
    if (wk.lane == 0) {
      a.cur_rank[w] = rank;
      a.best_rank[w] = rank;
      a.best_step[w] = 0;
      a.flips[w] = 0;
      a.state[w] = bad ? -1 : 0;
      a.since[w] = 0;
      a.pluses[w] = 0;
      if (bad && a.status) atomicOr(a.status, bad);
    }
  }
}

template <int NW>
__global__ __launch_bounds__(64) void flip2_advance_kernel(Flip2Args a) {
  Walk2<NW> wk;
  wk.K = a.K;
  wk.lane = threadIdx.x;
  const int64_t n_row = static_cast<int64_t>(a.K) * 3;
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);
  for (int64_t w = blockIdx.x; w < a.W; w += gridDim.x) {
    const int L0 = a.cur_rank[w];
    if (a.state[w] != 0 || L0 < 0 || L0 > a.K) continue;  // left exactly as it is (uniform)
    const uint64_t g = a.walk0 + static_cast<uint64_t>(w);
    wk.load(a.cur + w * n_row, uni(L0));
    wk.refresh_all();
    int best = uni(a.best_rank[w]);
    int since = uni(a.since[w]);
    int64_t flipped = 0, plused = 0;
    int stuck = 0;
    U4 o64{0, 0, 0, 0};
    for (int k = 0; k < a.n_steps; ++k) {
      if ((k & 63) == 0) {  // the draws of steps k .. k + 63, one per lane
        const uint32_t t = static_cast<uint32_t>(static_cast<uint64_t>(a.step0) + static_cast<uint64_t>(k + wk.lane));
        o64 = philox4x32_10(U4{static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), t, TG_FLIP2_DOMAIN}, k0, k1);
      }
      int cnt[NW], inc[NW], tot[NW];
      const int C = wk.matches(cnt, inc, tot);
      const int before = wk.L;
      const int64_t cap64 = static_cast<int64_t>(best) + a.plus_slack;
      const bool can = before >= 2 && before < (cap64 < a.K ? cap64 : a.K);
      const bool want = a.plus_after > 0 && (C == 0 || since >= a.plus_after);
      if (want && can) {
        wk.plus(lane_of(o64.y, k & 63), lane_of(o64.z, k & 63));
        ++plused;
        since = 0;
      } else if (C == 0) {
        stuck = 1;
        break;
      } else {
        wk.flip(lane_of(o64.x, k & 63), C, cnt, inc, tot);
        ++flipped;
        since = wk.L < before ? 0 : since == INT32_MAX ? since : since + 1;
      }
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
      a.flips[w] += flipped;
      a.since[w] = since;
      a.pluses[w] += plused;
      if (stuck) a.state[w] = 1;
    }
  }
}

struct Flip2ResidualArgs {
  const int8_t* targets;  // (M, S, S, S)
  const int32_t* lists;   // (M, K, 3)
  const int32_t* ranks;   // (M)
  int32_t* residual;      // (M)
  int64_t M;
  int K, S;
};

constexpr int kFlip2Cells = TG_MAX_S * TG_MAX_S / 64;  // (i, j) cells per lane

// A wavefront per list: lane l owns the cells (i, j) = l, l + 64, ... of the S x S front face, each a dword over k; a
// term whose m_0 has bit i and whose m_1 has bit j XORs its m_2 into it.
__global__ __launch_bounds__(64) void flip2_residual_kernel(Flip2ResidualArgs a) {
  const int lane = threadIdx.x, SS = a.S * a.S;
  uint32_t im[kFlip2Cells], jm[kFlip2Cells];  // bit i and bit j of my cells; 0 beyond the face
#pragma unroll
  for (int c = 0; c < kFlip2Cells; ++c) {
    const int cell = lane + 64 * c, i = cell / a.S, j = cell - i * a.S;
    im[c] = cell < SS ? 1u << i : 0u;
    jm[c] = cell < SS ? 1u << j : 0u;
  }
  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    const int rank = uni(a.ranks[m]);
    if (rank < 0 || rank > a.K) {  // checked before it addresses anything
      if (lane == 0) a.residual[m] = -1;
      continue;
    }
    const int32_t* rows = a.lists + m * a.K * 3;
    uint32_t acc[kFlip2Cells];
#pragma unroll
    for (int c = 0; c < kFlip2Cells; ++c) acc[c] = 0;
    for (int base = 0; base < rank; base += 64) {
      const int t = base + lane, n = rank - base < 64 ? rank - base : 64;
      const uint32_t w0 = t < rank ? static_cast<uint32_t>(rows[t * 3]) : 0u;
      const uint32_t w1 = t < rank ? static_cast<uint32_t>(rows[t * 3 + 1]) : 0u;
      const uint32_t w2 = t < rank ? static_cast<uint32_t>(rows[t * 3 + 2]) : 0u;
      for (int u = 0; u < n; ++u) {
        const uint32_t m0 = lane_of(w0, u), m1 = lane_of(w1, u), m2 = lane_of(w2, u);
#pragma unroll
        for (int c = 0; c < kFlip2Cells; ++c)
          if (64 * c < SS) acc[c] ^= (m0 & im[c]) != 0 && (m1 & jm[c]) != 0 ? m2 : 0u;
      }
    }
    const int8_t* target = a.targets + m * SS * a.S;
    int diff = 0;
#pragma unroll
    for (int c = 0; c < kFlip2Cells; ++c) {
      const int cell = lane + 64 * c;
      if (cell < SS)
        for (int k = 0; k < a.S; ++k) diff += static_cast<int>(((acc[c] >> k) ^ static_cast<uint32_t>(target[cell * a.S + k])) & 1u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) diff += __shfl_xor(diff, d);
    if (lane == 0) a.residual[m] = diff;
  }
}

}  // namespace tg

namespace {

int flip2_sizes(const char* fn, int64_t M, int64_t W, int K, int S, int shift) {
  if (const int rc = check_lists(fn, K, S, shift, TG_FLIP_MAX_K)) return rc;
  const int64_t most = INT64_MAX / (static_cast<int64_t>(TG_FLIP_MAX_K) * 3 * TG_MAX_S * TG_MAX_S);
  if (M < 0 || M > most) return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M);
  if (W < 0 || W > most) return tg_internal_fail(TG_ERR_INVALID, "%s: W=%lld out of range", fn, (long long)W);
  return TG_OK;
}

int flip2_steps(const char* fn, int64_t step0, int64_t n_steps, int64_t plus_after, int64_t plus_slack) {
  if (n_steps < 1 || n_steps > TG_FLIP_MAX_STEPS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_steps=%lld outside [1,%d]", fn, (long long)n_steps, TG_FLIP_MAX_STEPS);
  if (step0 < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: step0=%lld < 0", fn, (long long)step0);
  if (step0 > (int64_t{1} << 32) || step0 + n_steps > (int64_t{1} << 32))
    return tg_internal_fail(TG_ERR_INVALID, "%s: step0 + n_steps=%llu beyond 2^32", fn,
                            (unsigned long long)(static_cast<uint64_t>(step0) + static_cast<uint64_t>(n_steps)));
  if (plus_after < 0 || plus_after > TG_FLIP2_MAX_PLUS_AFTER)
    return tg_internal_fail(TG_ERR_INVALID, "%s: plus_after=%lld outside [0,%d]", fn, (long long)plus_after, TG_FLIP2_MAX_PLUS_AFTER);
  if (plus_slack < 0 || plus_slack > TG_FLIP_MAX_K)
    return tg_internal_fail(TG_ERR_INVALID, "%s: plus_slack=%lld outside [0,%d]", fn, (long long)plus_slack, TG_FLIP_MAX_K);
  return TG_OK;
}

int flip2_state_pointers(const char* fn, const int32_t* cur, const int32_t* cur_rank, const int32_t* best,
                         const int32_t* best_rank, const int64_t* best_step, const int64_t* flips, const int32_t* state,
                         const int32_t* since, const int64_t* pluses) {
  const struct { const void* p; const char* name; int align; } all[] = {
      {cur, "cur", 4}, {cur_rank, "cur_rank", 4}, {best, "best", 4}, {best_rank, "best_rank", 4}, {best_step, "best_step", 8},
      {flips, "flips", 8}, {state, "state", 4}, {since, "since", 4}, {pluses, "pluses", 8}};
  for (const auto& x : all)
    if (!x.p) return tg_internal_fail(TG_ERR_INVALID, "%s: null %s", fn, x.name);
  if (cur == best) return tg_internal_fail(TG_ERR_INVALID, "%s: cur == best: the two lists must be distinct", fn);
  for (const auto& x : all)
    if (!aligned(x.p, x.align)) return tg_internal_fail(TG_ERR_INVALID, "%s: %s not %d-byte aligned", fn, x.name, x.align);
  return TG_OK;
}

// a wavefront per walk or list: as many workgroups as there is work, up to what the device holds a few times over
template <typename Kern, typename Args>
int launch_flip2(const char* fn, Kern kernel, int64_t work, const Args& a, hipStream_t st) {
  return launch_resident(fn, kernel, work, 32, 64, 0, st, a);
}

}  // namespace

extern "C" int tg_flip2_check(int64_t M, int64_t W, int K, int S, int shift, int64_t step0, int64_t n_steps,
                              int64_t plus_after, int64_t plus_slack) {
  if (const int rc = flip2_sizes("tg_flip2_check", M, W, K, S, shift)) return rc;
  return flip2_steps("tg_flip2_check", step0, n_steps, plus_after, plus_slack);
}

extern "C" int tg_flip2_begin(const int8_t* tokens, const int64_t* lengths, int64_t M, const int64_t* src, int64_t W, int K,
                              int S, int shift, int32_t* cur, int32_t* cur_rank, int32_t* best, int32_t* best_rank,
                              int64_t* best_step, int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses,
                              uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_flip2_begin";
  if (const int rc = flip2_sizes(fn, M, W, K, S, shift)) return rc;
  if (!src && W != M) return tg_internal_fail(TG_ERR_INVALID, "%s: W=%lld != M=%lld without src", fn, (long long)W, (long long)M);
  if (W == 0) return TG_OK;
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!lengths) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths", fn);
  if (const int rc = flip2_state_pointers(fn, cur, cur_rank, best, best_rank, best_step, flips, state, since, pluses)) return rc;
  if (!aligned(lengths, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: lengths not 8-byte aligned", fn);
  if (!aligned(src, 8)) return tg_internal_fail(TG_ERR_INVALID, "%s: src not 8-byte aligned", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const tg::Flip2Args a{tokens, lengths, src, M, W, cur, cur_rank, best, best_rank, best_step, flips, state, since, pluses,
                        status, 0, 0, 0, 0, K, S, shift, 0, 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_flip2(fn, tg::flip2_begin_kernel<1>, W, a, st);
  return launch_flip2(fn, tg::flip2_begin_kernel<2>, W, a, st);
}

extern "C" int tg_flip2_advance(int32_t* cur, int32_t* cur_rank, int32_t* best, int32_t* best_rank, int64_t* best_step,
                                int64_t* flips, int32_t* state, int32_t* since, int64_t* pluses, int64_t W, int K, int S,
                                uint64_t seed, uint64_t walk0, int64_t step0, int64_t n_steps, int64_t plus_after,
                                int64_t plus_slack, tg_stream_t stream) {
  const char* fn = "tg_flip2_advance";
  if (const int rc = flip2_sizes(fn, 0, W, K, S, 0)) return rc;
  if (const int rc = flip2_steps(fn, step0, n_steps, plus_after, plus_slack)) return rc;
  if (W == 0) return TG_OK;
  if (const int rc = flip2_state_pointers(fn, cur, cur_rank, best, best_rank, best_step, flips, state, since, pluses)) return rc;
  const tg::Flip2Args a{nullptr, nullptr, nullptr, 0, W, cur, cur_rank, best, best_rank, best_step, flips, state, since,
                        pluses, nullptr, seed, walk0, step0, static_cast<int>(n_steps), K, S, 0,
                        static_cast<int>(plus_after), static_cast<int>(plus_slack)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K <= 64) return launch_flip2(fn, tg::flip2_advance_kernel<1>, W, a, st);
  return launch_flip2(fn, tg::flip2_advance_kernel<2>, W, a, st);
}

extern "C" int tg_flip2_residual(const int8_t* targets, const int32_t* lists, const int32_t* ranks, int64_t M, int K, int S,
                                 int32_t* residual, tg_stream_t stream) {
  const char* fn = "tg_flip2_residual";
  if (const int rc = flip2_sizes(fn, M, 0, K, S, 0)) return rc;
  if (M == 0) return TG_OK;
  if (!targets) return tg_internal_fail(TG_ERR_INVALID, "%s: null targets", fn);
  if (!lists) return tg_internal_fail(TG_ERR_INVALID, "%s: null lists", fn);
  if (!ranks) return tg_internal_fail(TG_ERR_INVALID, "%s: null ranks", fn);
  if (!residual) return tg_internal_fail(TG_ERR_INVALID, "%s: null residual", fn);
  if (!aligned(lists, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: lists not 4-byte aligned", fn);
  if (!aligned(ranks, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: ranks not 4-byte aligned", fn);
  if (!aligned(residual, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: residual not 4-byte aligned", fn);
  const tg::Flip2ResidualArgs a{targets, lists, ranks, residual, M, K, S};
  return launch_flip2(fn, tg::flip2_residual_kernel, M, a, static_cast<hipStream_t>(stream));
}
