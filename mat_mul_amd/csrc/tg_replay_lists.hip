// Move lists of the solution search, replayed and stored as games of a replay ring
// (include/tensor_game_replay_lists.h).  gfx950 only; part of libtensorgame.so.
//
// tg_replay_add_lists: four launches with `stored`, three without, no host sync.
//   - lists_valid_kernel (one workgroup per list): checks the length and the group, then replays the list ROW BY ROW: a
//     thread takes rows (i, j, 0 .. S-1) of the tensor and runs the L moves on that one row in registers, so nothing is
//     stored and no barrier is needed until the flags are combined; writes stored[m] and ORs the status bits;
//   - lists_plan_kernel (one workgroup of 1024): the plan of the ring protocol (tg_ring.h) over the valid lists (select
//     0) or the first shortest one (select 1); the parked index is the list's; with select 1 stored[] is cut down to
//     the winner.  Without `stored` the plan calls the validity replay itself, one thread per list;
//   - lists_emit_kernel (one workgroup per stored game and per kEmitChunk entries of the tensor -- the entries are
//     independent of each other, and a game alone is too little work for a CU): its entries of the game's frames as below;
//     the first workgroup of a game also writes its tokens and rewards;
//   - the rebuild of offset (tg_internal_ring_rebuild).
//
// The emit kernel loads its entries of the T frames of the start state into LDS, as bytes, and walks s = -(T-1) .. L-1:
// for s <= 0 the tensor is frame -s of the start state, for s > 0 it is head_s = head_{s-1} - u (x) v (x) w, frame 0
// updated in place.  Tensor s is frame f of move s + f for every f < T with 0 <= s + f < L, so it is stored up to T times
// and then forgotten: every head is computed once, and no history is shifted along.  A destination frame starts at ((slot L + t) T + f) S^3 bytes, which at odd S^3 (S = 5, 9,
// 25) is aligned to nothing, so the access width is chosen per stored frame from the destination alone: bytes up to the
// first 16-byte boundary, then 16-byte stores whose four dwords are funnel-shifted out of five aligned LDS dwords, then
// a byte tail.  The barriers inside the walk are lds_barrier (tg_device.h): the frames streamed out are never read back.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_replay_lists.h"
#include "tg_host.h"
#include "tg_ring.h"

namespace tg {
namespace rl {

constexpr int kSmallBlock = 64;  // one wavefront per list or game while S^3 <= kSmallEntries
constexpr int kSmallEntries = 1024;
constexpr int kValidBlock = 1024;  // per list above kSmallEntries: the replay is latency bound, one workgroup per list
constexpr int kEmitChunk = 2048;   // entries of the tensor per emit workgroup above kSmallEntries (a multiple of 16)
constexpr int kTokenTile = 32;     // moves whose tokens the emit kernel fetches into LDS at once

struct ListArgs {
  tg_replay_buffer b;
  const int8_t* starts;    // (G,T,S^3)
  const int64_t* groups;   // (M) or NULL
  const int8_t* tokens;    // (M,K,3S)
  const int64_t* lengths;  // (M)
  int64_t G, M;
  int K, shift, select;
  uint8_t* stored;   // (M) or NULL
  uint32_t* status;  // (1) or NULL
};

// The status bits list m earns on the rows tid, tid + nthr, ... of its tensor (the length and group bits on every
// thread).  The length and the group are checked before they address anything; a list that fails either is not
// replayed.  A thread owns a row (i, j, 0 .. S-1) in registers and runs the L moves on it: per move it loads u[i] and
// v[j]; with kWave (every thread of a wavefront works on the same list, all of them active) lane k loads w[k] once and
// the row reads it from there, else the thread loads the S factors itself.
template <bool kWave>
__device__ __forceinline__ uint32_t list_flags(const ListArgs& p, int64_t m, int tid, int nthr) {
  const int64_t len = p.lengths[m];
  const int64_t g = p.groups ? p.groups[m] : m;
  uint32_t f = 0;
  if (len < 1 || len > p.K || len > p.b.L) f |= TG_REPLAY_LISTS_BAD_LENGTH;
  if (g < 0 || g >= p.G) f |= TG_REPLAY_LISTS_BAD_GROUP;
  if (f) return f;
  const int S = p.b.S, S2 = S * S, A3 = 3 * S, L = static_cast<int>(len), lane = tid & 63;
  const int8_t* tk = p.tokens + m * p.K * A3;
  const int8_t* st = p.starts + g * p.b.T * S2 * S;  // frame 0
  for (int base = 0; base < S2; base += nthr) {      // uniform over the workgroup: no lane leaves before the last row
    const bool on = base + tid < S2;
    const int row = on ? base + tid : S2 - 1, i = row / S, j = row - i * S;
    uint32_t h[TG_MAX_S];  // unsigned: the 32-bit wrap is defined
#pragma unroll
    for (int k = 0; k < TG_MAX_S; ++k) h[k] = k < S ? static_cast<uint32_t>(static_cast<int32_t>(st[row * S + k])) : 0;
    uint32_t out = 0;
    for (int t = 0; t < L; ++t) {
      const int8_t* a = tk + t * A3;
      const int32_t uv = (a[i] - p.shift) * (a[S + j] - p.shift);
      const int32_t wl = kWave ? a[2 * S + (lane < S ? lane : 0)] - p.shift : 0;
#pragma unroll
      for (int k = 0; k < TG_MAX_S; ++k) {
        if (k < S) {  // (no break: the loop must unroll for h to stay in registers)
          const int32_t w = kWave ? __builtin_amdgcn_readlane(wl, k) : a[2 * S + k] - p.shift;
          h[k] -= static_cast<uint32_t>(uv * w);  // |u v w| <= 192^3
          out |= h[k] + 128u > 255u;  // outside [-128,127]
        }
      }
    }
    uint32_t left = 0;
#pragma unroll
    for (int k = 0; k < TG_MAX_S; ++k) left |= h[k];
    if (on && out) f |= TG_REPLAY_LISTS_BAD_RANGE;
    if (on && left) f |= TG_REPLAY_LISTS_NOT_ZERO;
  }
  return f;
}

__global__ __launch_bounds__(kValidBlock) void lists_valid_kernel(ListArgs p) {
  __shared__ uint32_t all;
  const int t = threadIdx.x;
  for (int64_t m = blockIdx.x; m < p.M; m += gridDim.x) {
    if (t == 0) all = 0;
    __syncthreads();
    const uint32_t f = list_flags<true>(p, m, t, blockDim.x);
    if (f) atomicOr(&all, f);
    __syncthreads();
    if (t == 0) {
      p.stored[m] = all == 0;
      if (all && p.status) atomicOr(p.status, all);
    }
    __syncthreads();  // `all` is read before the next list clears it
  }
}

// whether list m is valid: what the validity kernel left in stored[m], or, without it, the replay by this thread alone
__device__ __forceinline__ bool list_valid(const ListArgs& p, int64_t m, uint32_t* flags) {
  if (p.stored) return p.stored[m] != 0;
  const uint32_t f = list_flags<false>(p, m, 0, 1);
  *flags |= f;
  return f == 0;
}

__global__ __launch_bounds__(kRingScanBlock) void lists_plan_kernel(ListArgs p) {
  __shared__ int64_t sh[kRingScanBlock];
  __shared__ int64_t best_l[kRingScanBlock];
  __shared__ int64_t best_m[kRingScanBlock];
  const int t = threadIdx.x;
  const int64_t next = ring_next(p.b);
  int64_t cnt = 0, bl = 0, bm = -1;
  uint32_t flags = 0;
  for (int64_t m = t; m < p.M; m += kRingScanBlock) {
    if (!list_valid(p, m, &flags)) continue;
    ++cnt;
    const int64_t len = p.lengths[m];
    if (bm < 0 || len < bl) bl = len, bm = m;  // within a thread m rises: the first shortest stays
  }
  if (!p.stored) {  // the bits the validity kernel would have set
    uint32_t all = 0;
    for (uint32_t bit = 1; bit <= TG_REPLAY_LISTS_NOT_ZERO; bit <<= 1)
      if (__syncthreads_or(flags & bit)) all |= bit;
    if (t == 0 && all && p.status) atomicOr(p.status, all);
  }
  int64_t V, n_surv;
  if (p.select == 0) {
    ring_plan_all(p.b, next, p.M, cnt, sh, [&](int64_t m0, int32_t* len, int64_t* park) {
      const int64_t m = m0 + t;
      const bool ok = m < p.M && list_valid(p, m, &flags);
      *len = ok ? static_cast<int32_t>(p.lengths[m]) : 0;
      *park = m;
      return ok;
    }, &V, &n_surv);
  } else {
    // (shorter, or equal at a smaller list index) wins: the sequential first-strict-maximum of the final reward -L
    const int64_t win = ring_best(bl, bm, best_l, best_m, [](int64_t a, int64_t b) { return a < b; });
    V = n_surv = ring_plan_one(p.b, next, win, best_l[0]);
    if (p.stored)  // every thread has read the flags of the lists it rewrites
      for (int64_t m = t; m < p.M; m += kRingScanBlock) p.stored[m] = m == win;
  }
  ring_commit(p.b, next, V, n_surv);
}

__device__ __forceinline__ int8_t lds_byte(const uint32_t* w, int e) {
  return static_cast<int8_t>(w[e >> 2] >> (8 * (e & 3)));
}

// the dword at byte offset 4 * at + o (o = 0..3) of the dword array w
__device__ __forceinline__ uint32_t lds_dword(const uint32_t* w, int at, int o) {
  const uint64_t two = static_cast<uint64_t>(w[at + 1]) << 32 | w[at];
  return static_cast<uint32_t>(two >> (8 * o));
}

// The n bytes of the tensor held in LDS (dwords w, byte 0 first; one dword of padding behind them) to dst, which has any
// alignment: bytes up to dst's first 16-byte boundary, 16-byte stores, a byte tail.  Exactly dst[0 .. n) is written.
__device__ __forceinline__ void store_tensor(int8_t* dst, const uint32_t* w, int n, int t, int nthr) {
  const int lead = static_cast<int>(-reinterpret_cast<uintptr_t>(dst) & 15);
  const int pre = lead < n ? lead : n;
  const int wide = (n - pre) / 16;
  for (int e = t; e < pre; e += nthr) dst[e] = lds_byte(w, e);
  uint4* out = reinterpret_cast<uint4*>(dst + pre);
  for (int c = t; c < wide; c += nthr) {
    const int at = (pre + 16 * c) >> 2, o = pre & 3;  // 16 c keeps the byte offset inside a dword
    out[c] = make_uint4(lds_dword(w, at, o), lds_dword(w, at + 1, o), lds_dword(w, at + 2, o), lds_dword(w, at + 3, o));
  }
  for (int e = pre + 16 * wide + t; e < n; e += nthr) dst[e] = lds_byte(w, e);
}

// entries of the tensor per emit workgroup, and its dynamic LDS in dwords: the entries' bytes (+ 2 of padding) of the T
// frames of the start state, uv[S^2], w[S], the token bytes of kTokenTile moves
__host__ __device__ inline int emit_chunk(int S) { return S * S * S <= kSmallEntries ? S * S * S : kEmitChunk; }
__host__ __device__ inline int tensor_words(int S) { return (emit_chunk(S) + 3) / 4 + 2; }
__host__ __device__ inline int emit_lds_words(int S, int T) {
  return T * tensor_words(S) + S * S + S + (kTokenTile * 3 * S + 3) / 4;
}

__global__ __launch_bounds__(kBlock) void lists_emit_kernel(ListArgs p) {
  extern __shared__ uint32_t lds[];
  int64_t slot, m;
  int len;
  if (!ring_survivor(p.b, blockIdx.x, &slot, &m, &len)) return;
  const int t = threadIdx.x, nthr = blockDim.x;
  const int S = p.b.S, S2 = S * S, N3 = S2 * S, A3 = 3 * S, T = p.b.T;
  const int64_t L = p.b.L;
  const int64_t g = p.groups ? p.groups[m] : m;
  const int8_t* tk = p.tokens + m * p.K * A3;
  const int8_t* st = p.starts + g * T * N3;
  int8_t* frames = p.b.frames + slot * L * T * N3;
  const int e0 = blockIdx.y * emit_chunk(S);                          // this workgroup's entries: [e0, e0 + nE)
  const int nE = N3 - e0 < emit_chunk(S) ? N3 - e0 : emit_chunk(S);

  // The T frames of the start state, TW dwords each (byte b = entry e0 + b); frame 0 becomes the head and is updated in
  // place.  Every global load of the walk's first kTokenTile moves is issued here, before the first frame store: a load
  // issued later waits behind the stores this wavefront has in flight.
  const int TW = tensor_words(S), nW = (nE + 3) / 4;
  uint32_t* head = lds;
  int32_t* uv = reinterpret_cast<int32_t*>(lds + T * TW);
  int32_t* wv = uv + S2;
  int8_t* tok = reinterpret_cast<int8_t*>(wv + S);  // the tokens of moves [tile, tile + kTokenTile)
  const uint64_t magic = (uint64_t{1} << 32) / S + 1;  // (e * magic) >> 32 == e / S for e < 2^15, S <= 32
  for (int f = 0; f < T; ++f) {
    const int8_t* src = st + static_cast<int64_t>(f) * N3 + e0;
    const bool dwords = (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    for (int wd = t; wd < nW + 2; wd += nthr) {  // the two dwords of padding store_tensor may read (and shift away): 0
      uint32_t x = 0;
      if (dwords && 4 * wd + 4 <= nE) {
        x = reinterpret_cast<const uint32_t*>(src)[wd];
      } else {
        for (int q = 0; q < 4; ++q)
          if (4 * wd + q < nE) x |= static_cast<uint32_t>(static_cast<uint8_t>(src[4 * wd + q])) << (8 * q);
      }
      head[f * TW + wd] = x;
    }
  }
  for (int q = t; q < (len < kTokenTile ? len : kTokenTile) * A3; q += nthr) tok[q] = tk[q];
  if (blockIdx.y == 0) {
    copy_bytes(p.b.tokens + slot * L * A3, tk, static_cast<int64_t>(len) * A3, t, nthr);
    for (int q = t; q < len; q += nthr) p.b.rewards[slot * L + q] = -static_cast<float>(q + 1);
  }

  for (int s = -(T - 1); s < len; ++s) {
    lds_barrier();  // the stores of the tensor before this one have read it
    if (s > 0) {
      // the tokens come through LDS, one fetch per kTokenTile moves
      const int mv = s - 1, tile = mv - mv % kTokenTile;
      if (mv == tile && tile > 0) {
        const int n = (len - tile < kTokenTile ? len - tile : kTokenTile) * A3;
        for (int q = t; q < n; q += nthr) tok[q] = tk[tile * A3 + q];
        lds_barrier();
      }
      const int8_t* row = tok + (mv - tile) * A3;
      for (int r = t; r < S2; r += nthr) {
        const int i = static_cast<int>(r * magic >> 32);
        uv[r] = (row[i] - p.shift) * (row[S + r - i * S] - p.shift);
      }
      for (int k = t; k < S; k += nthr) wv[k] = row[2 * S + k] - p.shift;
      lds_barrier();
      for (int wd = t; wd < nW; wd += nthr) {
        const uint32_t x = head[wd];
        uint32_t y = 0;
        for (int q = 0; q < 4; ++q) {
          if (4 * wd + q >= nE) break;
          const int e = e0 + 4 * wd + q;
          const int r = static_cast<int>(e * magic >> 32);
          const int32_t b = static_cast<int8_t>(x >> (8 * q));
          y |= static_cast<uint32_t>((b - uv[r] * wv[e - r * S]) & 0xff) << (8 * q);  // a valid list stays in int8
        }
        head[wd] = y;
      }
    }
    lds_barrier();
    const uint32_t* cur = s < 0 ? head + (-s) * TW : head;
    for (int f = s < 0 ? -s : 0; f < T && s + f < len; ++f)
      store_tensor(frames + (static_cast<int64_t>(s + f) * T + f) * N3 + e0, cur, nE, t, nthr);
  }
}

}  // namespace rl
}  // namespace tg

extern "C" int tg_replay_add_lists(const tg_replay_buffer* buf, const int8_t* starts, int64_t G, const int64_t* groups,
                                   const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int shift, int select,
                                   uint8_t* stored, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_replay_add_lists";
  if (!buf) return tg_internal_fail(TG_ERR_INVALID, "%s: null buffer", fn);
  if (int rc = check_ring_sizes(fn, "", buf)) return rc;
  if (M < 0 || M > INT32_MAX) return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M);
  if (G < 0 || G > INT32_MAX) return tg_internal_fail(TG_ERR_INVALID, "%s: G=%lld out of range", fn, (long long)G);
  if (K < 1 || K > TG_REPLAY_MAX_ACTIONS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: K=%d outside [1,%d]", fn, K, TG_REPLAY_MAX_ACTIONS);
  if (shift < 0 || shift > TG_REPLAY_LISTS_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_REPLAY_LISTS_MAX_SHIFT);
  if (select != 0 && select != 1) return tg_internal_fail(TG_ERR_INVALID, "%s: select=%d (0 all, 1 best)", fn, select);
  if (M == 0) return TG_OK;
  if (!groups && M > G)
    return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld > G=%lld with null groups", fn, (long long)M, (long long)G);
  if (int rc = check_ring_arrays(fn, "", buf)) return rc;
  if ((G > 0 && !starts) || !tokens || !lengths)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null starts, tokens or lengths", fn);
  if (!aligned(lengths, 8) || !aligned(groups, 8) || !aligned(status, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: lengths, groups or status not aligned to their elements", fn);
  const tg::rl::ListArgs p{*buf, starts, groups, tokens, lengths, G, M, K, shift, select, stored, status};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = buf->S;
  const bool small = S * S * S <= tg::rl::kSmallEntries;
  const unsigned block = small ? tg::rl::kSmallBlock : tg::kBlock;
  const unsigned chunks = (S * S * S + tg::rl::emit_chunk(S) - 1) / tg::rl::emit_chunk(S);
  const size_t lds = sizeof(uint32_t) * tg::rl::emit_lds_words(S, buf->T);
  const int64_t games = select ? 1 : (M < buf->C ? M : buf->C);
  if (stored)
    if (int rc = launch(fn, tg::rl::lists_valid_kernel, grid_for(M), small ? block : tg::rl::kValidBlock, 0, st, p))
      return rc;
  if (int rc = launch(fn, tg::rl::lists_plan_kernel, 1, tg::kRingScanBlock, 0, st, p)) return rc;
  if (int rc = launch(fn, tg::rl::lists_emit_kernel, dim3(static_cast<unsigned>(games), chunks), block, lds, st, p))
    return rc;
  return tg_internal_ring_rebuild(buf, st);
}
