// tg_ring.h -- the one protocol by which games enter a tg_replay_buffer ring (include/tensor_game_replay.h), shared by
// tg_replay_add (tg_replay.hip), tg_replay_add_packed (tg_replay_io.hip) and tg_replay_add_lists (tg_replay_lists.hip).
//
// The ring words: ring[0] = the next slot to write, in [0, C) for every ring this library has written and folded into
// it (ring_next) otherwise, so no slot index leaves the buffer; ring[1] = games ever added.
//
// An add is three launches on one stream and no host sync:
//   - the PLAN (one workgroup of kRingScanBlock) ranks the valid items of the call in item order.  With V of them,
//     n_surv = min(V, C) survive: rank r >= V - n_surv goes to slot (next + r) mod C (the earlier ones would be
//     overwritten within this call and are never written).  For every survivor the plan writes length[slot] and PARKS
//     the entry's index for it (a game, a first row, a list) in offset[slot]; it parks n_surv in offset[C], and then
//     advances the ring words (ring_commit);
//   - the COPY (one workgroup per possible survivor j) finds its slot back from the advanced ring[0], n_surv and j,
//     reads what was parked there (ring_survivor) and writes the game's frames, tokens and rewards;
//   - the REBUILD (tg_internal_ring_rebuild, one workgroup) restores offset = the exclusive prefix sums of length over
//     the C slots, offset[C] = every stored move.  Between the plan and the rebuild offset holds parked values and is
//     not an offset table: an add and a gather on one buffer must be ordered, as the header says.
// No atomics are needed: the plan is ONE workgroup, so a barrier orders its reads of ring[0] before the write, and the
// survivors' ranks are distinct modulo C (there are at most C of them), so every slot has one writer in the plan and
// one workgroup in the copy.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_replay.h"
#include "tg_host.h"

namespace tg {

constexpr int kRingScanBlock = 1024;

// exclusive prefix sum of v over the workgroup (kRingScanBlock threads); *total = the sum of all.  sh: kRingScanBlock
// int64.
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t* sh, int64_t* total) {
  const int t = threadIdx.x;
  __syncthreads();  // sh's previous readers are done
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kRingScanBlock; d <<= 1) {
    const int64_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  *total = sh[kRingScanBlock - 1];
  return sh[t] - v;
}

// ring[0] as a slot (a consistent ring holds 0 .. C-1; anything else is folded into it, so no index leaves the buffer)
__device__ __forceinline__ int64_t ring_next(const tg_replay_buffer& b) {
  const int64_t C = b.C;
  return (b.ring[0] % C + C) % C;
}

// The select-0 plan over items 0 .. n-1, by the whole plan workgroup.  cnt: the valid items this thread counted (the
// threads may split the items in any way).  item(g0, &len, &park) is called by every thread together, chunk after
// chunk, for item g0 + threadIdx.x: whether it is valid (false past n), its length and the index to park.  It may use
// block_exclusive_scan on sh itself.  *V = the valid items, *n_surv = the slots written.
template <typename Item>
__device__ __forceinline__ void ring_plan_all(const tg_replay_buffer& b, int64_t next, int64_t n, int64_t cnt,
                                              int64_t* sh, Item&& item, int64_t* V, int64_t* n_surv) {
  const int64_t C = b.C;
  block_exclusive_scan(cnt, sh, V);
  *n_surv = *V < C ? *V : C;
  const int64_t r0 = *V - *n_surv;  // ranks below r0 would be overwritten within this call: never written
  int64_t base = 0;
  for (int64_t g0 = 0; g0 < n; g0 += kRingScanBlock) {
    int32_t len;
    int64_t park;
    const bool ok = item(g0, &len, &park);
    int64_t chunk;
    const int64_t r = base + block_exclusive_scan(ok, sh, &chunk);
    if (ok && r >= r0) {
      const int64_t slot = (next + r) % C;
      b.offset[slot] = park;
      b.length[slot] = len;
    }
    base += chunk;
  }
}

// The select-1 winner over the workgroup: every thread brings its best (key, idx), idx < 0 for none and idx the
// smallest among equal keys.  better(a, b): key a beats key b; equal keys go to the smaller idx, which is what a
// sequential first-strict-best leaves.  Returns the winning idx (or -1) with its key in sh_key[0].
template <typename K, typename Better>
__device__ __forceinline__ int64_t ring_best(K key, int64_t idx, K* sh_key, int64_t* sh_idx, Better better) {
  const int t = threadIdx.x;
  sh_key[t] = key;
  sh_idx[t] = idx;
  __syncthreads();
  for (int d = kRingScanBlock / 2; d > 0; d >>= 1) {
    if (t < d) {
      const K k2 = sh_key[t + d];
      const int64_t i2 = sh_idx[t + d];
      if (i2 >= 0 && (sh_idx[t] < 0 || better(k2, sh_key[t]) || (k2 == sh_key[t] && i2 < sh_idx[t]))) {
        sh_key[t] = k2;
        sh_idx[t] = i2;
      }
    }
    __syncthreads();
  }
  return sh_idx[0];
}

// The select-1 plan: the winner `win` of `len` moves (win < 0: none) goes to slot `next`.  Returns V = n_surv.
__device__ __forceinline__ int64_t ring_plan_one(const tg_replay_buffer& b, int64_t next, int64_t win, int64_t len) {
  if (threadIdx.x == 0 && win >= 0) {
    b.offset[next] = win;
    b.length[next] = static_cast<int32_t>(len);
  }
  return win >= 0 ? 1 : 0;
}

// The plan's epilogue: the ring words advance by the V valid items (ring[1] becomes games_added instead when that is
// >= 0) and the survivor count is parked.
__device__ __forceinline__ void ring_commit(const tg_replay_buffer& b, int64_t next, int64_t V, int64_t n_surv,
                                            int64_t games_added = -1) {
  __syncthreads();  // every thread has read ring[0]
  if (threadIdx.x == 0) {
    b.ring[0] = (next + V) % b.C;
    b.ring[1] = games_added >= 0 ? games_added : b.ring[1] + V;
    b.offset[b.C] = n_surv;
  }
}

// Survivor j of the plan that ran before: its slot, the index parked there and its length; false for j >= n_surv.
__device__ __forceinline__ bool ring_survivor(const tg_replay_buffer& b, int64_t j, int64_t* slot, int64_t* parked,
                                              int* len) {
  const int64_t C = b.C, n_surv = b.offset[C];
  if (j >= n_surv) return false;
  *slot = ((b.ring[0] - n_surv + j) % C + C) % C;
  *parked = b.offset[*slot];
  *len = b.length[*slot];
  return true;
}

// n bytes from s to d by nthr threads (this one is t): the widest access both addresses allow (16 bytes, dwords, or
// bytes), then a byte tail
__device__ __forceinline__ void copy_bytes(int8_t* d, const int8_t* s, int64_t n, int t, int nthr) {
  const uintptr_t both = reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s);
  int64_t done = 0;
  if ((both & 15) == 0) {
    done = n & ~static_cast<int64_t>(15);
    for (int64_t c = t; c < done / 16; c += nthr) reinterpret_cast<uint4*>(d)[c] = reinterpret_cast<const uint4*>(s)[c];
  } else if ((both & 3) == 0) {
    done = n & ~static_cast<int64_t>(3);
    for (int64_t c = t; c < done / 4; c += nthr)
      reinterpret_cast<uint32_t*>(d)[c] = reinterpret_cast<const uint32_t*>(s)[c];
  }
  for (int64_t e = done + t; e < n; e += nthr) d[e] = s[e];
}

// ---- the host checks of a descriptor; `what` names the buffer in the message: "", "played " or "best " ---------------
inline int check_ring_sizes(const char* fn, const char* what, const tg_replay_buffer* b) {
  if (b->C < 1 || b->C > TG_REPLAY_MAX_CAPACITY)
    return tg_internal_fail(TG_ERR_INVALID, "%s: %sC=%d outside [1,%d]", fn, what, b->C, TG_REPLAY_MAX_CAPACITY);
  if (b->L < 1 || b->L > TG_REPLAY_MAX_ACTIONS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: %sL=%d outside [1,%d]", fn, what, b->L, TG_REPLAY_MAX_ACTIONS);
  if (b->T < 1 || b->T > TG_REPLAY_MAX_T)
    return tg_internal_fail(TG_ERR_INVALID, "%s: %sT=%d outside [1,%d]", fn, what, b->T, TG_REPLAY_MAX_T);
  if (b->S < 1 || b->S > TG_MAX_S)
    return tg_internal_fail(TG_ERR_INVALID, "%s: %sS=%d outside [1,%d]", fn, what, b->S, TG_MAX_S);
  return TG_OK;
}

inline int check_ring_arrays(const char* fn, const char* what, const tg_replay_buffer* b) {
  if (!b->frames || !b->tokens || !b->rewards || !b->length || !b->offset || !b->ring)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null %sbuffer array", fn, what);
  if (!aligned(b->rewards, 4) || !aligned(b->length, 4) || !aligned(b->offset, 8) || !aligned(b->ring, 8))
    return tg_internal_fail(TG_ERR_INVALID, "%s: %sbuffer arrays not aligned to their elements", fn, what);
  return TG_OK;
}

}  // namespace tg

using tg::check_ring_arrays;
using tg::check_ring_sizes;
