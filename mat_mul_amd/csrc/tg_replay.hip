// Replay buffers of played games and mixed training batches (include/tensor_game_replay.h).  gfx950 only; part of
// libtensorgame.so.
//
// tg_replay_add: the three launches of the ring protocol (tg_ring.h), no host sync.
//   - replay_plan_kernel (one workgroup of 1024): the plan over the storable games (select 0) or the one with the best
//     final reward (select 1); the parked index is the game's;
//   - replay_copy_kernel (one workgroup per possible survivor): copies the game's frames, takes the argmax token of
//     every (move, step) of its policy and copies its rewards;
//   - ring_rebuild_kernel (one workgroup of 1024): offset = exclusive prefix sums of length over the C slots.  It is
//     the library's only one: tg_internal_ring_rebuild launches it for the other two entries as well.
// tg_replay_items: the three item kernels of tg_items.h with the MixedRows policy -- a row resolves through the epoch
// table (or directly) to a synthetic item, which takes the tg_demo_items path unchanged, or to a stored move, found by a
// binary search over offset and written as a plain frame copy.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/tensor_game_replay.h"
#include "tg_items.h"
#include "tg_ring.h"

namespace tg {

// ---- rows of a mixed batch ------------------------------------------------------------------------------------------
struct BufView {        // what a gather reads of one buffer; C == 0: the buffer is absent (holds nothing)
  const int8_t* frames;
  const int8_t* tokens;
  const float* rewards;
  const int64_t* offset;
  int32_t C, L;
};

struct MixArgs {
  BufView buf[2];       // played, best
  const uint8_t* kind;  // epoch table [len_data], or NULL: every row is of direct_kind at source index idx[n]
  const int64_t* src;
  int64_t len_data;
  int direct_kind;
};

struct MixedRows {
  static constexpr bool kMixed = true;
  MixArgs x;

  // the kind (3: a bad dataset index) and the source index of row n
  __device__ __forceinline__ int lookup(const ItemArgs& a, int64_t n, int64_t& s) const {
    const int64_t i = a.idx[n];
    if (!x.kind) {
      s = i;
      return x.direct_kind;
    }
    const bool ok = i >= 0 && i < x.len_data;
    s = ok ? x.src[i] : -1;
    return ok ? x.kind[i] : 3;
  }

  // a synthetic row (valid or not); a stored move or a bad row is an invalid synthetic item here
  __device__ __forceinline__ Item item(const ItemArgs& a, int64_t n) const {
    int64_t s;
    const int k = lookup(a, n, s);
    Item it;
    it.valid = k == TG_REPLAY_SYNTH && s >= 0 && s < a.n_demos * a.R;
    it.d = it.valid ? s / a.R : 0;
    it.k = it.valid ? static_cast<int>(s - it.d * a.R) : 0;
    return it;
  }

  // row n is move m of slot `slot` of buffer b: the slot with offset[slot] <= s < offset[slot+1] (empty slots have
  // offset[slot] == offset[slot+1] and are never found); false for anything else
  __device__ __forceinline__ bool stored(const ItemArgs& a, int64_t n, BufView& b, int& slot, int& m) const {
    int64_t s;
    const int k = lookup(a, n, s);
    if (k != TG_REPLAY_PLAYED && k != TG_REPLAY_BEST) return false;
    b = k == TG_REPLAY_PLAYED ? x.buf[0] : x.buf[1];
    if (b.C <= 0 || s < 0 || s >= b.offset[b.C]) return false;
    int lo = 0, hi = b.C - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (b.offset[mid + 1] > s) hi = mid;
      else lo = mid + 1;
    }
    const int64_t mm = s - b.offset[lo];
    slot = lo;
    m = static_cast<int>(mm);
    return mm >= 0 && mm < b.L;  // (holds for a consistent buffer; the guard keeps every read inside it)
  }

  // PlayedGamesDataset.__getitem__: the stored frames, scalar = m, the stored tokens and reward
  template <typename OutT>
  __device__ __forceinline__ bool write_stored(const ItemArgs& a, int64_t n, OutT* out, int t, int nthr) const {
    BufView b;
    int slot, m;
    if (!stored(a, n, b, slot, m)) return false;
    const int N3 = a.S * a.S * a.S, A3 = 3 * a.S;
    const int64_t row = static_cast<int64_t>(slot) * b.L + m;
    if (t == 0) {
      if (a.scalars) a.scalars[n] = static_cast<float>(m);
      if (a.rewards) a.rewards[n] = b.rewards[row];
    }
    if (a.actions)
      for (int q = t; q < A3; q += nthr) a.actions[n * A3 + q] = b.tokens[row * A3 + q];
    const int8_t* f = b.frames + row * a.T * N3;
    write_frame(out, a.T * N3, t, nthr, [&](int e) { return static_cast<int>(f[e]); });
    return true;
  }
};

// ---- tg_replay_add --------------------------------------------------------------------------------------------------
struct AddArgs {
  tg_replay_buffer b;
  const int8_t* states;  // (B,L,T,S^3)
  const float* policy;   // (B,L,3S,n_logits)
  const float* rewards;  // (B,L)
  const int64_t* lengths;
  int64_t B;
  int n_logits, select;
  uint32_t* status;
};

__device__ __forceinline__ bool storable(int64_t len, int L) { return len >= 1 && len <= L; }

__global__ __launch_bounds__(kRingScanBlock) void replay_plan_kernel(AddArgs p) {
  __shared__ int64_t sh[kRingScanBlock];
  __shared__ float best_r[kRingScanBlock];
  __shared__ int64_t best_g[kRingScanBlock];
  const int t = threadIdx.x, L = p.b.L;
  const int64_t next = ring_next(p.b);
  int64_t cnt = 0;
  int bad = 0;
  float br = -1e6f;  // act_step: best_reward = -1e6, strict >
  int64_t bg = -1;
  for (int64_t g = t; g < p.B; g += kRingScanBlock) {
    const int64_t len = p.lengths[g];
    const bool ok = storable(len, L);
    cnt += ok;
    bad |= !ok;
    if (ok) {
      const float r = p.rewards[g * L + len - 1];
      if (r > br) br = r, bg = g;  // within a thread g rises: the first maximum stays
    }
  }
  if (__syncthreads_or(bad) && t == 0 && p.status) atomicOr(p.status, 1u);
  int64_t V, n_surv;
  if (p.select == 0) {
    ring_plan_all(p.b, next, p.B, cnt, sh, [&](int64_t g0, int32_t* len, int64_t* park) {
      const int64_t g = g0 + t, n = g < p.B ? p.lengths[g] : 0;
      *len = static_cast<int32_t>(n);
      *park = g;
      return storable(n, L);
    }, &V, &n_surv);
  } else {
    // (reward greater, or equal at a smaller game index) wins: the sequential first-strict-maximum
    const int64_t g = ring_best(br, bg, best_r, best_g, [](float a, float b) { return a > b; });
    V = n_surv = ring_plan_one(p.b, next, g, g >= 0 ? p.lengths[g] : 0);
  }
  ring_commit(p.b, next, V, n_surv);
}

// torch.argmax over n floats: the first maximal index, a NaN counts as the maximum (the first NaN wins)
__device__ __forceinline__ int argmax_first(const float* v, int n) {
  float best = v[0];
  int at = 0;
  if (std::isnan(best)) return 0;
  for (int q = 1; q < n; ++q) {
    const float x = v[q];
    if (std::isnan(x)) return q;
    if (x > best) best = x, at = q;
  }
  return at;
}

__global__ __launch_bounds__(kBlock) void replay_copy_kernel(AddArgs p) {
  int64_t slot, g;
  int len;
  if (!ring_survivor(p.b, blockIdx.x, &slot, &g, &len)) return;
  const int t = threadIdx.x, L = p.b.L, A3 = 3 * p.b.S;
  const int64_t fb = static_cast<int64_t>(p.b.T) * p.b.S * p.b.S * p.b.S;  // bytes per state
  copy_bytes(p.b.frames + slot * L * fb, p.states + g * L * fb, len * fb, t, kBlock);
  const float* pol = p.policy + g * L * A3 * static_cast<int64_t>(p.n_logits);
  int8_t* tk = p.b.tokens + slot * L * A3;
  for (int q = t; q < len * A3; q += kBlock)
    tk[q] = static_cast<int8_t>(argmax_first(pol + static_cast<int64_t>(q) * p.n_logits, p.n_logits));
  for (int m = t; m < len; m += kBlock) p.b.rewards[slot * L + m] = p.rewards[g * L + m];
}

__global__ __launch_bounds__(kRingScanBlock) void ring_rebuild_kernel(tg_replay_buffer b) {
  __shared__ int64_t sh[kRingScanBlock];
  const int t = threadIdx.x, per = (b.C + kRingScanBlock - 1) / kRingScanBlock;
  const int lo = min(t * per, b.C), hi = min(lo + per, b.C);
  int64_t sum = 0;
  for (int s = lo; s < hi; ++s) sum += b.length[s];
  int64_t total;
  int64_t run = block_exclusive_scan(sum, sh, &total);
  for (int s = lo; s < hi; ++s) {
    b.offset[s] = run;
    run += b.length[s];
  }
  if (t == 0) b.offset[b.C] = total;
}

}  // namespace tg

namespace {

struct MixKernels {
  static constexpr const char* kName = "tg_replay_items";
  template <typename OutT, typename Acc>
  static constexpr auto s4() { return tg::items_s4_kernel<tg::MixedRows, OutT, Acc, tg::MixArgs>; }
  template <int S, typename OutT>
  static constexpr auto mfma() { return tg::items_mfma_kernel<tg::MixedRows, S, OutT, tg::MixArgs>; }
  template <typename OutT>
  static constexpr auto exact() { return tg::items_exact_kernel<tg::MixedRows, OutT, tg::MixArgs>; }
};

}  // namespace

extern "C" int tg_replay_add(const tg_replay_buffer* buf, const int8_t* states, const float* policy, int n_logits,
                             const float* rewards, const int64_t* lengths, int64_t B, int select, uint32_t* status,
                             tg_stream_t stream) {
  const char* fn = "tg_replay_add";
  if (!buf) return tg_internal_fail(TG_ERR_INVALID, "%s: null buffer", fn);
  if (int rc = check_ring_sizes(fn, "", buf)) return rc;
  if (int rc = check_ring_arrays(fn, "", buf)) return rc;
  if (n_logits < 1 || n_logits > TG_REPLAY_MAX_LOGITS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_logits=%d outside [1,%d]", fn, n_logits, TG_REPLAY_MAX_LOGITS);
  if (select != 0 && select != 1) return tg_internal_fail(TG_ERR_INVALID, "%s: select=%d (0 all, 1 best)", fn, select);
  if (B < 0 || B > INT32_MAX) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld out of range", fn, (long long)B);
  if (B == 0) return TG_OK;
  if (!states || !policy || !rewards || !lengths)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null states, policy, rewards or lengths", fn);
  if (!aligned(policy, 4) || !aligned(rewards, 4) || !aligned(lengths, 8))
    return tg_internal_fail(TG_ERR_INVALID, "%s: policy, rewards or lengths not aligned to their elements", fn);
  const tg::AddArgs p{*buf, states, policy, rewards, lengths, B, n_logits, select, status};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t copies = select ? 1 : (B < buf->C ? B : buf->C);
  if (int rc = launch(fn, tg::replay_plan_kernel, 1, tg::kRingScanBlock, 0, st, p)) return rc;
  if (int rc = launch(fn, tg::replay_copy_kernel, static_cast<unsigned>(copies), tg::kBlock, 0, st, p)) return rc;
  return tg_internal_ring_rebuild(buf, st);
}

int tg_internal_ring_rebuild(const tg_replay_buffer* buf, hipStream_t st) {
  return launch("tg_internal_ring_rebuild", tg::ring_rebuild_kernel, 1, tg::kRingScanBlock, 0, st, *buf);
}

extern "C" int tg_replay_items(const int8_t* tokens, const int8_t* targets, int64_t n_demos, int R, int S,
                               int64_t target_stride_bytes, int shift, const tg_replay_buffer* played,
                               const tg_replay_buffer* best, const uint8_t* kind, const int64_t* src, int64_t len_data,
                               int direct_kind, const int64_t* item_idx, int64_t N, int T, int out_dtype,
                               void* frames_out, float* scalars_out, int8_t* actions_out, float* rewards_out,
                               uint8_t* overflow, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_replay_items";
  if (int rc = check_items(fn, n_demos, R, S, target_stride_bytes, T, out_dtype)) return rc;
  const tg_replay_buffer* bufs[2] = {played, best};
  const char* names[2] = {"played ", "best "};
  for (int q = 0; q < 2; ++q) {
    if (!bufs[q]) continue;
    if (int rc = check_ring_sizes(fn, names[q], bufs[q])) return rc;
    if (int rc = check_ring_arrays(fn, names[q], bufs[q])) return rc;
    if (bufs[q]->S != S || bufs[q]->T != T)
      return tg_internal_fail(TG_ERR_INVALID, "%s: %sbuffer has S=%d T=%d, the items S=%d T=%d", fn, names[q],
                              bufs[q]->S, bufs[q]->T, S, T);
  }
  if (kind) {
    if (!src) return tg_internal_fail(TG_ERR_INVALID, "%s: null src with an epoch table", fn);
    if (len_data < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: len_data=%lld", fn, (long long)len_data);
  } else if (direct_kind < TG_REPLAY_SYNTH || direct_kind > TG_REPLAY_BEST) {
    return tg_internal_fail(TG_ERR_INVALID, "%s: direct_kind=%d outside [0,2]", fn, direct_kind);
  }
  tg::MixArgs x{};
  for (int q = 0; q < 2; ++q)
    if (bufs[q]) x.buf[q] = tg::BufView{bufs[q]->frames, bufs[q]->tokens, bufs[q]->rewards, bufs[q]->offset,
                                        bufs[q]->C, bufs[q]->L};
  x.kind = kind;
  x.src = src;
  x.len_data = len_data;
  x.direct_kind = direct_kind;
  const tg::ItemArgs a{tokens, targets, n_demos, target_stride_bytes, item_idx, N, frames_out, scalars_out, actions_out,
                       rewards_out, overflow, status, R, S, T, shift, 0, 0};
  return run_items<MixKernels>(a, out_dtype, static_cast<hipStream_t>(stream), x);
}
