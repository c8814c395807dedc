// Sampled policy rollouts (include/tensor_game_rollout.h, tg_rollout_advance): everything the reference's solution
// search does between two network calls (training.py:253-268 and the running statistics of :343-346) in ONE launch.
// gfx950 only; part of libtensorgame.so.
//
// A row is a byte stream: T frames of N = S^3 bytes read, T written, in place.  The unit of work is an ITEM: W bytes at
// one element position of a row, through all T frames -- the thread that owns an item loads the head and the T - 1
// frames that stay, then stores them one frame later and the new head in front, so the history shift needs no second
// buffer and no ordering between threads.  W = 16 (aligned uint4) when S % 4 == 0 and the frames are 16-byte aligned,
// else W = 4 as unaligned dwords with the N % 4 last bytes of a row in a byte-wise tail item.  The rows of a group are
// next to each other and a workgroup owns whole groups (several small ones, so that a workgroup has about kRollItems
// items): the per-row counts meet in LDS (integer LDS adds: exact, order-free) and one thread per group updates the
// group's records -- one writer per record, no global atomics.
//
// Row mask (tg_rollout_advance_masked, M = true): a group is ACTIVE in a launch iff its solved_step is negative when the
// launch starts.  Every wave reads the solved_step of the workgroup's groups itself (they are written only behind the
// second barrier, which no wave passes before all have read), so the decision to return -- no group active -- is uniform
// without a barrier.  Of an inactive group nothing else is read and nothing is written; the activity of the groups lives
// in LDS from the first barrier on, because the records change while the rows are written back.  M = false is the plain
// entry: the same code with every test of the mask compiled out.
//
// Slots (include/tensor_game_rollout_slots.h, tg_rollout_advance_slots, mode 2): the masked step with the activity of a
// group read from three words (slot_state, solved_step, slot_step) and the step index per group: both go to LDS
// before one extra barrier, so everything behind it is the masked code with `step` looked up per group.  The body is
// one text, tg_rollout_body.h, included into rollout_advance_kernel<W, M> (Q = false: the code objects of its four
// instantiations are unchanged) and into rollout_advance_slots_kernel<W>, whose argument block carries the two extra
// pointers.  tg_rollout_refill (a one-workgroup plan kernel with a block scan, then one workgroup per
// slot) is at the end of the file.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_rollout_slots.h"  // and, through it, tensor_game_rollout[_masked].h
#include "tg_host.h"

namespace tg {

constexpr int kRollItems = 1024;     // items a workgroup aims for (four per thread)
constexpr int kRollMaxRows = 1024;   // rows of one workgroup: >= TG_NET_MAX_SAMPLES, >= kRollItems / (items per row)
constexpr int kRollTokBytes = 6144;  // their tokens: >= TG_NET_MAX_SAMPLES * 3 * TG_MAX_S

struct RolloutArgs {
  int8_t* frames;
  const int8_t* tokens;
  float* scalars;
  int32_t* nnz;
  uint8_t* overflow;
  int32_t *best_nnz, *hits, *solved_step, *solved_sample;
  int8_t* actions;
  uint8_t* active;  // M only, may be null: 1 for the rows of a group still unsolved after this step, else 0
  int64_t G;        // groups
  int n, S, T, dim_s, step, max_actions, shift;
  int gpw;          // groups per workgroup
  int ipr;          // items per row (the tail item included)
  int words;        // 1: tokens and actions move as aligned dwords (S % 4 == 0, 4-byte aligned pointers)
};

struct RolloutSlotArgs : RolloutArgs {
  const int64_t* slot_state;  // (G)
  int32_t* slot_step;         // (G)
};

struct __attribute__((packed)) RollU32 { uint32_t v; };

// nb valid bytes (nb == W: the whole item) at p -> q; bytes beyond nb read as zero
template <int W>
__device__ __forceinline__ void roll_load(const int8_t* p, int nb, uint32_t (&q)[W / 4]) {
  if constexpr (W == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
  } else {
    if (nb == 4) {
      q[0] = reinterpret_cast<const RollU32*>(p)->v;
    } else {
      q[0] = 0;
      for (int k = 0; k < nb; ++k) q[0] |= static_cast<uint32_t>(static_cast<uint8_t>(p[k])) << (8 * k);
    }
  }
}
template <int W>
__device__ __forceinline__ void roll_store(int8_t* p, int nb, const uint32_t (&q)[W / 4]) {
  if constexpr (W == 16) {
    *reinterpret_cast<uint4*>(p) = uint4{q[0], q[1], q[2], q[3]};
  } else {
    if (nb == 4) {
      reinterpret_cast<RollU32*>(p)->v = q[0];
    } else {
      for (int k = 0; k < nb; ++k) p[k] = static_cast<int8_t>(q[0] >> (8 * k));
    }
  }
}

__device__ __forceinline__ const int64_t* slot_state_of(const RolloutArgs&) { return nullptr; }
__device__ __forceinline__ int32_t* slot_step_of(const RolloutArgs&) { return nullptr; }
__device__ __forceinline__ const int64_t* slot_state_of(const RolloutSlotArgs& a) { return a.slot_state; }
__device__ __forceinline__ int32_t* slot_step_of(const RolloutSlotArgs& a) { return a.slot_step; }

template <int W, bool M>
__global__ __launch_bounds__(kBlock) void rollout_advance_kernel(const RolloutArgs a) {
  constexpr bool Q = false;
#include "tg_rollout_body.h"
}

template <int W>
__global__ __launch_bounds__(kBlock) void rollout_advance_slots_kernel(const RolloutSlotArgs a) {
  constexpr bool M = true, Q = true;
#include "tg_rollout_body.h"
}

// ---- tg_rollout_refill ------------------------------------------------------------------------------------------------
constexpr int kRefillScan = 1024;  // threads of the plan kernel; each owns up to TG_ROLLOUT_MAX_SLOTS / kRefillScan slots

struct RefillArgs {
  const int8_t* q_states;
  const float* q_scalars;
  int64_t N;
  int64_t* head;
  int64_t first_state;
  uint32_t seed_lo, seed_hi;
  int n_uniforms;  // 0: no uniforms
  int8_t* frames;
  float* scalars;
  int32_t* nnz;
  uint8_t* overflow;
  int32_t *best_nnz, *hits, *solved_step, *solved_sample;
  const int8_t* actions;
  uint8_t* active;
  int64_t* slot_state;
  int32_t* slot_step;
  int32_t *out_best_nnz, *out_hits, *out_solved_step, *out_solved_sample;
  uint8_t* out_overflow;
  int8_t* out_tokens;
  int64_t* rows;
  float* uniforms;
  int32_t* live;
  int R;  // slots
  int n, S, T, dim_s, max_actions;
  int wide;  // 1: 16-byte copies of the frames
};

// 0: the slot keeps its state; 1: it is finished (flush, then take); 2: it is empty (take)
__device__ __forceinline__ int slot_kind(const RefillArgs& a, int64_t g) {
  if (a.slot_state[g] < 0) return 2;
  return a.solved_step[g] >= 0 || a.slot_step[g] >= a.max_actions ? 1 : 0;
}

// The plan: in slot order, the j-th slot that wants a state gets head + j, or -1 when the queue is dry.  The answer
// goes to rows[g * n], which the fill kernel reads before it writes the slot's row keys; head and live are updated.
__global__ __launch_bounds__(kRefillScan) void rollout_refill_plan_kernel(const RefillArgs a) {
  __shared__ int sh[kRefillScan];
  const int t = threadIdx.x;
  const int per = (a.R + kRefillScan - 1) / kRefillScan;  // <= 64
  const int lo = min(t * per, a.R), hi = min(lo + per, a.R);
  int64_t head = a.head[0];
  head = head < 0 ? 0 : head > a.N ? a.N : head;
  int want = 0;
  for (int g = lo; g < hi; ++g) want += slot_kind(a, g) != 0;
  sh[t] = want;
  __syncthreads();
  for (int d = 1; d < kRefillScan; d <<= 1) {
    const int add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int64_t total = sh[kRefillScan - 1], avail = a.N - head;
  int64_t j = sh[t] - want;
  for (int g = lo; g < hi; ++g)
    if (slot_kind(a, g) != 0) {
      a.rows[static_cast<int64_t>(g) * a.n] = j < avail ? head + j : -1;
      ++j;
    }
  if (t == 0) {  // every thread read head[0] before the first barrier
    const int64_t taken = total < avail ? total : avail;
    a.head[0] = head + taken;
    a.live[0] = static_cast<int32_t>(a.R - total + taken);
  }
}

// One workgroup per slot: flush a finished slot, fill a slot that takes a state, then active and the uniforms.
__global__ __launch_bounds__(kBlock) void rollout_refill_fill_kernel(const RefillArgs a) {
  const int tid = threadIdx.x, n = a.n, K = a.max_actions, A3 = 3 * a.S;
  const int64_t g = blockIdx.x, b0 = g * n;
  const int kind = slot_kind(a, g);
  const int64_t old = a.slot_state[g];
  const int step = a.slot_step[g], sstep = a.solved_step[g], ssample = a.solved_sample[g];
  const int64_t q = kind ? a.rows[b0] : old;  // the state the slot holds from now on, < 0: none
  __syncthreads();                            // all of the above is read by every thread before any of it is written

  if (kind == 1 && old < a.N) {
    if (tid == 0) {
      a.out_best_nnz[old] = a.best_nnz[g];
      a.out_hits[old] = a.hits[g];
      a.out_solved_step[old] = sstep;
      a.out_solved_sample[old] = ssample;
      uint8_t ovf = 0;
      for (int s = 0; s < n; ++s) ovf |= a.overflow[b0 + s];
      a.out_overflow[old] = ovf ? 1 : 0;
    }
    const bool won = sstep >= 0 && sstep < K && ssample >= 0 && ssample < n;
    const int8_t* const src = a.actions + (b0 + (won ? ssample : 0)) * K * A3;
    int8_t* const dst = a.out_tokens + old * K * A3;
    const int keep = won ? (sstep + 1) * A3 : 0;
    for (int x = tid; x < K * A3; x += kBlock) dst[x] = x < keep ? src[x] : static_cast<int8_t>(0);
    __syncthreads();  // the overflow flags are read before they are cleared
  }

  if (kind && q >= 0) {
    const int64_t RB = static_cast<int64_t>(a.T) * a.S * a.S * a.S;  // bytes of a row
    const int8_t* const src = a.q_states + q * RB;
    int8_t* const dst = a.frames + b0 * RB;
    if (a.wide) {
      const int ipr = static_cast<int>(RB / 16);
      for (int x = tid; x < n * ipr; x += kBlock)
        reinterpret_cast<uint4*>(dst)[x] = reinterpret_cast<const uint4*>(src)[x % ipr];
    } else {
      const int full = static_cast<int>(RB / 4), ipr = static_cast<int>((RB + 3) / 4);
      for (int x = tid; x < n * ipr; x += kBlock) {
        const int r = x / ipr, c = x - r * ipr;
        const int8_t* const sp = src + 4 * c;
        int8_t* const dp = dst + r * RB + 4 * c;
        if (c < full) {
          reinterpret_cast<RollU32*>(dp)->v = reinterpret_cast<const RollU32*>(sp)->v;
        } else {
          for (int k = 0; k < static_cast<int>(RB) - 4 * full; ++k) dp[k] = sp[k];
        }
      }
    }
    if (a.scalars)
      for (int x = tid; x < n * a.dim_s; x += kBlock) a.scalars[b0 * a.dim_s + x] = a.q_scalars[q * a.dim_s + x % a.dim_s];
    for (int s = tid; s < n; s += kBlock) {
      a.rows[b0 + s] = (a.first_state + q) * n + s;
      a.nnz[b0 + s] = 0;
      a.overflow[b0 + s] = 0;
    }
    if (tid == 0) {
      a.best_nnz[g] = a.S * a.S * a.S;
      a.hits[g] = 0;
      a.solved_step[g] = -1;
      a.solved_sample[g] = -1;
      a.slot_state[g] = q;
      a.slot_step[g] = 0;
    }
  } else if (kind) {
    for (int s = tid; s < n; s += kBlock) a.rows[b0 + s] = -1;
    if (tid == 0) a.slot_state[g] = -1;
  }
  if (a.active)
    for (int s = tid; s < n; s += kBlock) a.active[b0 + s] = q >= 0 ? 1 : 0;

  if (a.uniforms && q >= 0) {
    const int nu = a.n_uniforms, quads = (nu + 3) / 4;
    const uint32_t call = kind ? 0u : static_cast<uint32_t>(step);
    for (int x = tid; x < n * quads; x += kBlock) {
      const int s = x / quads, c = x - s * quads;
      const uint32_t key = static_cast<uint32_t>((a.first_state + q) * n + s);
      const U4 w = philox4x32_10(U4{key, call, 0u, static_cast<uint32_t>(c)}, a.seed_lo, a.seed_hi);
      const uint32_t word[4] = {w.x, w.y, w.z, w.w};
      float* const u = a.uniforms + (b0 + s) * nu + 4 * c;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * c + k < nu) u[k] = static_cast<float>(word[k] >> 8) * 5.9604644775390625e-8f;
    }
  }
}

}  // namespace tg

namespace {

int rollout_check(const char* fn, int64_t B, int n, int S, int T, int dim_s, int step, int max_actions,
                  int with_actions) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (T < 1 || T > TG_NET_MAX_T)
    return tg_internal_fail(TG_ERR_INVALID, "%s: T=%d outside [1,%d] (TG_NET_MAX_T)", fn, T, TG_NET_MAX_T);
  if (n < 1 || n > TG_NET_MAX_SAMPLES)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n=%d outside [1,%d] (TG_NET_MAX_SAMPLES)", fn, n, TG_NET_MAX_SAMPLES);
  if (B < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld < 0", fn, (long long)B);
  if (B % n) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld is not a multiple of n=%d", fn, (long long)B, n);
  if (dim_s < 0 || dim_s > 64) return tg_internal_fail(TG_ERR_INVALID, "%s: dim_s=%d outside [0,64]", fn, dim_s);
  if (step < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: step=%d < 0", fn, step);
  if (with_actions && (max_actions < 1 || step >= max_actions))
    return tg_internal_fail(TG_ERR_INVALID, "%s: step=%d outside [0, max_actions=%d) of the actions record", fn, step,
                            max_actions);
  return TG_OK;
}

}  // namespace

extern "C" int tg_rollout_check(int64_t B, int n, int S, int T, int dim_s, int step, int max_actions, int with_actions) {
  return rollout_check("tg_rollout_check", B, n, S, T, dim_s, step, max_actions, with_actions);
}

namespace {

int slots_check(const char* fn, int64_t B, int n, int max_actions) {
  if (max_actions < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: max_actions=%d < 1", fn, max_actions);
  if (B / n > TG_ROLLOUT_MAX_SLOTS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: B/n=%lld slots, more than %d (TG_ROLLOUT_MAX_SLOTS)", fn,
                            (long long)(B / n), TG_ROLLOUT_MAX_SLOTS);
  return TG_OK;
}

// tg_rollout_advance (masked = false: `active` is ignored), tg_rollout_advance_masked, and tg_rollout_advance_slots
// (slots = true: masked, `step` is ignored, slot_state / slot_step say which groups are stepped and at which index)
int rollout_entry(const char* fn, bool masked, bool slots, const int64_t* slot_state, int32_t* slot_step, int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz,
                  uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                  int8_t* actions, uint8_t* active, int64_t B, int n, int S, int T, int dim_s, int step, int max_actions,
                  int shift, tg_stream_t stream) {
  if (int rc = rollout_check(fn, B, n, S, T, dim_s, step, max_actions, actions != nullptr)) return rc;
  if (slots)
    if (int rc = slots_check(fn, B, n, max_actions)) return rc;
  if (B == 0) return TG_OK;
  if (!frames) return tg_internal_fail(TG_ERR_INVALID, "%s: null frames", fn);
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!nnz) return tg_internal_fail(TG_ERR_INVALID, "%s: null nnz", fn);
  if (!best_nnz || !hits || !solved_step || !solved_sample)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null group record (best_nnz, hits, solved_step, solved_sample)", fn);
  if (slots && (!slot_state || !slot_step)) return tg_internal_fail(TG_ERR_INVALID, "%s: null slot_state or slot_step", fn);
  if (!aligned(nnz, 4) || !aligned(best_nnz, 4) || !aligned(hits, 4) || !aligned(solved_step, 4) ||
      !aligned(solved_sample, 4) || (scalars && !aligned(scalars, 4)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: nnz, the group records and scalars must be 4-byte aligned", fn);
  if (slots && (!aligned(slot_state, 8) || !aligned(slot_step, 4)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: slot_state must be 8-byte and slot_step 4-byte aligned", fn);

  const int N = S * S * S;
  const bool wide = S % 4 == 0 && aligned(frames, 16);  // then N % 64 == 0: every frame of every row is 16-byte aligned
  const int W = wide ? 16 : 4;
  tg::RolloutArgs a{frames, tokens, scalars, nnz, overflow, best_nnz, hits, solved_step, solved_sample, actions,
                    masked ? active : nullptr, B / n, n, S, T, scalars ? dim_s : 0, step, max_actions, shift, 1, (N + W - 1) / W, 0};
  a.words = S % 4 == 0 && aligned(tokens, 4) && (!actions || aligned(actions, 4));
  // several small groups per workgroup, within the LDS tables of the kernel
  int64_t gpw = tg::kRollItems / (static_cast<int64_t>(n) * a.ipr);
  if (gpw * n > tg::kRollMaxRows) gpw = tg::kRollMaxRows / n;
  if (gpw * n * 3 * S > tg::kRollTokBytes) gpw = tg::kRollTokBytes / (n * 3 * S);
  if (gpw > a.G) gpw = a.G;
  a.gpw = static_cast<int>(gpw < 1 ? 1 : gpw);
  const int64_t grid = (a.G + a.gpw - 1) / a.gpw;
  if (grid > 0x7fffffffll) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld: too large a grid", fn, (long long)B);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 dg(static_cast<unsigned>(grid)), db(tg::kBlock);
  if (slots) {
    tg::RolloutSlotArgs sa;
    static_cast<tg::RolloutArgs&>(sa) = a;
    sa.slot_state = slot_state, sa.slot_step = slot_step;
    if (wide) return launch(fn, tg::rollout_advance_slots_kernel<16>, dg, db, 0, st, sa);
    return launch(fn, tg::rollout_advance_slots_kernel<4>, dg, db, 0, st, sa);
  }
  if (masked) {
    if (wide) return launch(fn, tg::rollout_advance_kernel<16, true>, dg, db, 0, st, a);
    return launch(fn, tg::rollout_advance_kernel<4, true>, dg, db, 0, st, a);
  }
  if (wide) return launch(fn, tg::rollout_advance_kernel<16, false>, dg, db, 0, st, a);
  return launch(fn, tg::rollout_advance_kernel<4, false>, dg, db, 0, st, a);
}

}  // namespace

extern "C" int tg_rollout_advance(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz, uint8_t* overflow,
                                  int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                                  int8_t* actions, int64_t B, int n, int S, int T, int dim_s, int step, int max_actions,
                                  int shift, tg_stream_t stream) {
  return rollout_entry("tg_rollout_advance", false, false, nullptr, nullptr, frames, tokens, scalars, nnz, overflow, best_nnz, hits, solved_step,
                       solved_sample, actions, nullptr, B, n, S, T, dim_s, step, max_actions, shift, stream);
}

extern "C" int tg_rollout_advance_masked(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz,
                                         uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step,
                                         int32_t* solved_sample, int8_t* actions, uint8_t* active, int64_t B, int n,
                                         int S, int T, int dim_s, int step, int max_actions, int shift,
                                         tg_stream_t stream) {
  return rollout_entry("tg_rollout_advance_masked", true, false, nullptr, nullptr, frames, tokens, scalars, nnz, overflow, best_nnz, hits,
                       solved_step, solved_sample, actions, active, B, n, S, T, dim_s, step, max_actions, shift, stream);
}

extern "C" int tg_rollout_advance_slots(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz,
                                        uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step,
                                        int32_t* solved_sample, int8_t* actions, uint8_t* active,
                                        const int64_t* slot_state, int32_t* slot_step, int64_t B, int n, int S, int T,
                                        int dim_s, int max_actions, int shift, tg_stream_t stream) {
  // step 0 passes the step checks of the plain entry whenever max_actions >= 1, which slots_check asks for
  return rollout_entry("tg_rollout_advance_slots", true, true, slot_state, slot_step, frames, tokens, scalars, nnz,
                       overflow, best_nnz, hits, solved_step, solved_sample, actions, active, B, n, S, T, dim_s, 0,
                       max_actions, shift, stream);
}

extern "C" int tg_rollout_refill(const int8_t* q_states, const float* q_scalars, int64_t N, int64_t* head,
                                 int64_t first_state, uint64_t seed, int n_uniforms, int8_t* frames, float* scalars,
                                 int32_t* nnz, uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step,
                                 int32_t* solved_sample, const int8_t* actions, uint8_t* active, int64_t* slot_state,
                                 int32_t* slot_step, int32_t* out_best_nnz, int32_t* out_hits, int32_t* out_solved_step,
                                 int32_t* out_solved_sample, uint8_t* out_overflow, int8_t* out_tokens, int64_t* rows,
                                 float* uniforms, int32_t* live, int64_t B, int n, int S, int T, int dim_s,
                                 int max_actions, tg_stream_t stream) {
  const char* fn = "tg_rollout_refill";
  if (int rc = rollout_check(fn, B, n, S, T, dim_s, 0, max_actions, 1)) return rc;
  if (int rc = slots_check(fn, B, n, max_actions)) return rc;
  if (N < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld < 0", fn, (long long)N);
  if (first_state < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: first_state=%lld < 0", fn, (long long)first_state);
  if (uniforms && n_uniforms != 3 * S)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_uniforms=%d with uniforms given: must be 3*S=%d", fn, n_uniforms, 3 * S);
  if (B == 0 || N == 0) return TG_OK;
  if (!q_states) return tg_internal_fail(TG_ERR_INVALID, "%s: null q_states", fn);
  if (scalars && dim_s > 0 && !q_scalars) return tg_internal_fail(TG_ERR_INVALID, "%s: null q_scalars with scalars given", fn);
  if (!head) return tg_internal_fail(TG_ERR_INVALID, "%s: null head", fn);
  if (!frames) return tg_internal_fail(TG_ERR_INVALID, "%s: null frames", fn);
  if (!nnz) return tg_internal_fail(TG_ERR_INVALID, "%s: null nnz", fn);
  if (!overflow) return tg_internal_fail(TG_ERR_INVALID, "%s: null overflow", fn);
  if (!best_nnz || !hits || !solved_step || !solved_sample)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null group record (best_nnz, hits, solved_step, solved_sample)", fn);
  if (!actions) return tg_internal_fail(TG_ERR_INVALID, "%s: null actions", fn);
  if (!slot_state || !slot_step) return tg_internal_fail(TG_ERR_INVALID, "%s: null slot_state or slot_step", fn);
  if (!out_best_nnz || !out_hits || !out_solved_step || !out_solved_sample || !out_overflow || !out_tokens)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null output (out_best_nnz, out_hits, out_solved_step, "
                            "out_solved_sample, out_overflow, out_tokens)", fn);
  if (!rows) return tg_internal_fail(TG_ERR_INVALID, "%s: null rows", fn);
  if (!live) return tg_internal_fail(TG_ERR_INVALID, "%s: null live", fn);
  if (!aligned(nnz, 4) || !aligned(best_nnz, 4) || !aligned(hits, 4) || !aligned(solved_step, 4) ||
      !aligned(solved_sample, 4) || (scalars && !aligned(scalars, 4)) || (q_scalars && !aligned(q_scalars, 4)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: nnz, the group records, scalars and q_scalars must be 4-byte aligned", fn);
  if (!aligned(head, 8) || !aligned(slot_state, 8) || !aligned(rows, 8) || !aligned(slot_step, 4) || !aligned(live, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: head, slot_state and rows must be 8-byte, slot_step and live 4-byte "
                            "aligned", fn);
  if (!aligned(out_best_nnz, 4) || !aligned(out_hits, 4) || !aligned(out_solved_step, 4) || !aligned(out_solved_sample, 4) ||
      (uniforms && !aligned(uniforms, 4)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: the int32 outputs and uniforms must be 4-byte aligned", fn);

  tg::RefillArgs a{};
  a.q_states = q_states, a.q_scalars = q_scalars, a.N = N, a.head = head, a.first_state = first_state;
  a.seed_lo = static_cast<uint32_t>(seed), a.seed_hi = static_cast<uint32_t>(seed >> 32);
  a.n_uniforms = uniforms ? n_uniforms : 0;
  a.frames = frames, a.scalars = dim_s > 0 ? scalars : nullptr, a.nnz = nnz, a.overflow = overflow;
  a.best_nnz = best_nnz, a.hits = hits, a.solved_step = solved_step, a.solved_sample = solved_sample;
  a.actions = actions, a.active = active, a.slot_state = slot_state, a.slot_step = slot_step;
  a.out_best_nnz = out_best_nnz, a.out_hits = out_hits, a.out_solved_step = out_solved_step;
  a.out_solved_sample = out_solved_sample, a.out_overflow = out_overflow, a.out_tokens = out_tokens;
  a.rows = rows, a.uniforms = uniforms, a.live = live;
  a.R = static_cast<int>(B / n), a.n = n, a.S = S, a.T = T, a.dim_s = dim_s, a.max_actions = max_actions;
  a.wide = S % 4 == 0 && aligned(frames, 16) && aligned(q_states, 16);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = launch(fn, tg::rollout_refill_plan_kernel, dim3(1), dim3(tg::kRefillScan), 0, st, a)) return rc;
  return launch(fn, tg::rollout_refill_fill_kernel, dim3(static_cast<unsigned>(a.R)), dim3(tg::kBlock), 0, st, a);
}
