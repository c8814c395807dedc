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
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_rollout.h"  // and, through it, tensor_game_rollout_masked.h
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

template <int W, bool M>
__global__ __launch_bounds__(kBlock) void rollout_advance_kernel(const RolloutArgs a) {
  __shared__ __attribute__((aligned(16))) int8_t s_tok[kRollTokBytes];
  __shared__ int s_nnz[kRollMaxRows];
  __shared__ int s_ovf[kRollMaxRows];
  __shared__ uint8_t s_act[M ? kRollMaxRows : 1];  // per group of the workgroup (at most one group per row)
  const int tid = threadIdx.x;
  const int S = a.S, S2 = S * S, N = S2 * S, A3 = 3 * S, T = a.T, n = a.n;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * a.gpw;
  const int ng = static_cast<int>(a.G - g0 < a.gpw ? a.G - g0 : a.gpw);  // >= 1: the grid is ceil(G / gpw)
  const int rows = ng * n;
  const int64_t b0 = g0 * n;
  bool mixed = false;  // some groups of this workgroup may be inactive: a workgroup of ONE group that goes on is active
  if constexpr (M) {
    bool any = false;
    for (int base = 0; base < ng; base += 64) {  // every wave over all the groups: the same answer in each
      const int lg = base + (tid & 63);
      const bool act = lg < ng && a.solved_step[g0 + lg] < 0;
      if (tid < 64 && lg < ng) s_act[lg] = act;
      any |= act;
    }
    if (!__any(any)) return;
    mixed = ng > 1;
  }

  // ---- the rows' tokens into LDS (and into the record of played actions), scalars + 1, the counters cleared
  if (a.words) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tokens + b0 * A3);
    const int wpr = A3 / 4;
    for (int x = tid; x < rows * wpr; x += kBlock) {
      if (M && mixed && a.solved_step[g0 + x / wpr / n] >= 0) continue;
      const uint32_t t = src[x];
      reinterpret_cast<uint32_t*>(s_tok)[x] = t;
      if (a.actions) {
        const int r = x / wpr, c = x - r * wpr;
        reinterpret_cast<uint32_t*>(a.actions + ((b0 + r) * a.max_actions + a.step) * A3)[c] = t;
      }
    }
  } else {
    const int8_t* src = a.tokens + b0 * A3;
    for (int x = tid; x < rows * A3; x += kBlock) {
      if (M && mixed && a.solved_step[g0 + x / A3 / n] >= 0) continue;
      const int8_t t = src[x];
      s_tok[x] = t;
      if (a.actions) {
        const int r = x / A3, c = x - r * A3;
        a.actions[((b0 + r) * a.max_actions + a.step) * A3 + c] = t;
      }
    }
  }
  if (a.scalars) {
    float* sc = a.scalars + b0 * a.dim_s;
    for (int x = tid; x < rows * a.dim_s; x += kBlock) {
      if (M && mixed && a.solved_step[g0 + x / a.dim_s / n] >= 0) continue;
      sc[x] += 1.0f;
    }
  }
  for (int r = tid; r < rows; r += kBlock) s_nnz[r] = 0, s_ovf[r] = 0;
  __syncthreads();

  // ---- the items: new head, history shift, per-row counts
  const int full = N / W;  // items of W whole bytes; item `full` (W == 4 only) is the N % 4 tail
  const int nkeep = T > 1 ? T - 1 : 1;  // frames loaded: 0 .. T - 2 move back by one; T == 1 loads the head alone
  const int total = rows * a.ipr;
  for (int it = tid; it < total; it += kBlock) {
    const int lr = it / a.ipr, c = it - lr * a.ipr;
    if (M && mixed && !s_act[lr / n]) continue;
    const int nb = c < full ? W : N - full * W;
    const int e0 = c * W;
    int8_t* const row = a.frames + (b0 + lr) * static_cast<int64_t>(T) * N + e0;
    uint32_t fr[TG_NET_MAX_T][W / 4];
#pragma unroll
    for (int t = 0; t < TG_NET_MAX_T - 1; ++t)
      if (t < nkeep) roll_load<W>(row + static_cast<int64_t>(t) * N, nb, fr[t]);

    const int8_t* const tk = s_tok + lr * A3;
    int i = e0 / S2, rem = e0 - i * S2, j = rem / S, l = rem - j * S;
    uint32_t uv = static_cast<uint32_t>(tk[i] - a.shift) * static_cast<uint32_t>(tk[S + j] - a.shift);
    uint32_t head[W / 4];
    int ovf = 0, cnt = 0;
#pragma unroll
    for (int d = 0; d < W / 4; ++d) {
      uint32_t out = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (4 * d + t < nb) {
          const int p = static_cast<int>(uv * static_cast<uint32_t>(tk[2 * S + l] - a.shift));
          const int nw = sbyte(fr[0][d], t) - p;  // 32-bit, then narrowed with wrap as tg_step_i8 does
          ovf |= nw + 128;
          out |= (static_cast<uint32_t>(nw) & 255u) << (8 * t);
          if (++l == S) {  // the row (i, j) of the tensor ends inside the item: next factors (tk[S] / tk[2S] past the
            l = 0;         // last element are in-row reads of v_0 / w_0 that are never used)
            if (++j == S) j = 0, ++i;
            uv = static_cast<uint32_t>(tk[i] - a.shift) * static_cast<uint32_t>(tk[S + j] - a.shift);
          }
        }
      }
      head[d] = out;
      cnt = count_nonzero_bytes(out, cnt);
    }
#pragma unroll
    for (int t = TG_NET_MAX_T - 2; t >= 0; --t)
      if (t < T - 1) roll_store<W>(row + static_cast<int64_t>(t + 1) * N, nb, fr[t]);
    roll_store<W>(row, nb, head);
    if (cnt) atomicAdd(&s_nnz[lr], cnt);
    if (ovf & ~255) s_ovf[lr] = 1;
  }
  __syncthreads();

  // ---- per row, then per group
  for (int r = tid; r < rows; r += kBlock) {
    if (M && mixed && !s_act[r / n]) continue;
    a.nnz[b0 + r] = s_nnz[r];
    if (a.overflow && s_ovf[r]) a.overflow[b0 + r] = 1;
    if (M && a.active) {  // the group's verdict again, per row: no third barrier
      const int* const grp = s_nnz + r / n * n;
      bool zero = false;
      for (int s = 0; s < n; ++s) zero |= grp[s] == 0;
      a.active[b0 + r] = zero ? 0 : 1;
    }
  }
  for (int lg = tid; lg < ng; lg += kBlock) {
    if (M && mixed && !s_act[lg]) continue;
    int best = s_nnz[lg * n], first = -1;
    for (int s = n - 1; s >= 0; --s) {
      const int v = s_nnz[lg * n + s];
      best = v < best ? v : best;
      first = v == 0 ? s : first;
    }
    const int64_t g = g0 + lg;
    const int old = a.best_nnz[g];
    a.best_nnz[g] = best < old ? best : old;
    if (best == 0) {
      a.hits[g] += 1;
      if (a.solved_step[g] < 0) a.solved_step[g] = a.step, a.solved_sample[g] = first;
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

// tg_rollout_advance (masked = false: `active` is ignored) and tg_rollout_advance_masked
int rollout_entry(const char* fn, bool masked, int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz,
                  uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                  int8_t* actions, uint8_t* active, int64_t B, int n, int S, int T, int dim_s, int step, int max_actions,
                  int shift, tg_stream_t stream) {
  if (int rc = rollout_check(fn, B, n, S, T, dim_s, step, max_actions, actions != nullptr)) return rc;
  if (B == 0) return TG_OK;
  if (!frames) return tg_internal_fail(TG_ERR_INVALID, "%s: null frames", fn);
  if (!tokens) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens", fn);
  if (!nnz) return tg_internal_fail(TG_ERR_INVALID, "%s: null nnz", fn);
  if (!best_nnz || !hits || !solved_step || !solved_sample)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null group record (best_nnz, hits, solved_step, solved_sample)", fn);
  if (!aligned(nnz, 4) || !aligned(best_nnz, 4) || !aligned(hits, 4) || !aligned(solved_step, 4) ||
      !aligned(solved_sample, 4) || (scalars && !aligned(scalars, 4)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: nnz, the group records and scalars must be 4-byte aligned", fn);

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
  return rollout_entry("tg_rollout_advance", false, frames, tokens, scalars, nnz, overflow, best_nnz, hits, solved_step,
                       solved_sample, actions, nullptr, B, n, S, T, dim_s, step, max_actions, shift, stream);
}

extern "C" int tg_rollout_advance_masked(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz,
                                         uint8_t* overflow, int32_t* best_nnz, int32_t* hits, int32_t* solved_step,
                                         int32_t* solved_sample, int8_t* actions, uint8_t* active, int64_t B, int n,
                                         int S, int T, int dim_s, int step, int max_actions, int shift,
                                         tg_stream_t stream) {
  return rollout_entry("tg_rollout_advance_masked", true, frames, tokens, scalars, nnz, overflow, best_nnz, hits,
                       solved_step, solved_sample, actions, active, B, n, S, T, dim_s, step, max_actions, shift, stream);
}
