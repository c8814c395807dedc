// Items of a synthetic-demonstration set (include/tensor_game_demos.h, tg_demo_items): what
// SyntheticDemoDataset.__getitem__ (reference datasets.py:78-122) returns for a shuffled batch of flat indices, each
// item with its own (demo d, action index k), in ONE launch.  gfx950 only; part of libtensorgame.so.
// The bodies and the per-size kernel choice live in tg_items.h; here they run with the DemoRows policy.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_demos.h"
#include "tg_items.h"

namespace {

struct DemoKernels {
  static constexpr const char* kName = "tg_demo_items";
  template <typename OutT, typename Acc>
  static auto s4() { return tg::items_s4_kernel<tg::DemoRows, OutT, Acc>; }
  template <int S, typename OutT>
  static auto mfma() { return tg::items_mfma_kernel<tg::DemoRows, S, OutT>; }
  template <typename OutT>
  static auto exact() { return tg::items_exact_kernel<tg::DemoRows, OutT>; }
};

}  // namespace

extern "C" int tg_demo_items(const int8_t* tokens, const int8_t* targets, int64_t n_demos, int R, int S,
                             int64_t target_stride_bytes, const int64_t* item_idx, int64_t N, int T, int out_dtype,
                             void* frames_out, float* scalars_out, int8_t* actions_out, float* rewards_out,
                             uint8_t* overflow, uint32_t* status, int shift, tg_stream_t stream) {
  const char* fn = "tg_demo_items";
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (R < 1 || R > TG_DEMO_MAX_ACTIONS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: R=%d outside [1,%d]", fn, R, TG_DEMO_MAX_ACTIONS);
  if (T < 1 || T > TG_DEMO_MAX_T) return tg_internal_fail(TG_ERR_INVALID, "%s: T=%d outside [1,%d]", fn, T, TG_DEMO_MAX_T);
  if (n_demos < 0 || n_demos > INT64_MAX / R)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_demos=%lld out of range", fn, (long long)n_demos);
  const int64_t N3 = static_cast<int64_t>(S) * S * S;
  if (target_stride_bytes < N3)
    return tg_internal_fail(TG_ERR_INVALID, "%s: target_stride_bytes=%lld < S^3=%lld", fn, (long long)target_stride_bytes,
                            (long long)N3);
  if (out_dtype < 0 || out_dtype > 3)
    return tg_internal_fail(TG_ERR_INVALID, "%s: out_dtype=%d (0 f32, 1 f16, 2 bf16, 3 int8)", fn, out_dtype);
  if (N < 0 || N > INT64_MAX / (T * N3)) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)N);
  if (N == 0) return TG_OK;
  if (!item_idx || !frames_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null item_idx or frames_out", fn);
  if (n_demos > 0 && (!tokens || !targets)) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens or targets", fn);
  const int esize = out_dtype == 3 ? 1 : out_dtype == 0 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(frames_out) % esize)
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames_out not aligned to its %d-byte elements", fn, esize);
  tg::ItemArgs a{tokens, targets, n_demos, target_stride_bytes, item_idx, N, frames_out, scalars_out, actions_out,
                 rewards_out, overflow, status, R, S, T, shift, 0, 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (out_dtype) {
    case 0: return dispatch_items<float, DemoKernels>(a, st);
    case 1: return dispatch_items<__half, DemoKernels>(a, st);
    case 2: return dispatch_items<__hip_bfloat16, DemoKernels>(a, st);
    default: return dispatch_items<int8_t, DemoKernels>(a, st);
  }
}
