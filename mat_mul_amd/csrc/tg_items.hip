// Items of a synthetic-demonstration set (include/tensor_game_demos.h, tg_demo_items): what
// SyntheticDemoDataset.__getitem__ (reference datasets.py:78-122) returns for a shuffled batch of flat indices, each
// item with its own (demo d, action index k), in ONE launch.  gfx950 only; part of libtensorgame.so.
// The bodies and the per-size kernel choice live in tg_items.h; here they run with the DemoRows policy.
#include <hip/hip_runtime.h>

#include "tg_items.h"

namespace {

struct DemoKernels {
  static constexpr const char* kName = "tg_demo_items";
  template <typename OutT, typename Acc>
  static constexpr auto s4() { return tg::items_s4_kernel<tg::DemoRows, OutT, Acc>; }
  template <int S, typename OutT>
  static constexpr auto mfma() { return tg::items_mfma_kernel<tg::DemoRows, S, OutT>; }
  template <typename OutT>
  static constexpr auto exact() { return tg::items_exact_kernel<tg::DemoRows, OutT>; }
};

}  // namespace

extern "C" int tg_demo_items(const int8_t* tokens, const int8_t* targets, int64_t n_demos, int R, int S,
                             int64_t target_stride_bytes, const int64_t* item_idx, int64_t N, int T, int out_dtype,
                             void* frames_out, float* scalars_out, int8_t* actions_out, float* rewards_out,
                             uint8_t* overflow, uint32_t* status, int shift, tg_stream_t stream) {
  if (int rc = check_items("tg_demo_items", n_demos, R, S, target_stride_bytes, T, out_dtype)) return rc;
  const tg::ItemArgs a{tokens, targets, n_demos, target_stride_bytes, item_idx, N, frames_out, scalars_out, actions_out,
                       rewards_out, overflow, status, R, S, T, shift, 0, 0};
  return run_items<DemoKernels>(a, out_dtype, static_cast<hipStream_t>(stream));
}
