// Shared by tg_train_sliced.hip (training at S = TG_NET_WIDE2_S) and tg_train_s25.hip (training at S = TG_NET_WIDE3_S):
// the torso kernels by slices (defined in tg_train_sliced.hip; they take S at run time), their LDS plan, and the
// workspace parts the two sizes have in common.
#pragma once

#include "tg_train_common.h"

namespace tg {
namespace train {

// the torso kernels: tplan's buffers for one slice (3S grid rows, 3S input rows, a pair's 2S tokens), one sequence of scratch
__host__ __device__ inline TPlan tplan_slice(const tg_net_config& c) {
  const int S = c.S, cin = S * c.T + 1;
  TPlan p;
  p.G = 0;
  p.IN = p.G + 3 * S * c.c;
  p.X = p.IN + 3 * S * cin;
  p.DO = p.X + 2 * S * c.c;
  p.DX = p.DO + 2 * S * c.c;
  p.SS = p.DX + 2 * S * c.c;
  p.DP = p.SS + TG_NET_MAX_DIM_S;
  p.SCR = p.DP + 3 * S;
  p.total = p.SCR + scr_plan(torso_geo(c, 1)).total;
  return p;
}

inline int torso_partials(const tg_net_config& c, int64_t B) {
  const int64_t units = B * c.S;
  return static_cast<int>(units < TG_NET_TRAIN_PARTIALS ? units : TG_NET_TRAIN_PARTIALS);
}

struct WsSliced {  // byte offsets into the workspace
  int64_t ee, dee, act, gl, flags, xs, slabs, total;
};

inline WsSliced ws_plan_sliced(const tg_net_config& c, int64_t B) {
  const int64_t J = 3LL * c.S * c.S, T2 = 2LL * c.S * c.S;
  WsSliced w;
  int64_t p = 0;
  w.ee = p; p += round256(4 * B * J * c.c);
  w.dee = p; p += round256(4 * B * J * c.c);
  w.act = p; p += round256(4 * B * c.torso_layers * 3 * T2 * c.c);
  w.gl = p; p += round256(4 * 2 * B);
  w.flags = p; p += round256(4 * B);
  w.xs = p; p += round256(4LL * partials(B) * c.blocks * 2 * c.n_steps * c.W);
  w.slabs = p; p += round256(4 * torso_partials(c, B) * net::offsets(c).total);
  w.total = p;
  return w;
}

// launch 1: the torso forward of one slice, B * S workgroups
__global__ void __launch_bounds__(NT) train_torso_fwd_slice_kernel(Args a);
// launch 3: the torso backward, a.P = Pt workgroups; Pd: the workgroups of launch 2, whose slabs hold the policy and
// value part already
__global__ void __launch_bounds__(NT) train_torso_bwd_slice_kernel(Args a, int Pd);

}  // namespace train
}  // namespace tg
