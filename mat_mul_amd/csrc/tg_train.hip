// The training loss of the AlphaTensor network and its gradient (include/tensor_game_train.h).  gfx950 only; part of
// libtensorgame.so.
//
// Four kernels, plain fp32 with every activation in LDS and the weights read from global memory:
//   - train_torso_fwd_kernel: one workgroup per game, the torso forward of tg_net.hip; before each attention pair it
//     saves the pair's input (2S^2 x c) to the workspace, and it writes ee there at the end.
//   - train_decode_kernel: P workgroups, each taking a contiguous run of games in order.  Per game: the teacher-forced
//     decoder on all n_steps positions at once (causal mask), saving every block's input and mid-point; the logits, the
//     value head and both losses; then the backward, block by block in reverse, each attention block recomputed from
//     its saved input (mha_bwd), into the workgroup's partial slab; dL/dee to the workspace.
//   - train_torso_bwd_kernel: the same P workgroups and games; the pairs in reverse, each recomputed from its saved input.
//   - train_reduce_kernel (tg_train_common.h): grad[i] = sum over p = 0 .. P-1 of slab p's element i, in that order; one more workgroup sums
//     the per-game losses and ORs the flags in a fixed tree.
// No float atomics: a slab element is only ever read-modified-written by one workgroup, between barriers.
#include "tg_train_common.h"

namespace tg {
namespace train {

// ---- kernel 1: the torso forward, saving each pair's input ----------------------------------------------------------
// CHUNKED (S = TG_NET_WIDE_S): a pair's S sequences are independent (layernorm and the MLP are row-wise, attention stays
// inside a sequence), so its attention block runs over `chunk` sequences at a time with scratch for that many.
template <bool CHUNKED>
__device__ inline void torso_fwd(const Args& a, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int S = c.S, S2 = S * S, T2 = 2 * S2, C = c.c, cin = S * c.T + 1;
  const int64_t g = blockIdx.x;
  if (g >= a.B) return;
  const TPlan L = CHUNKED ? tplan(c, chunk) : tplan(c);
  float *G = lds + L.G, *IN = lds + L.IN, *X = lds + L.X, *OUT = lds + L.DO, *SCR = lds + L.SCR;
  net::torso_inputs(c, a.off, a.w, a.frames, a.frames_i8, a.scalars, g, S, 0, IN);
  __syncthreads();
  for (int m = 0; m < 3; ++m) {
    const float* Wt = a.w + a.off.t_li2[m];
    net::mm(IN + m * S2 * cin, cin, S2, cin, Wt, C, C, Wt + cin * C, G + m * S2 * C, C);
  }
  __syncthreads();
  const Geo geo = torso_geo(c);
  for (int l = 0; l < c.torso_layers; ++l) {
    const Mha mh = mha_at(a.w + a.off.t_layer0 + l * a.off.t_layer, C, C, c.torso_heads, c.torso_d, c.torso_ff);
    for (int pr = 0; pr < 3; ++pr) {
      const int m1 = pr, m2 = pr == 2 ? 0 : pr + 1;
      float* save = a.act + ((g * c.torso_layers + l) * 3 + pr) * T2 * C;
      for (int it = threadIdx.x; it < T2 * C; it += NT) {
        const float v = G[net::pair_row(it / C, S, S, m1, m2) * C + it % C];
        X[it] = v;
        save[it] = v;
      }
      __syncthreads();
      if constexpr (CHUNKED) {
        for (int s0 = 0; s0 < S; s0 += chunk) {
          const int r0 = s0 * 2 * S * C;
          mha_fwd(torso_geo(c, S - s0 < chunk ? S - s0 : chunk), mh, X + r0, X + r0, OUT + r0, SCR);
        }
      } else {
        mha_fwd(geo, mh, X, X, OUT, SCR);
      }
      for (int it = threadIdx.x; it < T2 * C; it += NT) G[net::pair_row(it / C, S, S, m1, m2) * C + it % C] = OUT[it];
      __syncthreads();
    }
  }
  float* out = a.ee + g * 3 * S2 * C;
  for (int it = threadIdx.x; it < 3 * S2 * C; it += NT) out[it] = G[net::ee_row(it / C, S, S) * C + it % C];
}

__global__ void __launch_bounds__(NT) train_torso_fwd_kernel(Args a) { torso_fwd<false>(a, 0); }
__global__ void __launch_bounds__(NT) train_torso_fwd_chunk_kernel(Args a, int chunk) { torso_fwd<true>(a, chunk); }

// ---- kernel 2: the decoder, the losses, the decoder's backward (decode, tg_train_common.h) --------------------------
// A whole game's ee, dL/dee and saved block inputs in LDS, the cross-attention on all n_steps positions at once.
// KV (S = TG_NET_WIDE_S): the cross-attention without keys and values (scr_plan_kv).
template <bool KV>
struct WholeGame {
  __device__ DPlan plan(const tg_net_config& c) const { return KV ? dplan_kv(c) : dplan(c); }
  __device__ float* xs(const Args&, float* lds, const DPlan& L) const { return lds + L.XS; }
  __device__ void game(const Args& a, int64_t g, float* lds, const DPlan& L, const float*& EE, float*& DEE) const {
    const int JC = 3 * a.c.S * a.c.S * a.c.c;
    float* ee = lds + L.EE;
    DEE = lds + L.DEE;
    for (int it = threadIdx.x; it < JC; it += NT) {
      ee[it] = a.ee[g * JC + it];
      DEE[it] = 0.f;
    }
    EE = ee;
  }
  __device__ void cross_fwd(const Geo& g2, const Mha& w, const float* X, const float* EE, float* OUT, float* sc) const {
    mha_fwd<KV>(g2, w, X, EE, OUT, sc);
  }
  __device__ void cross_bwd(const Geo& g2, const Mha& w, const GMha& gw, const float* X, const float* EE,
                            const float* dOut, float* dX, float* DEE, float* sc) const {
    mha_bwd<KV>(g2, w, gw, X, EE, dOut, dX, DEE, sc);
  }
  __device__ void game_done(const Args& a, int64_t g, const float* DEE) const {
    const int JC = 3 * a.c.S * a.c.S * a.c.c;
    for (int it = threadIdx.x; it < JC; it += NT) a.dee[g * JC + it] = DEE[it];
  }
};

__global__ void __launch_bounds__(NT) train_decode_kernel(Args a) { decode(a, WholeGame<false>{}); }
__global__ void __launch_bounds__(NT) train_decode_kv_kernel(Args a) { decode(a, WholeGame<true>{}); }

// ---- kernel 3: the torso backward -----------------------------------------------------------------------------------
// CHUNKED: as torso_fwd; the chunks of a pair add their weight gradients to the slab one after another, in order.
template <bool CHUNKED>
__device__ inline void torso_bwd(const Args& a, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int S = c.S, S2 = S * S, T2 = 2 * S2, C = c.c, cin = S * c.T + 1;
  const TPlan L = CHUNKED ? tplan(c, chunk) : tplan(c);
  float *DG = lds + L.G, *IN = lds + L.IN, *X = lds + L.X, *DO = lds + L.DO, *DXP = lds + L.DX, *SS = lds + L.SS,
        *DP = lds + L.DP, *SCR = lds + L.SCR;
  float* gs = a.slabs + static_cast<int64_t>(blockIdx.x) * a.off.total;
  for (int64_t i = threadIdx.x; i < a.off.emb; i += NT) gs[i] = 0.f;
  __syncthreads();
  const Geo geo = torso_geo(c);
  int64_t ga, gz;
  game_range(a, ga, gz);
  for (int64_t g = ga; g < gz; ++g) {
    const float* dee = a.dee + g * 3 * S2 * C;
    for (int it = threadIdx.x; it < 3 * S2 * C; it += NT) DG[net::ee_row(it / C, S, S) * C + it % C] = dee[it];
    net::torso_inputs(c, a.off, a.w, a.frames, a.frames_i8, a.scalars, g, S, 0, IN);
    for (int q = threadIdx.x; q < c.dim_s; q += NT) SS[q] = a.scalars[g * c.dim_s + q];
    __syncthreads();
    for (int l = c.torso_layers - 1; l >= 0; --l) {
      const int64_t lo = a.off.t_layer0 + l * a.off.t_layer;
      const Mha mh = mha_at(a.w + lo, C, C, c.torso_heads, c.torso_d, c.torso_ff);
      const GMha gm = mha_at(gs + lo, C, C, c.torso_heads, c.torso_d, c.torso_ff);
      for (int pr = 2; pr >= 0; --pr) {
        const int m1 = pr, m2 = pr == 2 ? 0 : pr + 1;
        const float* save = a.act + ((g * c.torso_layers + l) * 3 + pr) * T2 * C;
        for (int it = threadIdx.x; it < T2 * C; it += NT) {
          X[it] = save[it];
          DO[it] = DG[net::pair_row(it / C, S, S, m1, m2) * C + it % C];
          DXP[it] = 0.f;
        }
        __syncthreads();
        if constexpr (CHUNKED) {
          for (int s0 = 0; s0 < S; s0 += chunk) {
            const int r0 = s0 * 2 * S * C;
            mha_bwd(torso_geo(c, S - s0 < chunk ? S - s0 : chunk), mh, gm, X + r0, X + r0, DO + r0, DXP + r0, DXP + r0,
                    SCR);
          }
        } else {
          mha_bwd(geo, mh, gm, X, X, DO, DXP, DXP, SCR);
        }
        for (int it = threadIdx.x; it < T2 * C; it += NT) DG[net::pair_row(it / C, S, S, m1, m2) * C + it % C] = DXP[it];
        __syncthreads();
      }
    }
    // G[m] = IN[m] li2[m] + b;  IN[m][tok][cin-1] = scalars . li1[m][:, tok] + b
    for (int m = 0; m < 3; ++m) {
      const int64_t o2 = a.off.t_li2[m];
      wgrad(IN + m * S2 * cin, cin, DG + m * S2 * C, C, S2, cin, C, gs + o2, C, gs + o2 + cin * C);
    }
    for (int it = threadIdx.x; it < 3 * S2; it += NT) {
      const int m = it / S2, tok = it % S2;
      const float* wr = a.w + a.off.t_li2[m] + (cin - 1) * C;
      const float* dg = DG + (m * S2 + tok) * C;
      float s = 0.f;
      for (int ch = 0; ch < C; ++ch) s = fmaf(dg[ch], wr[ch], s);
      DP[it] = s;
    }
    __syncthreads();
    for (int m = 0; m < 3; ++m) {
      const int64_t o1 = a.off.t_li1[m];
      wgrad(SS, c.dim_s, DP + m * S2, S2, 1, c.dim_s, S2, gs + o1, S2, gs + o1 + c.dim_s * S2);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NT) train_torso_bwd_kernel(Args a) { torso_bwd<false>(a, 0); }
__global__ void __launch_bounds__(NT) train_torso_bwd_chunk_kernel(Args a, int chunk) { torso_bwd<true>(a, chunk); }

}  // namespace train
}  // namespace tg

namespace {

int check_train_cfg(const char* fn, const tg_net_config* c) {
  if (int rc = tg_net_check(c)) return rc;
  if (c->S == TG_NET_WIDE2_S)  // not by these kernels (a whole game per workgroup); tg_train_sliced.hip trains this size
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: training at dim_3d=%d (TG_NET_WIDE2_S) is not built; inference and self-play only", fn,
                            c->S);
  const bool wide = tg::train::wide(*c);  // there the torso fits when one sequence at a time does
  const size_t lt = (wide ? tg::train::tplan(*c, 1) : tg::train::tplan(*c)).total * sizeof(float),
               ld = (wide ? tg::train::dplan_kv(*c) : tg::train::dplan(*c)).total * sizeof(float);
  if (lt > tg::kMaxDynamicLds || ld > tg::kMaxDynamicLds)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: the training LDS plan needs %zu (torso) / %zu (decoder) bytes > 160 KiB per workgroup",
                            fn, lt, ld);
  return TG_OK;
}

// the workspace: ee, dL/dee, the saved pair inputs, the per-game losses and flags, one slab per decoder workgroup
tg::train::Ws ws_whole(const tg_net_config& c, int64_t B) {
  return tg::train::ws_plan(c, B, tg::train::partials(B), false, false);
}

// The four launches of one call: the torso forward, the decoder, the torso backward when a gradient is wanted, the
// reduction.  lt, ld: the LDS bytes of the torso kernels and of the decoder; chunk: the chunked torso kernels' argument.
template <auto FWD, auto DEC, auto BWD, class... Chunk>
int launch_all(const char* fn, const tg::train::Args& a, size_t lt, size_t ld, hipStream_t st, Chunk... chunk) {
  const unsigned NT = tg::net::NT, P = static_cast<unsigned>(a.P);
  const int gb = a.grad ? static_cast<int>((a.off.total + NT - 1) / NT) : 0;
  if (int rc = lds_opt_in<FWD>(fn, lt)) return rc;
  if (int rc = lds_opt_in<DEC>(fn, ld)) return rc;
  if (int rc = lds_opt_in<BWD>(fn, lt)) return rc;
  if (int rc = launch(fn, FWD, static_cast<unsigned>(a.B), NT, lt, st, a, chunk...)) return rc;
  if (int rc = launch(fn, DEC, P, NT, ld, st, a)) return rc;
  if (a.grad)
    if (int rc = launch(fn, BWD, P, NT, lt, st, a, chunk...)) return rc;
  return launch(fn, tg::train::train_reduce_kernel, static_cast<unsigned>(gb + 1), NT, 0, st, a, gb);
}

}  // namespace

extern "C" {

int tg_net_train_check(const tg_net_config* cfg) { return check_train_cfg("tg_net_train_check", cfg); }

int tg_net_train_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes) {
  const char* fn = "tg_net_train_workspace_size";
  return tg::train::workspace_size(fn, check_train_cfg(fn, cfg), cfg, B, bytes, ws_whole);
}

// AlphaTensor.fwd_train (model.py:326-345) in train mode, the weighted loss and its backward (training.py:431-437)
int tg_net_loss_grad(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                     int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value, int64_t B,
                     float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                     const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, float* grad,
                     float* losses, uint32_t* status, tg_stream_t stream) {
  using namespace tg::train;
  const char* fn = "tg_net_loss_grad";
  if (int rc = check_train_cfg(fn, cfg)) return rc;
  Call k;
  if (int rc = prepare_call(fn, *cfg, ws_whole, theta, pos_fix, frames, frames_is_i8, scalars, g_action, g_value, B,
                            weight_pol, weight_val, dropout_p, seed, call, keep_in, keep_out, workspace, workspace_bytes,
                            grad, losses, status, k))
    return rc;
  k.a.P = partials(B);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide(*cfg)) {
    const int chunk = torso_chunk(*cfg);
    return launch_all<train_torso_fwd_chunk_kernel, train_decode_kv_kernel, train_torso_bwd_chunk_kernel>(
        fn, k.a, tplan(*cfg, chunk).total * sizeof(float), dplan_kv(*cfg).total * sizeof(float), st, chunk);
  }
  return launch_all<train_torso_fwd_kernel, train_decode_kernel, train_torso_bwd_kernel>(
      fn, k.a, tplan(*cfg).total * sizeof(float), dplan(*cfg).total * sizeof(float), st);
}

}  // extern "C"
