// The training loss and gradient at S = TG_NET_WIDE2_S (include/tensor_game_train_sliced.h) and at S = TG_NET_WIDE3_S
// (include/tensor_game_train_s25.h).  gfx950 only; part of libtensorgame.so.
//
// The four launches of tg_train.hip cut to fit a workgroup's LDS at 3 x 256 torso rows and J = 768 keys, on the building
// blocks of tg_train_common.h:
//   - train_torso_fwd_slice_kernel: one workgroup per (game, slice i), the torso forward on the slice's 3S rows; before
//     each attention pair it saves the pair's 2S x c input rows where tg_train.hip's torso keeps them, and it writes its
//     3S rows of ee.
//   - train_decode_sliced_kernel: Pd workgroups, tg_train_common.h's decoder body with a game's ee, dL/dee and saved block
//     inputs in the workspace and the cross-attention block over chunks of nq decoder positions (SlicedGame).
//   - train_torso_bwd_slice_kernel: Pt workgroups, each a contiguous run of (game, slice) units in order, the pairs in
//     reverse, each recomputed from its saved input, into slab p.
//   - train_reduce_kernel over the Pt slabs.
// S = TG_NET_WIDE3_S takes the same torso kernels (they take S at run time) and a decoder cut once more, because at
// n_steps = 75 and J = 1875 keys neither attention block of the decoder fits a workgroup's LDS beside the per-game rows:
//   - train_decode_s25_kernel: Pd workgroups, the decoder body over Game25.  The self-attention block runs over chunks of
//     nqs query positions against the keys up to the chunk's last row (causal: later keys have no weight); the
//     cross-attention block over chunks of nqx query positions against one layer-normed copy of ee in LDS, with
//     dL/d ln2(ee) in a J x c accumulator of the workgroup's own in the workspace and ln2's backward into dL/dee over
//     tiles of keys after the last chunk.
// No float atomics: a slab element, a dL/dee row, a saved block input and an accumulator element are only ever written
// by one workgroup, between barriers.
#include "../../include/tensor_game_net_s25.h"
#include "../../include/tensor_game_train_s25.h"
#include "../../include/tensor_game_train_sliced.h"
#include "tg_train_common.h"

namespace tg {
namespace train {

constexpr int kLnTile = 256;  // keys per tile of ln2's backward into dL/dee (2 * kLnTile floats of scratch)

// ---- LDS plans --------------------------------------------------------------------------------------------------------
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

// the self-attention block on nq query positions, keys and values of all n_steps
__host__ __device__ inline Geo self_geo25(const tg_net_config& c, int nq) {
  Geo g = self_geo(c);
  g.Lx = nq;
  return g;
}

// the cross-attention block on nq query positions
__host__ __device__ inline Geo cross_geo(const tg_net_config& c, int nq) {
  Geo g = cross_geo(c);
  g.Lx = nq;
  return g;
}

// S = TG_NET_WIDE2_S's decoder kernel: dplan's per-game rows without ee, dL/dee and the saved block inputs, and the larger
// of the self-attention's scratch and the cross-attention's for nq positions without keys and values
__host__ __device__ inline DPlan dplan_sliced(const tg_net_config& c, int nq) {
  return dplan_with(c, false, scr_plan_kv(cross_geo(c, nq)).total);
}

// Decoder positions per chunk of its cross-attention (even_chunk).
inline int decoder_chunk(const tg_net_config& c) {
  return even_chunk(c.n_steps, [&](int n) { return dplan_sliced(c, n).total; });
}

// S = TG_NET_WIDE3_S, floats behind the per-game rows: the self-attention block's scratch; ln2(ee) (J x c), which the
// caller holds with its gradient, and the cross-attention block's
__host__ __device__ inline int self_scr25(const tg_net_config& c, int nq) { return scr_plan(self_geo25(c, nq)).total; }
__host__ __device__ inline int cross_scr25(const tg_net_config& c, int nq) {
  return 3 * c.S * c.S * c.c + scr_plan_kv<true>(cross_geo(c, nq)).total;
}

// its decoder kernel: the same per-game rows, and the larger of the two blocks' needs (they run one after the other)
__host__ __device__ inline DPlan dplan25(const tg_net_config& c, int nqs, int nqx) {
  DPlan p = dplan_with(c, false, 0);
  const int s1 = self_scr25(c, nqs), s2 = cross_scr25(c, nqx);
  p.total = p.SCR + (s1 > s2 ? s1 : s2);
  return p;
}

struct Chunks25 {
  int nqs, nqx;  // query positions per chunk of the self- and of the cross-attention; 0: not even one fits
};

// The one plan function of S = TG_NET_WIDE3_S's decoder: even_chunk per block.
inline Chunks25 decoder_chunks25(const tg_net_config& c) {
  const int rows = dplan_with(c, false, 0).SCR;
  return Chunks25{even_chunk(c.n_steps, [&](int n) { return rows + self_scr25(c, n); }),
                  even_chunk(c.n_steps, [&](int n) { return rows + cross_scr25(c, n); })};
}

inline int torso_partials(const tg_net_config& c, int64_t B) {
  const int64_t units = B * c.S;
  return static_cast<int>(units < TG_NET_TRAIN_PARTIALS ? units : TG_NET_TRAIN_PARTIALS);
}

// ---- launch 1: the torso forward of one slice, B * S workgroups -------------------------------------------------------
__global__ void __launch_bounds__(NT) train_torso_fwd_slice_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int S = c.S, L2 = 2 * S, C = c.c, cin = S * c.T + 1;
  const int64_t T2 = 2LL * S * S, g = blockIdx.x / S;
  const int i = blockIdx.x % S;
  const TPlan L = tplan_slice(c);
  float *G = lds + L.G, *IN = lds + L.IN, *X = lds + L.X, *OUT = lds + L.DO, *SCR = lds + L.SCR;
  net::torso_inputs(c, a.off, a.w, a.frames, a.frames_i8, a.scalars, g, 1, i, IN);
  __syncthreads();
  for (int m = 0; m < 3; ++m) {
    const float* Wt = a.w + a.off.t_li2[m];
    net::mm(IN + m * S * cin, cin, S, cin, Wt, C, C, Wt + cin * C, G + m * S * C, C);
  }
  __syncthreads();
  const Geo geo = torso_geo(c, 1);
  for (int l = 0; l < c.torso_layers; ++l) {
    const Mha mh = mha_at(a.w + a.off.t_layer0 + l * a.off.t_layer, C, C, c.torso_heads, c.torso_d, c.torso_ff);
    for (int pr = 0; pr < 3; ++pr) {
      const int m1 = pr, m2 = pr == 2 ? 0 : pr + 1;
      float* save = a.act + (((g * c.torso_layers + l) * 3 + pr) * T2 + i * L2) * C;
      for (int it = threadIdx.x; it < L2 * C; it += NT) {
        const float v = G[net::pair_row(it / C, S, 1, m1, m2) * C + it % C];
        X[it] = v;
        save[it] = v;
      }
      __syncthreads();
      mha_fwd(geo, mh, X, X, OUT, SCR);
      for (int it = threadIdx.x; it < L2 * C; it += NT) G[net::pair_row(it / C, S, 1, m1, m2) * C + it % C] = OUT[it];
      __syncthreads();
    }
  }
  float* out = a.ee + (g * 3 * S * S + i * 3 * S) * C;  // ee_row is the identity on a slice's rows
  for (int it = threadIdx.x; it < 3 * S * C; it += NT) out[it] = G[it];
}

// ---- launch 2: the decoder, the losses, the decoder's backward --------------------------------------------------------
// What both sizes' game strategies keep in the workspace: ee and dL/dee of the game, the saved block inputs in this
// workgroup's part of xs.
struct WorkspaceGame {
  float* xs_all;
  __device__ float* xs(const Args& a, float*, const DPlan&) const {
    return xs_all + static_cast<int64_t>(blockIdx.x) * a.c.blocks * 2 * a.c.n_steps * a.c.W;
  }
  __device__ void game(const Args& a, int64_t g, float*, const DPlan&, const float*& EE, float*& DEE) const {
    const int JC = 3 * a.c.S * a.c.S * a.c.c;
    EE = a.ee + g * JC;
    DEE = a.dee + g * JC;
    for (int it = threadIdx.x; it < JC; it += NT) DEE[it] = 0.f;
  }
  __device__ void game_done(const Args&, int64_t, const float*) const {}
};

// The chunk loops below are written out, each with its own row count: behind a helper that hands a callback the chunk's
// first row and row count, or one that returns the chunk's Geo, the decoder kernels come out with other instructions.
//
// S = TG_NET_WIDE2_S: the cross-attention block over chunks of nq decoder positions.  Every step of it is row-wise in the
// positions given ee, the chunks add their weight gradients to the slab and their dL/dee to the game's rows one after
// another, in position order.
struct SlicedGame : WorkspaceGame {
  int nq;
  __device__ DPlan plan(const tg_net_config& c) const { return dplan_sliced(c, nq); }
  __device__ void cross_fwd(const Geo& g2, const Mha& w, const float* X, const float* EE, float* OUT, float* sc) const {
    for (int r0 = 0; r0 < g2.Lx; r0 += nq) {
      Geo q = g2;
      q.Lx = g2.Lx - r0 < nq ? g2.Lx - r0 : nq;
      mha_fwd<true, true>(q, w, X + r0 * g2.c1, EE, OUT + r0 * g2.c1, sc);
    }
  }
  __device__ void cross_bwd(const Geo& g2, const Mha& w, const GMha& gw, const float* X, const float* EE,
                            const float* dOut, float* dX, float* DEE, float* sc) const {
    for (int r0 = 0; r0 < g2.Lx; r0 += nq) {
      Geo q = g2;
      q.Lx = g2.Lx - r0 < nq ? g2.Lx - r0 : nq;
      mha_bwd<true, true>(q, w, gw, X + r0 * g2.c1, EE, dOut + r0 * g2.c1, dX + r0 * g2.c1, DEE, sc);
    }
  }
};

__global__ void __launch_bounds__(NT) train_decode_sliced_kernel(Args a, float* xs, int nq) {
  decode(a, SlicedGame{{xs}, nq});
}

// S = TG_NET_WIDE3_S: both attention blocks by chunks of query positions, which add their weight gradients to the slab
// one after another, in position order.
struct Game25 : WorkspaceGame {
  float* dyn_all;
  int nqs, nqx;
  __device__ DPlan plan(const tg_net_config& c) const { return dplan25(c, nqs, nqx); }
  // rows r0 .. r0 + n - 1 attend to the keys 0 .. r0 + n - 1; X is both the queries' rows and the keys'
  __device__ void self_fwd(const Geo& g1, const Mha& w, const float* X, float* OUT, float* sc) const {
    for (int r0 = 0; r0 < g1.Lx; r0 += nqs) {
      Geo q = g1;
      q.Lx = g1.Lx - r0 < nqs ? g1.Lx - r0 : nqs;
      q.Ly = r0 + q.Lx;
      mha_fwd(q, w, X + r0 * g1.c1, X, OUT + r0 * g1.c1, sc);
    }
  }
  __device__ void self_bwd(const Geo& g1, const Mha& w, const GMha& gw, const float* X, const float* dOut, float* dX,
                           float* sc) const {
    for (int r0 = 0; r0 < g1.Lx; r0 += nqs) {
      Geo q = g1;
      q.Lx = g1.Lx - r0 < nqs ? g1.Lx - r0 : nqs;
      q.Ly = r0 + q.Lx;
      mha_bwd(q, w, gw, X + r0 * g1.c1, X, dOut + r0 * g1.c1, dX + r0 * g1.c1, dX, sc);
    }
  }
  // sc: ln2(ee) (J x c2), then the chunks' scratch
  __device__ void cross_fwd(const Geo& g2, const Mha& w, const float* X, const float* EE, float* OUT, float* sc) const {
    float* YN = sc;
    sc += g2.Ly * g2.c2;
    net::layernorm(EE, g2.c2, g2.Ly, g2.c2, w.ln2w, w.ln2b, YN, g2.c2);
    __syncthreads();
    for (int r0 = 0; r0 < g2.Lx; r0 += nqx) {
      Geo q = g2;
      q.Lx = g2.Lx - r0 < nqx ? g2.Lx - r0 : nqx;
      mha_fwd<true, true, true>(q, w, X + r0 * g2.c1, YN, OUT + r0 * g2.c1, sc);
    }
  }
  __device__ void cross_bwd(const Geo& g2, const Mha& w, const GMha& gw, const float* X, const float* EE,
                            const float* dOut, float* dX, float* DEE, float* sc) const {
    const int JC = g2.Ly * g2.c2;
    float *YN = sc, *DYN = dyn_all + static_cast<int64_t>(blockIdx.x) * JC;
    sc += JC;
    net::layernorm(EE, g2.c2, g2.Ly, g2.c2, w.ln2w, w.ln2b, YN, g2.c2);
    for (int it = threadIdx.x; it < JC; it += NT) DYN[it] = 0.f;
    __syncthreads();
    for (int r0 = 0; r0 < g2.Lx; r0 += nqx) {
      Geo q = g2;
      q.Lx = g2.Lx - r0 < nqx ? g2.Lx - r0 : nqx;
      mha_bwd<true, true, true>(q, w, gw, X + r0 * g2.c1, YN, dOut + r0 * g2.c1, dX + r0 * g2.c1, DYN, sc);
    }
    ln_bwd_tiles(EE, g2.Ly, g2.c2, w.ln2w, DYN, DEE, gw.ln2w, gw.ln2b, sc, kLnTile);
  }
};

static_assert(has_self_hooks<Game25>::value, "decode must run Game25's self-attention chunks: the plan has no other room");

__global__ void __launch_bounds__(NT) train_decode_s25_kernel(Args a, float* xs, float* dyn, int nqs, int nqx) {
  decode(a, Game25{{xs}, dyn, nqs, nqx});
}

// ---- launch 3: the torso backward -------------------------------------------------------------------------------------
// a.P = Pt workgroups; Pd: the workgroups of launch 2, whose slabs hold the policy and value part already.
__global__ void __launch_bounds__(NT) train_torso_bwd_slice_kernel(Args a, int Pd) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int S = c.S, S2 = S * S, L2 = 2 * S, C = c.c, cin = S * c.T + 1;
  const int64_t T2 = 2LL * S2;
  const TPlan L = tplan_slice(c);
  float *DG = lds + L.G, *IN = lds + L.IN, *X = lds + L.X, *DO = lds + L.DO, *DXP = lds + L.DX, *SS = lds + L.SS,
        *DP = lds + L.DP, *SCR = lds + L.SCR;
  float* gs = a.slabs + static_cast<int64_t>(blockIdx.x) * a.off.total;
  const int64_t zero_to = static_cast<int>(blockIdx.x) < Pd ? a.off.emb : a.off.total;
  for (int64_t k = threadIdx.x; k < zero_to; k += NT) gs[k] = 0.f;
  __syncthreads();
  const Geo geo = torso_geo(c, 1);
  const int64_t units = a.B * S, u0 = units * blockIdx.x / a.P, u1 = units * (blockIdx.x + 1) / a.P;
  for (int64_t u = u0; u < u1; ++u) {
    const int64_t g = u / S;
    const int i = static_cast<int>(u % S);
    const float* dee = a.dee + (g * 3 * S2 + i * 3 * S) * C;
    for (int it = threadIdx.x; it < 3 * S * C; it += NT) DG[it] = dee[it];
    net::torso_inputs(c, a.off, a.w, a.frames, a.frames_i8, a.scalars, g, 1, i, IN);
    for (int q = threadIdx.x; q < c.dim_s; q += NT) SS[q] = a.scalars[g * c.dim_s + q];
    __syncthreads();
    for (int l = c.torso_layers - 1; l >= 0; --l) {
      const int64_t lo = a.off.t_layer0 + l * a.off.t_layer;
      const Mha mh = mha_at(a.w + lo, C, C, c.torso_heads, c.torso_d, c.torso_ff);
      const GMha gm = mha_at(gs + lo, C, C, c.torso_heads, c.torso_d, c.torso_ff);
      for (int pr = 2; pr >= 0; --pr) {
        const int m1 = pr, m2 = pr == 2 ? 0 : pr + 1;
        const float* save = a.act + (((g * c.torso_layers + l) * 3 + pr) * T2 + i * L2) * C;
        for (int it = threadIdx.x; it < L2 * C; it += NT) {
          X[it] = save[it];
          DO[it] = DG[net::pair_row(it / C, S, 1, m1, m2) * C + it % C];
          DXP[it] = 0.f;
        }
        __syncthreads();
        mha_bwd(geo, mh, gm, X, X, DO, DXP, DXP, SCR);
        for (int it = threadIdx.x; it < L2 * C; it += NT) DG[net::pair_row(it / C, S, 1, m1, m2) * C + it % C] = DXP[it];
        __syncthreads();
      }
    }
    // G[m] = IN[m] li2[m] + b on the slice's S rows;  IN[m][j][cin-1] = scalars . li1[m][:, i*S + j] + b
    for (int m = 0; m < 3; ++m) {
      const int64_t o2 = a.off.t_li2[m];
      wgrad(IN + m * S * cin, cin, DG + m * S * C, C, S, cin, C, gs + o2, C, gs + o2 + cin * C);
    }
    for (int it = threadIdx.x; it < 3 * S; it += NT) {
      const float* wr = a.w + a.off.t_li2[it / S] + (cin - 1) * C;
      const float* dg = DG + it * C;
      float s = 0.f;
      for (int ch = 0; ch < C; ++ch) s = fmaf(dg[ch], wr[ch], s);
      DP[it] = s;
    }
    __syncthreads();
    for (int m = 0; m < 3; ++m) {  // the slice's columns tok = i*S + j of li1[m] and of its bias
      const int64_t o1 = a.off.t_li1[m] + i * S;
      wgrad(SS, c.dim_s, DP + m * S, S, 1, c.dim_s, S, gs + o1, S2, gs + o1 + c.dim_s * S2);
    }
    __syncthreads();
  }
}

}  // namespace train
}  // namespace tg

namespace {

using namespace tg::train;

int check_sliced_cfg(const char* fn, const tg_net_config* c) {
  if (int rc = tg_net_check(c)) return rc;
  if (c->S != TG_NET_WIDE2_S)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: dim_3d=%d is not TG_NET_WIDE2_S=%d; every other size trains through tg_net_loss_grad "
                            "(tensor_game_train.h)",
                            fn, c->S, TG_NET_WIDE2_S);
  // the decoder fits when one position at a time does
  const size_t lt = tplan_slice(*c).total * sizeof(float), ld = dplan_sliced(*c, 1).total * sizeof(float);
  if (lt > tg::kMaxDynamicLds || ld > tg::kMaxDynamicLds)
    return tg_internal_fail(
        TG_ERR_UNSUPPORTED,
        "%s: the sliced training LDS plan needs %zu (torso) / %zu (decoder) bytes > 160 KiB per workgroup", fn, lt, ld);
  return TG_OK;
}

int check_s25_cfg(const char* fn, const tg_net_config* c) {
  if (c && c->S != TG_NET_WIDE3_S) {
    if (int rc = tg_net_check(c)) return rc;
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: dim_3d=%d is not TG_NET_WIDE3_S=%d; the other sizes train through tg_net_loss_grad "
                            "(tensor_game_train.h) and tg_net_loss_grad_sliced (tensor_game_train_sliced.h)",
                            fn, c->S, TG_NET_WIDE3_S);
  }
  if (int rc = tg_net_s25_check(c)) return rc;
  // the decoder fits when one position at a time does in either block
  const int rows = dplan_with(*c, false, 0).SCR;
  const size_t lt = tplan_slice(*c).total * sizeof(float), ls = (rows + self_scr25(*c, 1)) * sizeof(float),
               lx = (rows + cross_scr25(*c, 1)) * sizeof(float);
  if (lt > tg::kMaxDynamicLds || ls > tg::kMaxDynamicLds || lx > tg::kMaxDynamicLds)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: the S = 25 training LDS plan needs %zu (torso) / %zu (decoder, self-attention) / %zu "
                            "(decoder, cross-attention) bytes > 160 KiB per workgroup",
                            fn, lt, ls, lx);
  return TG_OK;
}

// the workspace: tg_train.hip's parts, the saved block inputs of each decoder workgroup and one slab per torso workgroup;
// at S = TG_NET_WIDE3_S also the accumulator of each decoder workgroup
Ws ws_sliced(const tg_net_config& c, int64_t B) { return ws_plan(c, B, torso_partials(c, B), true, false); }
Ws ws_s25(const tg_net_config& c, int64_t B) { return ws_plan(c, B, torso_partials(c, B), true, true); }

// The four launches of one call.  DEC: the size's decoder kernel, ld: its LDS bytes, more: its arguments after a.
template <auto DEC, class... More>
int launch_sliced(const char* fn, Args a, size_t ld, hipStream_t st, More... more) {
  const unsigned NT = tg::net::NT;
  const int Pd = partials(a.B), Pt = torso_partials(a.c, a.B);
  const size_t lt = tplan_slice(a.c).total * sizeof(float);
  const int gb = a.grad ? static_cast<int>((a.off.total + NT - 1) / NT) : 0;
  if (int rc = lds_opt_in<train_torso_fwd_slice_kernel>(fn, lt)) return rc;
  if (int rc = lds_opt_in<DEC>(fn, ld)) return rc;
  if (int rc = lds_opt_in<train_torso_bwd_slice_kernel>(fn, lt)) return rc;
  a.P = Pd;  // launch 2's game runs
  if (int rc = launch(fn, train_torso_fwd_slice_kernel, static_cast<unsigned>(a.B * a.c.S), NT, lt, st, a)) return rc;
  if (int rc = launch(fn, DEC, static_cast<unsigned>(Pd), NT, ld, st, a, more...)) return rc;
  a.P = Pt;  // launch 3's unit runs and the slabs launch 4 sums
  if (a.grad)
    if (int rc = launch(fn, train_torso_bwd_slice_kernel, static_cast<unsigned>(Pt), NT, lt, st, a, Pd)) return rc;
  return launch(fn, train_reduce_kernel, static_cast<unsigned>(gb + 1), NT, 0, st, a, gb);
}

}  // namespace

extern "C" {

int tg_net_train_sliced_check(const tg_net_config* cfg) { return check_sliced_cfg("tg_net_train_sliced_check", cfg); }

int tg_net_train_sliced_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes) {
  const char* fn = "tg_net_train_sliced_workspace_size";
  return workspace_size(fn, check_sliced_cfg(fn, cfg), cfg, B, bytes, ws_sliced);
}

int tg_net_loss_grad_sliced(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                            int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value,
                            int64_t B, float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                            const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes,
                            float* grad, float* losses, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_net_loss_grad_sliced";
  if (int rc = check_sliced_cfg(fn, cfg)) return rc;
  Call k;
  if (int rc = prepare_call(fn, *cfg, ws_sliced, theta, pos_fix, frames, frames_is_i8, scalars, g_action, g_value, B,
                            weight_pol, weight_val, dropout_p, seed, call, keep_in, keep_out, workspace, workspace_bytes,
                            grad, losses, status, k))
    return rc;
  const int nq = decoder_chunk(*cfg);
  return launch_sliced<train_decode_sliced_kernel>(fn, k.a, dplan_sliced(*cfg, nq).total * sizeof(float),
                                                   static_cast<hipStream_t>(stream), k.xs, nq);
}

int tg_net_train_s25_check(const tg_net_config* cfg) { return check_s25_cfg("tg_net_train_s25_check", cfg); }

int tg_net_train_s25_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes) {
  const char* fn = "tg_net_train_s25_workspace_size";
  return workspace_size(fn, check_s25_cfg(fn, cfg), cfg, B, bytes, ws_s25);
}

int tg_net_loss_grad_s25(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                         int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value, int64_t B,
                         float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                         const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, float* grad,
                         float* losses, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_net_loss_grad_s25";
  if (int rc = check_s25_cfg(fn, cfg)) return rc;
  Call k;
  if (int rc = prepare_call(fn, *cfg, ws_s25, theta, pos_fix, frames, frames_is_i8, scalars, g_action, g_value, B,
                            weight_pol, weight_val, dropout_p, seed, call, keep_in, keep_out, workspace, workspace_bytes,
                            grad, losses, status, k))
    return rc;
  const Chunks25 ch = decoder_chunks25(*cfg);
  return launch_sliced<train_decode_s25_kernel>(fn, k.a, dplan25(*cfg, ch.nqs, ch.nqx).total * sizeof(float),
                                                static_cast<hipStream_t>(stream), k.xs, k.dyn, ch.nqs, ch.nqx);
}

}  // extern "C"
