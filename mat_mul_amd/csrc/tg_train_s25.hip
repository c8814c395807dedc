// The training loss and gradient at S = TG_NET_WIDE3_S (include/tensor_game_train_s25.h).  gfx950 only; part of
// libtensorgame.so.
//
// The four launches of tg_train_sliced.hip with a decoder cut once more, because at n_steps = 75 and J = 1875 keys
// neither attention block of the decoder fits a workgroup's LDS beside the per-game rows:
//   - train_torso_fwd_slice_kernel, train_torso_bwd_slice_kernel (tg_train_sliced.hip) and train_reduce_kernel as there.
//   - train_decode_s25_kernel: Pd workgroups, tg_train_common.h's decoder body over Game25.  The self-attention block runs
//     over chunks of nqs query positions against the keys up to the chunk's last row (causal: later keys have no weight);
//     the cross-attention block over chunks of nqx query positions against one layer-normed copy of ee in LDS, with
//     dL/d ln2(ee) in a J x c accumulator of the workgroup's own in the workspace and ln2's backward into dL/dee over
//     tiles of keys after the last chunk.
// No float atomics: a slab element, a dL/dee row, a saved block input and an accumulator element are only ever written
// by one workgroup, between barriers.
#include "../../include/tensor_game_train_s25.h"
#include "../../include/tensor_game_net_s25.h"
#include "tg_train_slices.h"

namespace tg {
namespace train {

constexpr int kLnTile = 256;  // keys per tile of ln2's backward into dL/dee (2 * kLnTile floats of scratch)

// ---- LDS plans --------------------------------------------------------------------------------------------------------
// the self-attention block on nq query positions, keys and values of all n_steps
__host__ __device__ inline Geo self_geo25(const tg_net_config& c, int nq) {
  Geo g = self_geo(c);
  g.Lx = nq;
  return g;
}

// the cross-attention block on nq query positions, ln2(ee) and its gradient held by the caller
__host__ __device__ inline Geo cross_geo25(const tg_net_config& c, int nq) {
  Geo g = cross_geo(c);
  g.Lx = nq;
  return g;
}

// floats behind the per-game rows: the self-attention block's scratch; ln2(ee) (J x c) and the cross-attention block's
__host__ __device__ inline int self_scr25(const tg_net_config& c, int nq) { return scr_plan(self_geo25(c, nq)).total; }
__host__ __device__ inline int cross_scr25(const tg_net_config& c, int nq) {
  return 3 * c.S * c.S * c.c + scr_plan_kv<true>(cross_geo25(c, nq)).total;
}

// the decoder kernel: dplan's per-game rows without ee, dL/dee and the saved block inputs, and the larger of the two
// blocks' needs (they run one after the other)
__host__ __device__ inline DPlan dplan25(const tg_net_config& c, int nqs, int nqx) {
  DPlan p = dplan_with(c, false, 0);
  const int s1 = self_scr25(c, nqs), s2 = cross_scr25(c, nqx);
  p.total = p.SCR + (s1 > s2 ? s1 : s2);
  return p;
}

struct Chunks25 {
  int nqs, nqx;  // query positions per chunk of the self- and of the cross-attention; 0: not even one fits
};

// The one plan function: per block the fewest chunks whose plan fits, evened out (tg_train_sliced.hip's decoder_chunk).
inline Chunks25 decoder_chunks25(const tg_net_config& c) {
  const int rows = dplan_with(c, false, 0).SCR, room = kMaxDynamicLds / static_cast<int>(sizeof(float)) - rows;
  const auto even = [&](int n) {
    if (n == 0) return 0;
    const int chunks = (c.n_steps + n - 1) / n;
    return (c.n_steps + chunks - 1) / chunks;
  };
  int ns = c.n_steps, nx = c.n_steps;
  while (ns > 0 && self_scr25(c, ns) > room) --ns;
  while (nx > 0 && cross_scr25(c, nx) > room) --nx;
  return Chunks25{even(ns), even(nx)};
}

struct Ws25 {  // byte offsets into the workspace: tg_train_sliced.hip's parts and the accumulators
  WsSliced s;
  int64_t dyn, total;
};

inline Ws25 ws_plan25(const tg_net_config& c, int64_t B) {
  Ws25 w;
  w.s = ws_plan_sliced(c, B);
  w.dyn = w.s.total;
  w.total = w.dyn + round256(4LL * partials(B) * 3 * c.S * c.S * c.c);
  return w;
}

// ---- launch 2: the decoder, the losses, the decoder's backward --------------------------------------------------------
// ee, dL/dee and the saved block inputs as SlicedGame keeps them; both attention blocks by chunks of query positions,
// which add their weight gradients to the slab one after another, in position order.
struct Game25 {
  float *xs_all, *dyn_all;
  int nqs, nqx;
  __device__ DPlan plan(const tg_net_config& c) const { return dplan25(c, nqs, nqx); }
  __device__ float* xs(const Args& a, float*, const DPlan&) const {
    return xs_all + static_cast<int64_t>(blockIdx.x) * a.c.blocks * 2 * a.c.n_steps * a.c.W;
  }
  __device__ void game(const Args& a, int64_t g, float*, const DPlan&, const float*& EE, float*& DEE) const {
    const int JC = 3 * a.c.S * a.c.S * a.c.c;
    EE = a.ee + g * JC;
    DEE = a.dee + g * JC;
    for (int it = threadIdx.x; it < JC; it += NT) DEE[it] = 0.f;
  }
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
  __device__ void game_done(const Args&, int64_t, const float*) const {}
};

static_assert(has_self_hooks<Game25>::value, "decode must run Game25's self-attention chunks: the plan has no other room");

__global__ void __launch_bounds__(NT) train_decode_s25_kernel(Args a, float* xs, float* dyn, int nqs, int nqx) {
  decode(a, Game25{xs, dyn, nqs, nqx});
}

}  // namespace train
}  // namespace tg

namespace {

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
  const int rows = tg::train::dplan_with(*c, false, 0).SCR;
  const size_t lt = tg::train::tplan_slice(*c).total * sizeof(float),
               ls = (rows + tg::train::self_scr25(*c, 1)) * sizeof(float),
               lx = (rows + tg::train::cross_scr25(*c, 1)) * sizeof(float);
  if (lt > tg::kMaxDynamicLds || ls > tg::kMaxDynamicLds || lx > tg::kMaxDynamicLds)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: the S = 25 training LDS plan needs %zu (torso) / %zu (decoder, self-attention) / %zu "
                            "(decoder, cross-attention) bytes > 160 KiB per workgroup",
                            fn, lt, ls, lx);
  return TG_OK;
}

}  // namespace

extern "C" {

int tg_net_train_s25_check(const tg_net_config* cfg) { return check_s25_cfg("tg_net_train_s25_check", cfg); }

int tg_net_train_s25_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes) {
  const char* fn = "tg_net_train_s25_workspace_size";
  if (int rc = check_s25_cfg(fn, cfg)) return rc;
  if (B < 1 || B > (1LL << 24)) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld outside [1, 2^24]", fn, (long long)B);
  if (!bytes) return tg_internal_fail(TG_ERR_INVALID, "%s: null output", fn);
  *bytes = tg::train::ws_plan25(*cfg, B).total;
  return TG_OK;
}

int tg_net_loss_grad_s25(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                         int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value, int64_t B,
                         float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                         const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, float* grad,
                         float* losses, uint32_t* status, tg_stream_t stream) {
  using namespace tg::train;
  const char* fn = "tg_net_loss_grad_s25";
  if (int rc = check_s25_cfg(fn, cfg)) return rc;
  if (int rc = check_call(fn, theta, pos_fix, frames, frames_is_i8, scalars, g_action, g_value, B, weight_pol, weight_val,
                          dropout_p, workspace, grad, losses, status))
    return rc;
  const Ws25 ws = ws_plan25(*cfg, B);
  if (workspace_bytes < ws.total)
    return tg_internal_fail(TG_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes,
                            (long long)ws.total);
  Args a = call_args(*cfg, theta, pos_fix, frames, frames_is_i8, scalars, g_action, g_value, B, weight_pol, weight_val,
                     dropout_p, seed, call, keep_in, keep_out, grad, losses, status);
  char* base = static_cast<char*>(workspace);
  a.ee = reinterpret_cast<float*>(base + ws.s.ee);
  a.dee = reinterpret_cast<float*>(base + ws.s.dee);
  a.act = reinterpret_cast<float*>(base + ws.s.act);
  a.gl = reinterpret_cast<float*>(base + ws.s.gl);
  a.flags = reinterpret_cast<int*>(base + ws.s.flags);
  a.slabs = reinterpret_cast<float*>(base + ws.s.slabs);
  float *xs = reinterpret_cast<float*>(base + ws.s.xs), *dyn = reinterpret_cast<float*>(base + ws.dyn);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned NT = tg::net::NT;
  const int Pd = partials(B), Pt = torso_partials(*cfg, B);
  const Chunks25 ch = decoder_chunks25(*cfg);
  const size_t lt = tplan_slice(*cfg).total * sizeof(float), ld = dplan25(*cfg, ch.nqs, ch.nqx).total * sizeof(float);
  const int gb = grad ? static_cast<int>((a.off.total + NT - 1) / NT) : 0;
  if (int rc = lds_opt_in<train_torso_fwd_slice_kernel>(fn, lt)) return rc;
  if (int rc = lds_opt_in<train_decode_s25_kernel>(fn, ld)) return rc;
  if (int rc = lds_opt_in<train_torso_bwd_slice_kernel>(fn, lt)) return rc;
  a.P = Pd;  // launch 2's game runs
  if (int rc = launch(fn, train_torso_fwd_slice_kernel, static_cast<unsigned>(B * cfg->S), NT, lt, st, a)) return rc;
  if (int rc = launch(fn, train_decode_s25_kernel, static_cast<unsigned>(Pd), NT, ld, st, a, xs, dyn, ch.nqs, ch.nqx))
    return rc;
  a.P = Pt;  // launch 3's unit runs and the slabs launch 4 sums
  if (grad)
    if (int rc = launch(fn, train_torso_bwd_slice_kernel, static_cast<unsigned>(Pt), NT, lt, st, a, Pd)) return rc;
  return launch(fn, train_reduce_kernel, static_cast<unsigned>(gb + 1), NT, 0, st, a, gb);
}

}  // extern "C"
