// Shared by tg_train.hip (training, whole games) and tg_train_sliced.hip (training at S = TG_NET_WIDE2_S and at
// S = TG_NET_WIDE3_S): one attention block's geometry, LDS scratch, forward and backward; the kernels' arguments,
// workspace and LDS plans; the decoder's body (forward, losses, backward) over a policy that says where ee, dL/dee and
// the saved block inputs live and how the attention blocks run; the host path of the entries (the argument rules, the
// workspace's size, the kernels' arguments); and the fixed-order reduction.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "../../include/tensor_game.h"
#include "../../include/tensor_game_net.h"
#include "../../include/tensor_game_train.h"
#include "tg_device.h"
#include "tg_host.h"
#include "tg_net_common.h"

namespace tg {
namespace train {

using net::Mha;
using net::MhaT;
using net::mha_at;
using net::mha_size;
using net::NT;
using net::Off;
using GMha = MhaT<float*>;

// ---- one attention block: geometry and LDS scratch ------------------------------------------------------------------
// nseq independent sequences; x rows s*Lx + a (c1 wide), y rows s*Ly + b (c2 wide).  causal: the x rows are the last Lx
// of the Ly positions (all of them where Lx == Ly) and row a attends to the keys b <= a + Ly - Lx.
struct Geo {
  int nseq, Lx, Ly, c1, c2, H, d, ff, causal;
};

struct Scr {  // float offsets into an attention block's scratch
  int XN, YN, H1, MN, DH1, DXN, DYN, ST, F, DF, Q, K, V, O, DO, DQ, DK, DV, P, DS, total;
};

// YEXT: the caller holds the layer-normed y (it passes it as Y) and the accumulator of its gradient (it passes it as dY,
// zeroes it and takes it through ln2's backward itself), so the scratch has neither and ST is for the x rows (the
// cross-attention by chunks at S = TG_NET_WIDE3_S).
template <bool YEXT = false>
__host__ __device__ inline Scr scr_plan(const Geo& g) {
  const int N = g.nseq * g.Lx, M = g.nseq * g.Ly, MY = YEXT ? 0 : M, NM = N > MY ? N : MY, PS = g.nseq * g.Lx * g.Ly;
  Scr s;
  s.XN = 0;
  s.YN = s.XN + N * g.c1;
  s.H1 = s.YN + MY * g.c2;
  s.MN = s.H1 + N * g.c1;
  s.DH1 = s.MN + N * g.c1;
  s.DXN = s.DH1 + N * g.c1;
  s.DYN = s.DXN + N * g.c1;
  s.ST = s.DYN + MY * g.c2;
  const int u = s.ST + 2 * NM;  // the MLP's (F, DF) and the head's buffers share the rest
  s.F = u;
  s.DF = s.F + N * g.ff;
  s.Q = u;
  s.K = s.Q + N * g.d;
  s.V = s.K + M * g.d;
  s.O = s.V + M * g.d;
  s.DO = s.O + N * g.d;
  s.DQ = s.DO + N * g.d;
  s.DK = s.DQ + N * g.d;
  s.DV = s.DK + M * g.d;
  s.P = s.DV + M * g.d;
  s.DS = s.P + PS;
  const int heads_end = s.DS + PS, mlp_end = s.DF + N * g.ff;
  s.total = heads_end > mlp_end ? heads_end : mlp_end;
  return s;
}

// The same block without keys and values (the decoder's cross-attention at S = TG_NET_WIDE_S, 243 keys): as in
// tg_net.hip's decoder, a head's scores are (Wk_h^T q_a) . yn_b and its output Wv_h (sum_b p_ab yn_b), so a head holds
// c2-wide vectors per query (QK, YB and their gradients DQK, DYB) instead of M x d keys, values and their gradients.
// XN .. DF sit where scr_plan puts them; the head's buffers start where scr_plan's do; DO reuses O and DQ reuses Q.
struct ScrKV {
  int Q, O, QK, YB, DYB, DQK, P, DS, total;
};

template <bool YEXT = false>
__host__ __device__ inline ScrKV scr_plan_kv(const Geo& g) {
  const Scr s = scr_plan<YEXT>(g);
  const int N = g.nseq * g.Lx, PS = g.nseq * g.Lx * g.Ly;
  ScrKV k;
  k.Q = s.Q;
  k.O = k.Q + N * g.d;
  k.QK = k.O + N * g.d;
  k.YB = k.QK + N * g.c2;
  k.DYB = k.YB + N * g.c2;
  k.DQK = k.DYB + N * g.c2;
  k.P = k.DQK + N * g.c2;
  k.DS = k.P + PS;
  const int heads_end = k.DS + PS, mlp_end = s.DF + N * g.ff;
  k.total = heads_end > mlp_end ? heads_end : mlp_end;
  return k;
}

// ---- building blocks (all threads call them; each ends without a barrier) -------------------------------------------
// Y[r][i] = (Y[r][i] +) sum_o X[r][o] * Wt[i][o]   (X @ Wt^T, Wt rows contiguous)
__device__ inline void mmT(const float* X, int ldx, int R, int O, const float* __restrict__ Wt, int ldw, int I, float* Y,
                           int ldy, bool acc) {
  for (int it = threadIdx.x; it < R * I; it += NT) {
    const int i = it % I, r = it / I;
    const float* x = X + r * ldx;
    const float* w = Wt + static_cast<int64_t>(i) * ldw;
    float s = 0.f;
#pragma unroll 4
    for (int o = 0; o < O; ++o) s = fmaf(x[o], w[o], s);
    Y[r * ldy + i] = acc ? Y[r * ldy + i] + s : s;
  }
}

// gb[o] += sum_r Bm[r][o] (rows in order)
__device__ inline void bgrad(const float* Bm, int ldb, int R, int O, float* gb) {
  for (int o = threadIdx.x; o < O; o += NT) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += Bm[r * ldb + o];
    gb[o] += s;
  }
}

// gW[i][o] += sum_r A[r][i] * Bm[r][o] (rows in order); gb[o] += sum_r Bm[r][o] when gb.  gW, gb: a partial slab.
__device__ inline void wgrad(const float* A, int lda, const float* Bm, int ldb, int R, int I, int O, float* gW, int ldg,
                             float* gb) {
  for (int it = threadIdx.x; it < I * O; it += NT) {
    const int o = it % O, i = it / O;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s = fmaf(A[r * lda + i], Bm[r * ldb + o], s);
    gW[static_cast<int64_t>(i) * ldg + o] += s;
  }
  if (gb) bgrad(Bm, ldb, R, O, gb);
}

__device__ inline float gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ inline float gelu_grad(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}

// The backward of LayerNorm (eps 1e-5, biased variance) over R rows of n <= 64: dX[r] += J^T dY[r]; then (after a
// barrier) gw[i] += sum_r dY[r][i] xhat[r][i], gb[i] += sum_r dY[r][i].  st: 2R floats.
__device__ inline void ln_bwd(const float* X, int R, int n, const float* __restrict__ w, const float* dY, float* dX,
                              float* gw, float* gb, float* st) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5;
  const float inv_n = 1.f / static_cast<float>(n);
  for (int r = team; r < R; r += NT / 32) {
    const float* x = X + r * n;
    const float x0 = lane < n ? x[lane] : 0.f, x1 = lane + 32 < n ? x[lane + 32] : 0.f;
    float s = x0 + x1;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, 32);
    const float mean = s / static_cast<float>(n);
    const float d0 = lane < n ? x0 - mean : 0.f, d1 = lane + 32 < n ? x1 - mean : 0.f;
    float v = d0 * d0 + d1 * d1;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 32);
    const float rstd = 1.f / sqrtf(v / static_cast<float>(n) + 1e-5f);
    const float h0 = d0 * rstd, h1 = d1 * rstd;
    const float g0 = lane < n ? dY[r * n + lane] * w[lane] : 0.f;
    const float g1 = lane + 32 < n ? dY[r * n + lane + 32] * w[lane + 32] : 0.f;
    float sg = g0 + g1, sgh = g0 * h0 + g1 * h1;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
      sg += __shfl_xor(sg, m, 32);
      sgh += __shfl_xor(sgh, m, 32);
    }
    sg *= inv_n;
    sgh *= inv_n;
    if (lane < n) dX[r * n + lane] += rstd * (g0 - sg - h0 * sgh);
    if (lane + 32 < n) dX[r * n + lane + 32] += rstd * (g1 - sg - h1 * sgh);
    if (lane == 0) {
      st[2 * r] = mean;
      st[2 * r + 1] = rstd;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NT) {
    float sw = 0.f, sb = 0.f;
    for (int r = 0; r < R; ++r) {
      const float g = dY[r * n + i];
      sw = fmaf(g, (X[r * n + i] - st[2 * r]) * st[2 * r + 1], sw);
      sb += g;
    }
    gw[i] += sw;
    gb[i] += sb;
  }
}

// ln_bwd over tiles of `tile` rows, so that st holds 2 * tile floats whatever R is; the tiles add to gw and gb in row
// order.  Ends with a barrier.
__device__ inline void ln_bwd_tiles(const float* X, int R, int n, const float* __restrict__ w, const float* dY, float* dX,
                                    float* gw, float* gb, float* st, int tile) {
  for (int r0 = 0; r0 < R; r0 += tile) {
    ln_bwd(X + r0 * n, R - r0 < tile ? R - r0 : tile, n, w, dY + r0 * n, dX + r0 * n, gw, gb, st);
    __syncthreads();
  }
}

// softmax in place over the rows of the scores P (nseq x Lx x Ly), one thread per row; when causal, row a takes its
// first a + 1 entries and the rest become 0
__device__ inline void softmax_masked(const Geo& g, float* P) {
  const int Lx = g.Lx, Ly = g.Ly;
  for (int row = threadIdx.x; row < g.nseq * Lx; row += NT) {
    float* p = P + row * Ly;
    const int n = g.causal ? row % Lx + 1 + (Ly - Lx) : Ly;
    float m = p[0];
    for (int j = 1; j < n; ++j) m = fmaxf(m, p[j]);
    float s = 0.f;
    for (int j = 0; j < n; ++j) {
      const float e = expf(p[j] - m);
      p[j] = e;
      s += e;
    }
    const float inv = 1.f / s;
    for (int j = 0; j < n; ++j) p[j] *= inv;
    for (int j = n; j < Ly; ++j) p[j] = 0.f;
  }
}

// dS = P (dP - rowsum(P dP)) / sqrt(d) in place over the rows of DS = dP, one thread per row
__device__ inline void softmax_bwd(const Geo& g, const float* P, float* DS) {
  const int Ly = g.Ly;
  const float sd = sqrtf(static_cast<float>(g.d));
  for (int row = threadIdx.x; row < g.nseq * g.Lx; row += NT) {
    const float* p = P + row * Ly;
    float* ds = DS + row * Ly;
    float s = 0.f;
    for (int b = 0; b < Ly; ++b) s = fmaf(p[b], ds[b], s);
    for (int b = 0; b < Ly; ++b) ds[b] = p[b] * (ds[b] - s) / sd;
  }
}

// softmax_masked and softmax_bwd for rows of many keys (the cross-attention's J = 768 at S = TG_NET_WIDE2_S; never causal):
// a team of 32 lanes per row, as tg_net.hip's softmax_rows_team.  Lane l takes entries l, l + 32, ... in that order and the
// 32 partial results meet in a fixed butterfly, so a row's bits depend on neither the rows around it nor the launch.
__device__ inline void softmax_team(const Geo& g, float* P) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5, Ly = g.Ly;
  for (int row = team; row < g.nseq * g.Lx; row += NT / 32) {
    float* p = P + row * Ly;
    float m = -INFINITY;
    for (int j = lane; j < Ly; j += 32) m = fmaxf(m, p[j]);
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 32));
    float s = 0.f;
    for (int j = lane; j < Ly; j += 32) {
      const float e = expf(p[j] - m);
      p[j] = e;
      s += e;
    }
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) s += __shfl_xor(s, x, 32);
    const float inv = 1.f / s;
    for (int j = lane; j < Ly; j += 32) p[j] *= inv;
  }
}

__device__ inline void softmax_bwd_team(const Geo& g, const float* P, float* DS) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5, Ly = g.Ly;
  const float sd = sqrtf(static_cast<float>(g.d));
  for (int row = team; row < g.nseq * g.Lx; row += NT / 32) {
    const float* p = P + row * Ly;
    float* ds = DS + row * Ly;
    float s = 0.f;
    for (int b = lane; b < Ly; b += 32) s = fmaf(p[b], ds[b], s);
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) s += __shfl_xor(s, x, 32);
    for (int b = lane; b < Ly; b += 32) ds[b] = p[b] * (ds[b] - s) / sd;
  }
}

// One head's forward: Q (N x d), K, V (M x d), the attention P (nseq x Lx x Ly, 0 above the diagonal when causal) and
// O = P V (N x d).
__device__ inline void head_fwd(const Geo& g, const Mha& w, int h, const float* XN, const float* YN, float* sc) {
  const Scr S = scr_plan(g);
  const int N = g.nseq * g.Lx, M = g.nseq * g.Ly, d = g.d, hd = g.H * d, Lx = g.Lx, Ly = g.Ly;
  float *Q = sc + S.Q, *K = sc + S.K, *V = sc + S.V, *P = sc + S.P, *O = sc + S.O;
  net::mm(XN, g.c1, N, g.c1, w.q + h * d, hd, d, nullptr, Q, d);
  mmT(YN, g.c2, M, g.c2, w.k + h * d * g.c2, g.c2, d, K, d, false);
  net::mm(YN, g.c2, M, g.c2, w.v + h * d, hd, d, nullptr, V, d);
  __syncthreads();
  const float sd = sqrtf(static_cast<float>(d));
  for (int it = threadIdx.x; it < g.nseq * Lx * Ly; it += NT) {
    const int b = it % Ly, a = (it / Ly) % Lx, s = it / (Lx * Ly);
    if (g.causal && b > a + (Ly - Lx)) continue;
    const float* q = Q + (s * Lx + a) * d;
    const float* k = K + (s * Ly + b) * d;
    float acc = 0.f;
#pragma unroll 8
    for (int e = 0; e < d; ++e) acc = fmaf(q[e], k[e], acc);
    P[it] = acc / sd;
  }
  __syncthreads();
  softmax_masked(g, P);
  __syncthreads();
  for (int it = threadIdx.x; it < N * d; it += NT) {
    const int e = it % d, r = it / d, s = r / Lx;
    const float* pr = P + r * Ly;
    const float* v = V + s * Ly * d + e;
    float acc = 0.f;
    for (int b = 0; b < Ly; ++b) acc = fmaf(pr[b], v[b * d], acc);
    O[it] = acc;
  }
}

// One head's forward without keys and values (scr_plan_kv): Q (N x d), QK = Q Wk_h (N x c2), the attention P as in
// head_fwd, YB = P YN (N x c2) and O = YB Wv_h (N x d).  TEAM: the softmax by teams of 32 lanes (softmax_team).
template <bool TEAM = false, bool YEXT = false>
__device__ inline void head_fwd_kv(const Geo& g, const Mha& w, int h, const float* XN, const float* YN, float* sc) {
  const ScrKV S = scr_plan_kv<YEXT>(g);
  const int N = g.nseq * g.Lx, d = g.d, hd = g.H * d, c2 = g.c2, Lx = g.Lx, Ly = g.Ly;
  float *Q = sc + S.Q, *QK = sc + S.QK, *YB = sc + S.YB, *P = sc + S.P, *O = sc + S.O;
  net::mm(XN, g.c1, N, g.c1, w.q + h * d, hd, d, nullptr, Q, d);
  __syncthreads();
  net::mm(Q, d, N, d, w.k + h * d * c2, c2, c2, nullptr, QK, c2);  // k stored [hd][c2]: row e of head h is Wk_h[e]
  __syncthreads();
  const float sd = sqrtf(static_cast<float>(d));
  for (int it = threadIdx.x; it < g.nseq * Lx * Ly; it += NT) {
    const int b = it % Ly, a = (it / Ly) % Lx, s = it / (Lx * Ly);
    if (g.causal && b > a) continue;
    const float* qk = QK + (s * Lx + a) * c2;
    const float* y = YN + (s * Ly + b) * c2;
    float acc = 0.f;
#pragma unroll 8
    for (int i = 0; i < c2; ++i) acc = fmaf(qk[i], y[i], acc);
    P[it] = acc / sd;
  }
  __syncthreads();
  if constexpr (TEAM) softmax_team(g, P);
  else softmax_masked(g, P);
  __syncthreads();
  for (int it = threadIdx.x; it < N * c2; it += NT) {
    const int i = it % c2, r = it / c2, s = r / Lx;
    const float* pr = P + r * Ly;
    const float* y = YN + s * Ly * c2 + i;
    float acc = 0.f;
    for (int b = 0; b < Ly; ++b) acc = fmaf(pr[b], y[b * c2], acc);
    YB[it] = acc;
  }
  __syncthreads();
  net::mm(YB, c2, N, c2, w.v + h * d, hd, d, nullptr, O, d);
}

// MultiHeadAttention.forward (model.py:44-67) up to li2: XN, YN, H1 = X + li1(heads), MN = ln3(H1), F = li2(MN) (before
// the GELU).  With OUT, also OUT = H1 + li3(gelu(F)) (F then holds gelu(F)).  KV: the heads without keys and values
// (scr_plan_kv), TEAM: their softmax by teams.  Ends with a barrier.
template <bool KV = false, bool TEAM = false, bool YEXT = false>
__device__ inline void mha_fwd(const Geo& g, const Mha& w, const float* X, const float* Y, float* OUT, float* sc) {
  const Scr S = scr_plan<YEXT>(g);
  const int N = g.nseq * g.Lx, M = g.nseq * g.Ly, c1 = g.c1, d = g.d;
  float *XN = sc + S.XN, *YNS = sc + S.YN, *H1 = sc + S.H1, *MN = sc + S.MN, *F = sc + S.F,
        *O = sc + (KV ? scr_plan_kv<YEXT>(g).O : S.O);
  const float* YN = YEXT ? Y : YNS;
  net::layernorm(X, c1, N, c1, w.ln1w, w.ln1b, XN, c1);
  if constexpr (!YEXT) net::layernorm(Y, g.c2, M, g.c2, w.ln2w, w.ln2b, YNS, g.c2);
  for (int it = threadIdx.x; it < N * c1; it += NT) H1[it] = X[it] + w.li1b[it % c1];
  __syncthreads();
  for (int h = 0; h < g.H; ++h) {
    if constexpr (KV) head_fwd_kv<TEAM, YEXT>(g, w, h, XN, YN, sc);
    else head_fwd(g, w, h, XN, YN, sc);
    __syncthreads();
    net::mm(O, d, N, d, w.li1w + h * d * c1, c1, c1, nullptr, H1, c1, net::ACT_NONE, H1, nullptr, c1);
    __syncthreads();
  }
  net::layernorm(H1, c1, N, c1, w.ln3w, w.ln3b, MN, c1);
  __syncthreads();
  net::mm(MN, c1, N, c1, w.li2w, g.ff, g.ff, w.li2b, F, g.ff, OUT ? net::ACT_GELU : net::ACT_NONE);
  __syncthreads();
  if (OUT) {
    net::mm(F, g.ff, N, g.ff, w.li3w, c1, c1, w.li3b, OUT, c1, net::ACT_NONE, H1, nullptr, c1);
    __syncthreads();
  }
}

// The backward of head h without keys and values (scr_plan_kv), from DH1 = dL/dH1: recomputes the head's forward, adds
// the gradients of li1's slice, Wq_h, Wk_h and Wv_h into gw, dL/dXN into DXN and dL/dYN into DYN.  Ends with a barrier.
//   dO = DH1 li1_h^T;  dYB = dO Wv_h^T, dWv_h += YB^T dO;  dP_ab = dYB_a . yn_b;  dS = P (dP - rowsum(P dP)) / sqrt(d);
//   dQK = dS YN, dWk_h += Q^T dQK, dQ = dQK Wk_h;  dYN_b += sum_a (P_ab dYB_a + dS_ab QK_a).
template <bool TEAM = false, bool YEXT = false>
__device__ inline void head_bwd_kv(const Geo& g, const Mha& w, const GMha& gw, int h, const float* XN, const float* YN,
                                   const float* DH1, float* DXN, float* DYN, float* sc) {
  const ScrKV S = scr_plan_kv<YEXT>(g);
  const int N = g.nseq * g.Lx, M = g.nseq * g.Ly, c1 = g.c1, c2 = g.c2, d = g.d, hd = g.H * d, Lx = g.Lx, Ly = g.Ly;
  float *Q = sc + S.Q, *O = sc + S.O, *QK = sc + S.QK, *YB = sc + S.YB, *DYB = sc + S.DYB, *DQK = sc + S.DQK,
        *P = sc + S.P, *DS = sc + S.DS;
  float *DO = O, *DQ = Q;
  head_fwd_kv<TEAM, YEXT>(g, w, h, XN, YN, sc);
  __syncthreads();
  wgrad(O, d, DH1, c1, N, d, c1, gw.li1w + h * d * c1, c1, nullptr);
  __syncthreads();
  mmT(DH1, c1, N, c1, w.li1w + h * d * c1, c1, d, DO, d, false);
  __syncthreads();
  mmT(DO, d, N, d, w.v + h * d, hd, c2, DYB, c2, false);
  wgrad(YB, c2, DO, d, N, c2, d, gw.v + h * d, hd, nullptr);
  __syncthreads();
  for (int it = threadIdx.x; it < g.nseq * Lx * Ly; it += NT) {  // dP, into DS
    const int b = it % Ly, a = (it / Ly) % Lx, s = it / (Lx * Ly);
    const float* dy = DYB + (s * Lx + a) * c2;
    const float* y = YN + (s * Ly + b) * c2;
    float acc = 0.f;
    for (int i = 0; i < c2; ++i) acc = fmaf(dy[i], y[i], acc);
    DS[it] = acc;
  }
  __syncthreads();
  if constexpr (TEAM) softmax_bwd_team(g, P, DS);
  else softmax_bwd(g, P, DS);
  __syncthreads();
  for (int it = threadIdx.x; it < N * c2; it += NT) {
    const int i = it % c2, r = it / c2, s = r / Lx;
    const float* ds = DS + r * Ly;
    float acc = 0.f;
    for (int b = 0; b < Ly; ++b) acc = fmaf(ds[b], YN[(s * Ly + b) * c2 + i], acc);
    DQK[it] = acc;
  }
  for (int it = threadIdx.x; it < M * c2; it += NT) {
    const int i = it % c2, rb = it / c2, s = rb / Ly, b = rb % Ly;
    float acc = 0.f;
    for (int a = 0; a < Lx; ++a) {
      const int r = s * Lx + a;
      acc = fmaf(P[r * Ly + b], DYB[r * c2 + i], acc);
      acc = fmaf(DS[r * Ly + b], QK[r * c2 + i], acc);
    }
    DYN[it] += acc;
  }
  __syncthreads();
  wgrad(Q, d, DQK, c2, N, d, c2, gw.k + h * d * c2, c2, nullptr);
  __syncthreads();
  mmT(DQK, c2, N, c2, w.k + h * d * c2, c2, d, DQ, d, false);
  __syncthreads();
  wgrad(XN, c1, DQ, d, N, c1, d, gw.q + h * d, hd, nullptr);
  mmT(DQ, d, N, d, w.q + h * d, hd, c1, DXN, c1, true);
  __syncthreads();
}

// The backward of OUT = MHA(X, Y) for dOut: dX += dOUT/dX^T dOut, dY += ..., weight gradients into gw (a partial slab).
// dY may be dX (self-attention).  Recomputes the forward.  KV: the heads without keys and values, TEAM: their softmax by
// teams.  X, Y, dX and dY may lie in global memory that only this workgroup writes.  With YEXT, Y is ln2(y) and dY the
// accumulator of its gradient (see scr_plan).  Ends with a barrier.
template <bool KV = false, bool TEAM = false, bool YEXT = false>
__device__ inline void mha_bwd(const Geo& g, const Mha& w, const GMha& gw, const float* X, const float* Y,
                               const float* dOut, float* dX, float* dY, float* sc) {
  const Scr S = scr_plan<YEXT>(g);
  const int N = g.nseq * g.Lx, M = g.nseq * g.Ly, c1 = g.c1, c2 = g.c2, d = g.d, hd = g.H * d, ff = g.ff;
  const int Lx = g.Lx, Ly = g.Ly;
  float *XN = sc + S.XN, *YNS = sc + S.YN, *H1 = sc + S.H1, *MN = sc + S.MN, *DH1 = sc + S.DH1, *DXN = sc + S.DXN,
        *DYN = YEXT ? dY : sc + S.DYN, *ST = sc + S.ST, *F = sc + S.F, *DF = sc + S.DF;
  const float* YN = YEXT ? Y : YNS;
  float *Q = sc + S.Q, *K = sc + S.K, *V = sc + S.V, *O = sc + S.O, *DO = sc + S.DO, *DQ = sc + S.DQ, *DK = sc + S.DK,
        *DV = sc + S.DV, *P = sc + S.P, *DS = sc + S.DS;
  mha_fwd<KV, TEAM, YEXT>(g, w, X, Y, nullptr, sc);
  // the MLP: dF = (dOut li3^T) * gelu'(F)
  for (int it = threadIdx.x; it < N * ff; it += NT) {
    const int j = it % ff, r = it / ff;
    const float* dr = dOut + r * c1;
    const float* wr = w.li3w + j * c1;
    float s = 0.f;
    for (int o = 0; o < c1; ++o) s = fmaf(dr[o], wr[o], s);
    DF[it] = s * gelu_grad(F[it]);
  }
  __syncthreads();
  for (int it = threadIdx.x; it < N * ff; it += NT) F[it] = gelu(F[it]);
  __syncthreads();
  wgrad(F, ff, dOut, c1, N, ff, c1, gw.li3w, c1, gw.li3b);
  wgrad(MN, c1, DF, ff, N, c1, ff, gw.li2w, ff, gw.li2b);
  mmT(DF, ff, N, ff, w.li2w, ff, c1, DXN, c1, false);  // dMN, in DXN for now
  for (int it = threadIdx.x; it < N * c1; it += NT) DH1[it] = dOut[it];
  __syncthreads();
  ln_bwd(H1, N, c1, w.ln3w, DXN, DH1, gw.ln3w, gw.ln3b, ST);
  __syncthreads();
  // the residual and li1's bias; the heads' input gradients start from 0
  for (int it = threadIdx.x; it < N * c1; it += NT) {
    dX[it] += DH1[it];
    DXN[it] = 0.f;
  }
  if constexpr (!YEXT)
    for (int it = threadIdx.x; it < M * c2; it += NT) DYN[it] = 0.f;
  bgrad(DH1, c1, N, c1, gw.li1b);
  __syncthreads();
  for (int h = 0; h < g.H; ++h) {
    if constexpr (KV) {
      head_bwd_kv<TEAM, YEXT>(g, w, gw, h, XN, YN, DH1, DXN, DYN, sc);
      continue;
    }
    head_fwd(g, w, h, XN, YN, sc);
    __syncthreads();
    wgrad(O, d, DH1, c1, N, d, c1, gw.li1w + h * d * c1, c1, nullptr);
    mmT(DH1, c1, N, c1, w.li1w + h * d * c1, c1, d, DO, d, false);
    __syncthreads();
    // dP (into DS) and dV = P^T dO
    for (int it = threadIdx.x; it < g.nseq * Lx * Ly; it += NT) {
      const int b = it % Ly, a = (it / Ly) % Lx, s = it / (Lx * Ly);
      const float* o = DO + (s * Lx + a) * d;
      const float* v = V + (s * Ly + b) * d;
      float acc = 0.f;
      for (int e = 0; e < d; ++e) acc = fmaf(o[e], v[e], acc);
      DS[it] = acc;
    }
    for (int it = threadIdx.x; it < M * d; it += NT) {
      const int e = it % d, rb = it / d, s = rb / Ly, b = rb % Ly;
      float acc = 0.f;
      for (int a = 0; a < Lx; ++a) acc = fmaf(P[(s * Lx + a) * Ly + b], DO[(s * Lx + a) * d + e], acc);
      DV[it] = acc;
    }
    __syncthreads();
    softmax_bwd(g, P, DS);
    __syncthreads();
    // dQ = dS K, dK = dS^T Q
    for (int it = threadIdx.x; it < N * d; it += NT) {
      const int e = it % d, r = it / d, s = r / Lx;
      const float* ds = DS + r * Ly;
      float acc = 0.f;
      for (int b = 0; b < Ly; ++b) acc = fmaf(ds[b], K[(s * Ly + b) * d + e], acc);
      DQ[it] = acc;
    }
    for (int it = threadIdx.x; it < M * d; it += NT) {
      const int e = it % d, rb = it / d, s = rb / Ly, b = rb % Ly;
      float acc = 0.f;
      for (int a = 0; a < Lx; ++a) acc = fmaf(DS[(s * Lx + a) * Ly + b], Q[(s * Lx + a) * d + e], acc);
      DK[it] = acc;
    }
    __syncthreads();
    wgrad(XN, c1, DQ, d, N, c1, d, gw.q + h * d, hd, nullptr);
    wgrad(DK, d, YN, c2, M, d, c2, gw.k + h * d * c2, c2, nullptr);
    wgrad(YN, c2, DV, d, M, c2, d, gw.v + h * d, hd, nullptr);
    mmT(DQ, d, N, d, w.q + h * d, hd, c1, DXN, c1, true);
    net::mm(DK, d, M, d, w.k + h * d * c2, c2, c2, nullptr, DYN, c2, net::ACT_NONE, DYN, nullptr, c2);
    __syncthreads();
    mmT(DV, d, M, d, w.v + h * d, hd, c2, DYN, c2, true);
    __syncthreads();
  }
  ln_bwd(X, N, c1, w.ln1w, DXN, dX, gw.ln1w, gw.ln1b, ST);
  __syncthreads();
  if constexpr (YEXT) return;
  ln_bwd(Y, M, c2, w.ln2w, DYN, dY, gw.ln2w, gw.ln2b, ST);
  __syncthreads();
}

// ---- arguments, workspace, LDS plans ----------------------------------------------------------------------------------
struct Args {
  tg_net_config c;
  Off off;
  const float* w;
  const float* pos_fix;
  const void* frames;
  int frames_i8;
  const float* scalars;
  const int8_t* g_action;
  const float* g_value;
  int64_t B;
  int P, need_grad;
  float wpol, wval, p, scale;
  uint32_t seed_lo, seed_hi, call_lo;
  const uint8_t* keep_in;
  uint8_t* keep_out;
  float *ee, *dee, *act, *gl, *slabs;  // workspace parts
  int* flags;
  float* grad;
  float* losses;
  uint32_t* status;
};

struct Ws {  // byte offsets into the workspace; a part a family does not have takes no room
  int64_t ee, dee, act, gl, flags, xs, slabs, dyn, total;
};

inline int64_t round256(int64_t x) { return (x + 255) / 256 * 256; }

inline int partials(int64_t B) { return static_cast<int>(B < TG_NET_TRAIN_PARTIALS ? B : TG_NET_TRAIN_PARTIALS); }

// slabs: the partial slabs of the gradient.  xs: each of the decoder's partials(B) workgroups keeps its saved block inputs
// here; dyn: each has a J x c accumulator here (tg_train_sliced.hip).
inline Ws ws_plan(const tg_net_config& c, int64_t B, int slabs, bool xs, bool dyn) {
  const int64_t J = 3LL * c.S * c.S, T2 = 2LL * c.S * c.S;
  Ws w;
  int64_t p = 0;
  w.ee = p; p += round256(4 * B * J * c.c);
  w.dee = p; p += round256(4 * B * J * c.c);
  w.act = p; p += round256(4 * B * c.torso_layers * 3 * T2 * c.c);
  w.gl = p; p += round256(4 * 2 * B);
  w.flags = p; p += round256(4 * B);
  w.xs = p; p += round256(xs ? 4LL * partials(B) * c.blocks * 2 * c.n_steps * c.W : 0);
  w.slabs = p; p += round256(4LL * slabs * net::offsets(c).total);
  w.dyn = p; p += round256(dyn ? 4LL * partials(B) * J * c.c : 0);
  w.total = p;
  return w;
}

__host__ __device__ inline Geo torso_geo(const tg_net_config& c, int nseq) {
  return Geo{nseq, 2 * c.S, 2 * c.S, c.c, c.c, c.torso_heads, c.torso_d, c.torso_ff, 0};
}
__host__ __device__ inline Geo torso_geo(const tg_net_config& c) { return torso_geo(c, c.S); }
__host__ __device__ inline Geo self_geo(const tg_net_config& c) {
  return Geo{1, c.n_steps, c.n_steps, c.W, c.W, c.heads, c.d, c.ff, 1};
}
__host__ __device__ inline Geo cross_geo(const tg_net_config& c) {
  return Geo{1, c.n_steps, 3 * c.S * c.S, c.W, c.c, c.heads, c.d, c.ff, 0};
}

struct TPlan {  // torso kernels (floats)
  int G, IN, X, DO, DX, SS, DP, SCR, total;
};

// nseq: the sequences of a pair whose attention block runs at once (the scratch's size); c.S = the whole pair
__host__ __device__ inline TPlan tplan(const tg_net_config& c, int nseq) {
  const int S2 = c.S * c.S, T2 = 2 * S2, cin = c.S * c.T + 1;
  TPlan p;
  p.G = 0;
  p.IN = p.G + 3 * S2 * c.c;
  p.X = p.IN + 3 * S2 * cin;
  p.DO = p.X + T2 * c.c;
  p.DX = p.DO + T2 * c.c;
  p.SS = p.DX + T2 * c.c;
  p.DP = p.SS + TG_NET_MAX_DIM_S;
  p.SCR = p.DP + 3 * S2;
  p.total = p.SCR + scr_plan(torso_geo(c, nseq)).total;
  return p;
}
__host__ __device__ inline TPlan tplan(const tg_net_config& c) { return tplan(c, c.S); }

struct DPlan {  // decoder kernel (floats)
  int EE, DEE, XS, X, DX, XB, MO, DXB, LG, VH, DZ, KEEP, TOK, SCR, total;
};

// resident: ee, dL/dee and the saved block inputs XS are held in LDS (otherwise they take no room: the sliced decoder of
// tg_train_sliced.hip keeps them in the workspace); cross: the cross-attention block's scratch.
__host__ __device__ inline DPlan dplan_with(const tg_net_config& c, bool resident, int cross) {
  const int J = 3 * c.S * c.S, N = c.n_steps, W = c.W, nh = c.n_hidden, nq = c.n_quantile;
  DPlan p;
  p.EE = 0;
  p.DEE = p.EE + (resident ? J * c.c : 0);
  p.XS = p.DEE + (resident ? J * c.c : 0);
  p.X = p.XS + (resident ? c.blocks * 2 * N * W : 0);
  p.DX = p.X + N * W;
  p.XB = p.DX + N * W;
  p.MO = p.XB + N * W;
  p.DXB = p.MO + N * W;
  p.LG = p.DXB + N * W;
  p.VH = p.LG + N * c.n_logits;           // a1, a2, a3, da, db (nh each), q, dq, terms (nq each), row losses (N)
  p.DZ = p.VH + 5 * nh + 3 * nq + N;      // dz0 (W)
  p.KEEP = p.DZ + W;                      // uint8 mask (blocks x 2 x N x W)
  p.TOK = p.KEEP + (c.blocks * 2 * N * W + 3) / 4;  // int: input tokens (N), targets (N), flag
  const int s1 = scr_plan(self_geo(c)).total;
  p.SCR = p.TOK + 2 * N + 1;
  p.total = p.SCR + (s1 > cross ? s1 : cross);
  return p;
}

__host__ __device__ inline DPlan dplan(const tg_net_config& c) {
  return dplan_with(c, true, scr_plan(cross_geo(c)).total);
}

// the same with the cross-attention without keys and values (scr_plan_kv)
__host__ __device__ inline DPlan dplan_kv(const tg_net_config& c) {
  return dplan_with(c, true, scr_plan_kv(cross_geo(c)).total);
}

// S = TG_NET_WIDE_S takes the kernels below made for it: the torso's attention over a chunk of a pair's sequences at a
// time, and the decoder's cross-attention without keys and values.  Every other S keeps the whole-pair kernels.
__host__ __device__ inline bool wide(const tg_net_config& c) { return c.S == TG_NET_WIDE_S; }

// The rule of every chunked loop: `total` rows in the fewest chunks whose plan fits, evened out.  floats(n): the plan's
// size at n rows per chunk.  The rows per chunk; 0 if not even one row fits.
template <class Floats>
inline int even_chunk(int total, Floats floats) {
  int n = total;
  while (n > 0 && floats(n) * sizeof(float) > static_cast<size_t>(kMaxDynamicLds)) --n;
  if (n == 0) return 0;
  const int chunks = (total + n - 1) / n;
  return (total + chunks - 1) / chunks;
}

// Sequences per chunk of the wide torso.
inline int torso_chunk(const tg_net_config& c) {
  return even_chunk(c.S, [&](int n) { return tplan(c, n).total; });
}

// Whether a game strategy of decode runs the self-attention block itself (self_fwd / self_bwd).
template <class V, class = void>
struct has_self_hooks : std::false_type {};
template <class V>
struct has_self_hooks<V, std::void_t<decltype(&V::self_fwd)>> : std::true_type {};

__device__ inline void game_range(const Args& a, int64_t& g0, int64_t& g1) {
  g0 = a.B * blockIdx.x / a.P;
  g1 = a.B * (blockIdx.x + 1) / a.P;
}

// ---- the decoder, the losses, the decoder's backward ----------------------------------------------------------------
// The body of the decoder kernels: workgroup blockIdx.x of a.P takes its run of games in order, into its slab.  V says
// where a game's ee, dL/dee and the saved block inputs live and how the cross-attention block runs:
//   DPlan plan(c)                            the LDS plan;
//   float* xs(a, lds, L)                     the saved block inputs (blocks x 2 x n_steps x W), this workgroup's own;
//   void game(a, g, lds, L, EE, DEE)         sets EE and DEE for game g (EE filled, DEE zero after the next barrier);
//   void self_fwd / self_bwd                 optional: mha_fwd / mha_bwd of the self-attention block on all n_steps
//                                            positions, where the plan has no room for scr_plan(self_geo(c));
//   void cross_fwd / cross_bwd               mha_fwd / mha_bwd of the cross-attention block on all n_steps positions;
//   void game_done(a, g, DEE)                leaves dL/dee of game g in a.dee.
template <class V>
__device__ inline void decode(const Args& a, const V& v) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int W = c.W, C = c.c, H = c.heads, d = c.d, ff = c.ff, N = c.n_steps, NL = c.n_logits;
  const int nh = c.n_hidden, nq = c.n_quantile, NB = c.blocks;
  const DPlan L = v.plan(c);
  float *XS = v.xs(a, lds, L), *X = lds + L.X, *DX = lds + L.DX, *XB = lds + L.XB, *MO = lds + L.MO, *DXB = lds + L.DXB,
        *LG = lds + L.LG, *DZ = lds + L.DZ, *SCR = lds + L.SCR;
  float *A1 = lds + L.VH, *A2 = A1 + nh, *A3 = A2 + nh, *DA = A3 + nh, *DB = DA + nh, *QV = DB + nh, *DQV = QV + nq,
        *LQ = DQV + nq, *RL = LQ + nq;
  uint8_t* KEEP = reinterpret_cast<uint8_t*>(lds + L.KEEP);
  int* TIN = reinterpret_cast<int*>(lds + L.TOK);
  int *TGT = TIN + N, *BAD = TIN + 2 * N;
  const float* wb = a.w;
  float* gs = a.slabs + static_cast<int64_t>(blockIdx.x) * a.off.total;
  const Geo g1 = self_geo(c), g2 = cross_geo(c);
  const int blkm = 2 * W + mha_size(W, W, H, d, ff);  // offset of a block's ln2 within the block
  const int nW4 = (W + 3) / 4;

  if (a.need_grad) {
    for (int64_t i = a.off.emb + threadIdx.x; i < a.off.total; i += NT) gs[i] = 0.f;
    __syncthreads();
  }
  int64_t ga, gz;
  game_range(a, ga, gz);
  for (int64_t g = ga; g < gz; ++g) {
    // ---- inputs: ee, tokens, the dropout mask, the embedded START + shifted actions
    const float* EE;
    float* DEE;
    v.game(a, g, lds, L, EE, DEE);
    if (threadIdx.x == 0) {
      int bad = 0;
      for (int t = 0; t < N; ++t) {
        const int v = a.g_action[g * N + t];
        const bool ok = v >= 0 && v < NL;
        bad |= !ok;
        TGT[t] = v;
        TIN[t] = t == 0 ? NL : (TGT[t - 1] >= 0 && TGT[t - 1] < NL ? TGT[t - 1] : NL);
      }
      *BAD = bad;
    }
    for (int it = threadIdx.x; it < NB * 2 * N * nW4; it += NT) {
      const int grp = it % nW4, t = (it / nW4) % N, bw = it / (nW4 * N);
      uint8_t k4[4];
      if (a.keep_in) {
        for (int u = 0; u < 4; ++u)
          k4[u] = grp * 4 + u < W ? (a.keep_in[((g * NB * 2 + bw) * N + t) * W + grp * 4 + u] != 0) : 0;
      } else {
        const U4 ctr{static_cast<uint32_t>(g), a.call_lo, static_cast<uint32_t>(bw),
                     static_cast<uint32_t>(t * nW4 + grp)};
        const U4 wv = philox4x32_10(ctr, a.seed_lo, a.seed_hi);
        const uint32_t ws[4] = {wv.x, wv.y, wv.z, wv.w};
        for (int u = 0; u < 4; ++u) k4[u] = static_cast<float>(ws[u] >> 8) * 5.9604644775390625e-8f >= a.p;
      }
      for (int u = 0; u < 4 && grp * 4 + u < W; ++u) {
        KEEP[(bw * N + t) * W + grp * 4 + u] = k4[u];
        if (a.keep_out) a.keep_out[((g * NB * 2 + bw) * N + t) * W + grp * 4 + u] = k4[u];
      }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < N * W; it += NT) {
      const int t = it / W, i = it % W;
      X[it] = wb[a.off.emb + TIN[t] * W + i] + wb[a.off.pos + it] + a.pos_fix[it];
    }
    __syncthreads();
    // ---- forward
    for (int b = 0; b < NB; ++b) {
      const float* bp = wb + a.off.blk0 + b * a.off.blk;
      const Mha a1 = mha_at(bp + 2 * W, W, W, H, d, ff), a2 = mha_at(bp + blkm + 2 * W, W, C, H, d, ff);
      const uint8_t *k1 = KEEP + (b * 2) * N * W, *k2 = k1 + N * W;
      float *xin = XS + b * 2 * N * W, *xmid = xin + N * W;
      for (int it = threadIdx.x; it < N * W; it += NT) xin[it] = X[it];
      net::layernorm(X, W, N, W, bp, bp + W, XB, W);
      __syncthreads();
      if constexpr (has_self_hooks<V>::value) v.self_fwd(g1, a1, XB, MO, SCR);
      else mha_fwd(g1, a1, XB, XB, MO, SCR);
      for (int it = threadIdx.x; it < N * W; it += NT) {
        const float v = XB[it] + (k1[it] ? a.scale : 0.f) * MO[it];
        X[it] = v;
        xmid[it] = v;
      }
      __syncthreads();
      net::layernorm(X, W, N, W, bp + blkm, bp + blkm + W, XB, W);
      __syncthreads();
      v.cross_fwd(g2, a2, XB, EE, MO, SCR);
      for (int it = threadIdx.x; it < N * W; it += NT) X[it] = XB[it] + (k2[it] ? a.scale : 0.f) * MO[it];
      __syncthreads();
    }
    // ---- logits, value head, losses
    for (int it = threadIdx.x; it < N * W; it += NT) XB[it] = X[it] > 0.f ? X[it] : 0.f;
    __syncthreads();
    net::mm(XB, W, N, W, wb + a.off.out, NL, NL, wb + a.off.out + W * NL, LG, NL);
    net::mm(X, W, 1, W, wb + a.off.v[0], nh, nh, wb + a.off.v[0] + W * nh, A1, nh, net::ACT_RELU);
    __syncthreads();
    net::mm(A1, nh, 1, nh, wb + a.off.v[1], nh, nh, wb + a.off.v[1] + nh * nh, A2, nh, net::ACT_RELU);
    __syncthreads();
    net::mm(A2, nh, 1, nh, wb + a.off.v[2], nh, nh, wb + a.off.v[2] + nh * nh, A3, nh, net::ACT_RELU);
    __syncthreads();
    net::mm(A3, nh, 1, nh, wb + a.off.v[3], nq, nq, wb + a.off.v[3] + nh * nq, QV, nq);
    __syncthreads();
    const bool bad = *BAD != 0;
    for (int t = threadIdx.x; t < N; t += NT) {  // cross entropy of row t; LG becomes dL/dlogits
      float* lg = LG + t * NL;
      float mx = lg[0];
      for (int l = 1; l < NL; ++l) mx = fmaxf(mx, lg[l]);
      float s = 0.f;
      for (int l = 0; l < NL; ++l) s += expf(lg[l] - mx);
      const float lse = mx + logf(s);
      RL[t] = bad ? 0.f : lse - lg[TGT[t]];
      for (int l = 0; l < NL; ++l) lg[l] = bad ? 0.f : a.wpol * (expf(lg[l] - lse) - (l == TGT[t] ? 1.f : 0.f));
    }
    const float gv = a.g_value[g], vden = static_cast<float>(a.B) * static_cast<float>(nq);
    for (int j = threadIdx.x; j < nq; j += NT) {  // quantile loss term j and its gradient
      const float tau = (static_cast<float>(j) + 0.5f) / static_cast<float>(nq);
      const float dd = gv - QV[j], ad = fabsf(dd);
      const float kk = fabsf(tau - (dd > 0.f ? 1.f : 0.f));
      LQ[j] = kk * (ad < 1.f ? 0.5f * dd * dd : ad - 0.5f);  // the loss term, summed below
      DQV[j] = -a.wval / vden * kk * fminf(fmaxf(dd, -1.f), 1.f);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float lp = 0.f, lv = 0.f;
      for (int t = 0; t < N; ++t) lp += RL[t];
      for (int j = 0; j < nq; ++j) lv += LQ[j];
      a.gl[2 * g] = lp;
      a.gl[2 * g + 1] = lv;
      a.flags[g] = bad ? static_cast<int>(TG_TRAIN_STATUS_BAD_TOKEN) : 0;
    }
    __syncthreads();
    if (!a.need_grad) continue;

    // ---- backward: logits and value head
    wgrad(XB, W, LG, NL, N, W, NL, gs + a.off.out, NL, gs + a.off.out + W * NL);
    mmT(LG, NL, N, NL, wb + a.off.out, NL, W, DX, W, false);
    wgrad(A3, nh, DQV, nq, 1, nh, nq, gs + a.off.v[3], nq, gs + a.off.v[3] + nh * nq);
    mmT(DQV, nq, 1, nq, wb + a.off.v[3], nq, nh, DA, nh, false);
    __syncthreads();
    for (int it = threadIdx.x; it < N * W; it += NT) DX[it] = X[it] > 0.f ? DX[it] : 0.f;
    for (int i = threadIdx.x; i < nh; i += NT) DA[i] = A3[i] > 0.f ? DA[i] : 0.f;
    __syncthreads();
    wgrad(A2, nh, DA, nh, 1, nh, nh, gs + a.off.v[2], nh, gs + a.off.v[2] + nh * nh);
    mmT(DA, nh, 1, nh, wb + a.off.v[2], nh, nh, DB, nh, false);
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += NT) DB[i] = A2[i] > 0.f ? DB[i] : 0.f;
    __syncthreads();
    wgrad(A1, nh, DB, nh, 1, nh, nh, gs + a.off.v[1], nh, gs + a.off.v[1] + nh * nh);
    mmT(DB, nh, 1, nh, wb + a.off.v[1], nh, nh, DA, nh, false);
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += NT) DA[i] = A1[i] > 0.f ? DA[i] : 0.f;
    __syncthreads();
    wgrad(X, W, DA, nh, 1, W, nh, gs + a.off.v[0], nh, gs + a.off.v[0] + W * nh);
    mmT(DA, nh, 1, nh, wb + a.off.v[0], nh, W, DZ, W, false);
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += NT) DX[i] += DZ[i];
    __syncthreads();
    // ---- backward: the blocks in reverse
    for (int b = NB - 1; b >= 0; --b) {
      const float* bp = wb + a.off.blk0 + b * a.off.blk;
      float* gp = gs + a.off.blk0 + b * a.off.blk;
      const Mha a1 = mha_at(bp + 2 * W, W, W, H, d, ff), a2 = mha_at(bp + blkm + 2 * W, W, C, H, d, ff);
      const GMha ga1 = mha_at(gp + 2 * W, W, W, H, d, ff), ga2 = mha_at(gp + blkm + 2 * W, W, C, H, d, ff);
      const uint8_t *k1 = KEEP + (b * 2) * N * W, *k2 = k1 + N * W;
      const float *xin = XS + b * 2 * N * W, *xmid = xin + N * W;
      // x_out = xb2 + keep2 * att2(xb2, ee), xb2 = ln2(x_mid)
      net::layernorm(xmid, W, N, W, bp + blkm, bp + blkm + W, XB, W);
      for (int it = threadIdx.x; it < N * W; it += NT) {
        MO[it] = k2[it] ? a.scale * DX[it] : 0.f;
        DXB[it] = DX[it];
      }
      __syncthreads();
      v.cross_bwd(g2, a2, ga2, XB, EE, MO, DXB, DEE, SCR);
      for (int it = threadIdx.x; it < N * W; it += NT) DX[it] = 0.f;
      __syncthreads();
      ln_bwd(xmid, N, W, bp + blkm, DXB, DX, gp + blkm, gp + blkm + W, SCR);
      __syncthreads();
      // x_mid = xb1 + keep1 * att1(xb1, xb1), xb1 = ln1(x_in)
      net::layernorm(xin, W, N, W, bp, bp + W, XB, W);
      for (int it = threadIdx.x; it < N * W; it += NT) {
        MO[it] = k1[it] ? a.scale * DX[it] : 0.f;
        DXB[it] = DX[it];
      }
      __syncthreads();
      if constexpr (has_self_hooks<V>::value) v.self_bwd(g1, a1, ga1, XB, MO, DXB, SCR);
      else mha_bwd(g1, a1, ga1, XB, XB, MO, DXB, DXB, SCR);
      for (int it = threadIdx.x; it < N * W; it += NT) DX[it] = 0.f;
      __syncthreads();
      ln_bwd(xin, N, W, bp, DXB, DX, gp, gp + W, SCR);
      __syncthreads();
    }
    // ---- the embedding and pos_enc (one thread per feature, positions in order)
    for (int i = threadIdx.x; i < W; i += NT)
      for (int t = 0; t < N; ++t) {
        gs[a.off.emb + TIN[t] * W + i] += DX[t * W + i];
        gs[a.off.pos + t * W + i] += DX[t * W + i];
      }
    v.game_done(a, g, DEE);
    __syncthreads();
  }
}

// ---- the host path of the entries (every family's, after its own check of the configuration) -----------------------
using WsPlan = Ws (*)(const tg_net_config&, int64_t);  // a family's workspace at B games

// A *_workspace_size entry; rc: the family's check of cfg.
inline int workspace_size(const char* fn, int rc, const tg_net_config* cfg, int64_t B, int64_t* bytes, WsPlan plan) {
  if (rc) return rc;
  if (B < 1 || B > (1LL << 24)) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld outside [1, 2^24]", fn, (long long)B);
  if (!bytes) return tg_internal_fail(TG_ERR_INVALID, "%s: null output", fn);
  *bytes = plan(*cfg, B).total;
  return TG_OK;
}

struct Call {
  Args a;           // the kernels' arguments, all but P
  float *xs, *dyn;  // the workspace parts that are no member of Args (the family's plan says whether it has them)
};

// A loss entry up to its launches: the argument rules in this order, the workspace's size against the family's plan,
// then the kernels' arguments.
inline int prepare_call(const char* fn, const tg_net_config& cfg, WsPlan plan, const float* theta, const float* pos_fix,
                        const void* frames, int frames_is_i8, const float* scalars, const int8_t* g_action,
                        const float* g_value, int64_t B, float weight_pol, float weight_val, float dropout_p, uint64_t seed,
                        uint64_t call, const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes,
                        float* grad, float* losses, uint32_t* status, Call& k) {
  if (B < 1 || B > (1LL << 24)) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld outside [1, 2^24]", fn, (long long)B);
  if (!(dropout_p >= 0.f && dropout_p < 1.f))
    return tg_internal_fail(TG_ERR_INVALID, "%s: dropout_p=%g outside [0, 1)", fn, static_cast<double>(dropout_p));
  if (!std::isfinite(weight_pol) || !std::isfinite(weight_val))
    return tg_internal_fail(TG_ERR_INVALID, "%s: weight_pol or weight_val is not finite", fn);
  if (frames_is_i8 != 0 && frames_is_i8 != 1)
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames_is_i8=%d (0 float32, 1 int8)", fn, frames_is_i8);
  if (!theta || !pos_fix || !frames || !scalars || !g_action || !g_value || !workspace || !losses || !status)
    return tg_internal_fail(TG_ERR_INVALID,
                            "%s: null theta, pos_fix, frames, scalars, g_action, g_value, workspace, losses or status", fn);
  if (!aligned(theta, 4) || !aligned(pos_fix, 4) || !aligned(frames, frames_is_i8 ? 1 : 4) || !aligned(scalars, 4) ||
      !aligned(g_value, 4) || !aligned(grad, 4) || !aligned(losses, 4) || !aligned(status, 4) || !aligned(workspace, 256))
    return tg_internal_fail(TG_ERR_INVALID, "%s: an argument is not aligned to its elements (workspace: 256 bytes)", fn);
  const Ws ws = plan(cfg, B);
  if (workspace_bytes < ws.total)
    return tg_internal_fail(TG_ERR_INVALID, "%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes,
                            (long long)ws.total);
  Args& a = k.a;
  a = Args{};
  a.c = cfg;
  a.off = net::offsets(cfg);
  a.w = theta;
  a.pos_fix = pos_fix;
  a.frames = frames;
  a.frames_i8 = frames_is_i8;
  a.scalars = scalars;
  a.g_action = g_action;
  a.g_value = g_value;
  a.B = B;
  a.need_grad = grad != nullptr;
  a.wpol = weight_pol;
  a.wval = weight_val;
  a.p = dropout_p;
  a.scale = 1.f / (1.f - dropout_p);
  a.seed_lo = static_cast<uint32_t>(seed);
  a.seed_hi = static_cast<uint32_t>(seed >> 32);
  a.call_lo = static_cast<uint32_t>(call);
  a.keep_in = keep_in;
  a.keep_out = keep_out;
  a.grad = grad;
  a.losses = losses;
  a.status = status;
  char* base = static_cast<char*>(workspace);
  a.ee = reinterpret_cast<float*>(base + ws.ee);
  a.dee = reinterpret_cast<float*>(base + ws.dee);
  a.act = reinterpret_cast<float*>(base + ws.act);
  a.gl = reinterpret_cast<float*>(base + ws.gl);
  a.flags = reinterpret_cast<int*>(base + ws.flags);
  a.slabs = reinterpret_cast<float*>(base + ws.slabs);
  k.xs = reinterpret_cast<float*>(base + ws.xs);
  k.dyn = reinterpret_cast<float*>(base + ws.dyn);
  return TG_OK;
}

// ---- the last launch: the partial slabs, the losses, the status -----------------------------------------------------
// static: a kernel is launched from the object that defines it, so tg_train.hip and tg_train_sliced.hip each hold one.
static __global__ void __launch_bounds__(NT) train_reduce_kernel(Args a, int grad_blocks) {
  __shared__ float sp[NT], sv[NT];
  __shared__ int sf[NT];
  if (static_cast<int>(blockIdx.x) < grad_blocks) {
    const int64_t n = a.off.total, i = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int p = 0; p < a.P; ++p) s += a.slabs[p * n + i];
    a.grad[i] = s;
    return;
  }
  float lp = 0.f, lv = 0.f;
  int f = 0;
  for (int64_t g = threadIdx.x; g < a.B; g += NT) {
    lp += a.gl[2 * g];
    lv += a.gl[2 * g + 1];
    f |= a.flags[g];
  }
  sp[threadIdx.x] = lp;
  sv[threadIdx.x] = lv;
  sf[threadIdx.x] = f;
  __syncthreads();
  for (int s = NT / 2; s >= 1; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      sp[threadIdx.x] += sp[threadIdx.x + s];
      sv[threadIdx.x] += sv[threadIdx.x + s];
      sf[threadIdx.x] |= sf[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.losses[0] = sp[0];
    a.losses[1] = sv[0] / (static_cast<float>(a.B) * static_cast<float>(a.c.n_quantile));
    a.status[0] = static_cast<uint32_t>(sf[0]);
  }
}

}  // namespace train
}  // namespace tg
