// Shared by tg_net.hip (inference) and tg_train.hip (training): the weight blob's layout of include/tensor_game_net.h,
// the workgroup-level fp32 building blocks that work on activations in LDS, and the torso's input rows and row orders.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/tensor_game_net.h"

namespace tg {
namespace net {

constexpr int NT = 256;  // threads per workgroup (every network kernel)

// the row mask of the inference kernels: row g takes part when there is no mask or its flags byte holds every `need` bit
__device__ inline bool active(const uint8_t* flags, uint8_t need, int64_t g) {
  return !flags || (flags[g] & need) == need;
}

// ---- blob layout (the header's) ---------------------------------------------------------------------------------------
// one MHA's tensors; PT = const float* for the weights, float* for a gradient slab of the same layout
template <class PT>
struct MhaT {
  PT ln1w, ln1b, ln2w, ln2b, q, k, v, li1w, li1b, ln3w, ln3b, li2w, li2b, li3w, li3b;
};
using Mha = MhaT<const float*>;

__host__ __device__ inline int64_t mha_size(int c1, int c2, int H, int d, int ff) {
  const int64_t hd = static_cast<int64_t>(H) * d;
  return 2LL * c1 + 2LL * c2 + c1 * hd + hd * c2 + c2 * hd + hd * c1 + c1 + 2LL * c1 + static_cast<int64_t>(c1) * ff +
         ff + static_cast<int64_t>(ff) * c1 + c1;
}

template <class PT>
__device__ inline MhaT<PT> mha_at(PT p, int c1, int c2, int H, int d, int ff) {
  const int hd = H * d;
  MhaT<PT> m;
  m.ln1w = p; p += c1;
  m.ln1b = p; p += c1;
  m.ln2w = p; p += c2;
  m.ln2b = p; p += c2;
  m.q = p; p += c1 * hd;
  m.k = p; p += hd * c2;
  m.v = p; p += c2 * hd;
  m.li1w = p; p += hd * c1;
  m.li1b = p; p += c1;
  m.ln3w = p; p += c1;
  m.ln3b = p; p += c1;
  m.li2w = p; p += c1 * ff;
  m.li2b = p; p += ff;
  m.li3w = p; p += ff * c1;
  m.li3b = p;
  return m;
}

struct Off {                   // float offsets into the blob
  int64_t t_li1[3], t_li2[3];  // torso input projections
  int64_t t_layer0, t_layer;   // first torso layer, stride
  int64_t emb, pos, blk0, blk; // policy
  int64_t out, v[4];           // policy logits, value MLP
  int64_t total;
};

inline Off offsets(const tg_net_config& c) {
  Off o{};
  int64_t p = 0;
  const int64_t S2 = static_cast<int64_t>(c.S) * c.S, cin = static_cast<int64_t>(c.S) * c.T + 1;
  for (int g = 0; g < 3; ++g) { o.t_li1[g] = p; p += c.dim_s * S2 + S2; }
  for (int g = 0; g < 3; ++g) { o.t_li2[g] = p; p += cin * c.c + c.c; }
  o.t_layer0 = p;
  o.t_layer = mha_size(c.c, c.c, c.torso_heads, c.torso_d, c.torso_ff);
  p += o.t_layer * c.torso_layers;
  o.emb = p; p += static_cast<int64_t>(c.n_logits + 1) * c.W;
  o.pos = p; p += static_cast<int64_t>(c.n_steps) * c.W;
  o.blk0 = p;
  o.blk = 2LL * c.W + mha_size(c.W, c.W, c.heads, c.d, c.ff) + 2LL * c.W + mha_size(c.W, c.c, c.heads, c.d, c.ff);
  p += o.blk * c.blocks;
  o.out = p; p += static_cast<int64_t>(c.W) * c.n_logits + c.n_logits;
  const int64_t nh = c.n_hidden;
  o.v[0] = p; p += c.W * nh + nh;
  o.v[1] = p; p += nh * nh + nh;
  o.v[2] = p; p += nh * nh + nh;
  o.v[3] = p; p += nh * c.n_quantile + c.n_quantile;
  o.total = p;
  return o;
}

// ---- building blocks (all threads of the workgroup call them; each ends without a barrier) -------------------------
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };

// Y[r][o] = res2[r][o] + (res[r][o] + act(sum_i X[r][i] * Wt[i][o] + bias[o])) for r < R, o < O.
template <int RB>
__device__ inline void mm_rb(const float* X, int ldx, int R, int I, const float* __restrict__ Wt, int ldw, int O,
                             const float* __restrict__ bias, int act, const float* res, const float* res2, int ldr,
                             float* Y, int ldy) {
  const int groups = (R + RB - 1) / RB;
  for (int it = threadIdx.x; it < O * groups; it += NT) {
    const int o = it % O, r0 = (it / O) * RB;
    const float* xr[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) xr[u] = X + (r0 + u < R ? r0 + u : R - 1) * ldx;
    float acc[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) acc[u] = 0.f;
    const float* wp = Wt + o;
#pragma unroll 8
    for (int i = 0; i < I; ++i) {
      const float wv = wp[static_cast<int64_t>(i) * ldw];
#pragma unroll
      for (int u = 0; u < RB; ++u) acc[u] = fmaf(xr[u][i], wv, acc[u]);
    }
    const float b = bias ? bias[o] : 0.f;
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int r = r0 + u;
      if (r >= R) break;
      float v = acc[u] + b;
      if (act == ACT_GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
      else if (act == ACT_RELU) v = v > 0.f ? v : 0.f;
      if (res) v = res[r * ldr + o] + v;
      if (res2) v = res2[r * ldr + o] + v;
      Y[r * ldy + o] = v;
    }
  }
}

__device__ inline void mm(const float* X, int ldx, int R, int I, const float* Wt, int ldw, int O, const float* bias,
                          float* Y, int ldy, int act = ACT_NONE, const float* res = nullptr,
                          const float* res2 = nullptr, int ldr = 0) {
  const int work = R * O;
  if (work >= 8 * NT) mm_rb<8>(X, ldx, R, I, Wt, ldw, O, bias, act, res, res2, ldr, Y, ldy);
  else if (work >= 4 * NT) mm_rb<4>(X, ldx, R, I, Wt, ldw, O, bias, act, res, res2, ldr, Y, ldy);
  else if (work >= 2 * NT) mm_rb<2>(X, ldx, R, I, Wt, ldw, O, bias, act, res, res2, ldr, Y, ldy);
  else mm_rb<1>(X, ldx, R, I, Wt, ldw, O, bias, act, res, res2, ldr, Y, ldy);
}

// LayerNorm (eps 1e-5, biased variance) of R rows of n <= 64 floats: 32 lanes per row, two passes.
__device__ inline void layernorm(const float* X, int ldx, int R, int n, const float* __restrict__ w,
                                 const float* __restrict__ b, float* Y, int ldy) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5;
  for (int r = team; r < R; r += NT / 32) {
    const float* x = X + r * ldx;
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
    if (lane < n) Y[r * ldy + lane] = d0 * rstd * w[lane] + b[lane];
    if (lane + 32 < n) Y[r * ldy + lane + 32] = d1 * rstd * w[lane + 32] + b[lane + 32];
  }
}

// softmax in place over rows of n entries (one thread per row)
__device__ inline void softmax_rows(float* A, int rows, int n, int ld) {
  for (int r = threadIdx.x; r < rows; r += NT) {
    float* a = A + r * ld;
    float m = a[0];
    for (int j = 1; j < n; ++j) m = fmaxf(m, a[j]);
    float s = 0.f;
    for (int j = 0; j < n; ++j) {
      const float e = expf(a[j] - m);
      a[j] = e;
      s += e;
    }
    const float inv = 1.f / s;
    for (int j = 0; j < n; ++j) a[j] *= inv;
  }
}

// ---- the torso's rows (inference's torso, training's torso_fwd and torso_bwd) ---------------------------------------
// A workgroup holds nseq slices i0 <= i < i0 + nseq of a game's three grids as G[m][s][j] (s = i - i0, a row of c
// channels each): nseq = S with i0 = 0 is the whole game, nseq = 1 one slice.  With nseq a constant 1 the mappings below
// fold to the identity on a slice's rows.

// the sequence s of token r, in rows of L tokens per sequence
__device__ inline int seq_of(int r, int L, int nseq) { return nseq == 1 ? 0 : r / L; }

// pair (m1, m2): token r = s*2S + u is grid m1 row (s, u) for u < S, grid m2 row (s, u - S) otherwise
__device__ inline int pair_row(int r, int S, int nseq, int m1, int m2) {
  const int s = seq_of(r, 2 * S, nseq), u = r - s * 2 * S;
  return u < S ? (m1 * nseq + s) * S + u : (m2 * nseq + s) * S + u - S;
}

// ee row s*3S + m*S + j (counted from slice i0's first) is grid m row (s, j)
__device__ inline int ee_row(int row, int S, int nseq) {
  if (nseq == 1) return row;
  const int s = row / (3 * S), m = (row / S) % 3, j = row % S;
  return (m * nseq + s) * S + j;
}

// The torso's input rows of game g: IN[m][s][j][ch], ch = c3*T + t < S*T from the frames (int8 or float32, grid m
// through its permutation of the three indices), ch = S*T the scalar projection at (i, j).
__device__ inline void torso_inputs(const tg_net_config& c, const Off& off, const float* w, const void* frames,
                                    int frames_i8, const float* scalars, int64_t g, int nseq, int i0, float* IN) {
  const int S = c.S, S2 = S * S, cin = S * c.T + 1;
  const int64_t fstride = static_cast<int64_t>(c.T) * S2 * S;
  for (int it = threadIdx.x; it < 3 * nseq * S * cin; it += NT) {
    const int ch = it % cin, j = (it / cin) % S, i = i0 + (it / (cin * S)) % nseq, m = it / (cin * S * nseq);
    float v;
    if (ch == cin - 1) {
      const float* Wt = w + off.t_li1[m];
      const int tok = i * S + j;
      float s = 0.f;
      for (int q = 0; q < c.dim_s; ++q) s = fmaf(scalars[g * c.dim_s + q], Wt[q * S2 + tok], s);
      v = s + Wt[c.dim_s * S2 + tok];
    } else {
      const int c3 = ch / c.T, t = ch % c.T;
      int a0, a1, a2;
      if (m == 0) { a0 = i; a1 = j; a2 = c3; }
      else if (m == 1) { a0 = j; a1 = c3; a2 = i; }
      else { a0 = c3; a1 = i; a2 = j; }
      const int64_t idx = g * fstride + ((static_cast<int64_t>(t) * S + a0) * S + a1) * S + a2;
      v = frames_i8 ? static_cast<float>(static_cast<const int8_t*>(frames)[idx])
                    : static_cast<const float*>(frames)[idx];
    }
    IN[it] = v;
  }
}

}  // namespace net
}  // namespace tg
