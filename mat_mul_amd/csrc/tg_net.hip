// Fused eval-mode inference of the AlphaTensor network (include/tensor_game_net.h).  gfx950 only; part of
// libtensorgame.so.
//
// Three kernels, all plain fp32 with every activation in LDS and the weights read from global memory (they are shared by
// every workgroup and stay in L2):
//   - net_torso_kernel: one workgroup per game.  The three S x S x c grids stay in LDS for all layers; each attention
//     pair (m1, m2) is S independent sequences of 2S tokens, processed head by head (q, k, v of one head, scores,
//     softmax, a @ v, then its slice of li1 added into the residual), then the MLP.
//   - net_torso_slice_kernel (S = TG_NET_WIDE2_S): one workgroup per (game, i).  The first grid index is a batch index
//     from the first torso layer to the last (a pair concatenates rows (i, .) of two grids and nothing transposes a
//     grid), so the 3S rows (i, m, j) go through every layer without reading another slice.
//     Both are one body (torso<SLICE>) over nseq sequences of 2S tokens, nseq = S or 1: the same arithmetic per row.
//   - net_decode_kernel: one workgroup per (game, group of R samples of that game); with teacher forcing one row per
//     game.  Decodes position by position with a per-(row, block) cache of the self-attention's normalised key/value
//     input (W floats per position): with it, a head's scores are (Wk_h^T q_h) . y_j and its output is
//     Wv_h (sum_j a_j y_j), so neither keys nor values are stored.  The cross-attention does the same over ln2(ee) of
//     the game, normalised once per block at the start.  Under the causal mask this equals the reference's rerun of
//     the whole prefix.  The sampling rule runs per row at the end of each step; the value head runs in the workgroup
//     that holds sample 0, on the position-0 output.
//     At S = TG_NET_WIDE2_S (J = 768 keys) the cross-attention's softmax runs a 32-lane team per row
//     (net_decode_kernel<true>); every other size keeps one thread per row and its token-order sums.
//     At S = TG_NET_WIDE3_S (J = 1875 keys, include/tensor_game_net_s25.h) ln2(ee) once per block does not fit: there
//     net_decode_kernel<true, true> keeps one copy of ee normalised without scale and bias and applies each block's where
//     a row is consumed (the scale folded into the QK row, the bias constant over the keys of a softmax; the weighted sum
//     of the copy by 32-lane teams, scale and bias at its end).  The torso runs by slices there as well.
// Row mask (tg_net_torso_masked, tg_net_sample_masked): every workgroup of a game whose flags byte lacks one of the `need`
// bits (net::active) returns before its first barrier and before any load of the game's inputs, and writes nothing.  The
// test is uniform over the workgroup, and over the S slice workgroups / the `chunks` decoder workgroups of a game.
// Every matrix product goes through mm(): thread = (output column, group of RB rows), the weight element read once per
// RB rows, the rows read from LDS as broadcasts.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/tensor_game.h"
#include "../../include/tensor_game_net.h"
#include "../../include/tensor_game_net_s25.h"
#include "tg_device.h"
#include "tg_host.h"
#include "tg_net_common.h"

namespace tg {
namespace net {

// ---- LDS plans (floats) -----------------------------------------------------------------------------------------------
struct TorsoPlan {
  int G, X, XN, YN, Y, QKV, SC, total;
};

// nseq sequences of 2S tokens at once: the whole game (nseq = S) or one slice i of it, the rows (i, m, j) of the three
// grids (nseq = 1)
__host__ __device__ inline TorsoPlan torso_plan(const tg_net_config& c, int nseq) {
  const int N = nseq * 2 * c.S, cin = c.S * c.T + 1;
  int qkv = 3 * N * c.torso_d;
  if (N * c.torso_ff > qkv) qkv = N * c.torso_ff;
  if (3 * nseq * c.S * cin > qkv) qkv = 3 * nseq * c.S * cin;
  TorsoPlan p;
  p.G = 0;
  p.X = p.G + 3 * nseq * c.S * c.c;
  p.XN = p.X + N * c.c;
  p.YN = p.XN + N * c.c;
  p.Y = p.YN + N * c.c;
  p.QKV = p.Y + N * c.c;
  p.SC = p.QKV + qkv;
  p.total = p.SC + N * 2 * c.S;
  return p;
}

struct DecPlan {
  int EEN, CACHE, X, XB, XN, Q, QK, SC, YB, O, H1, M, F, LG, Z0, V1, V2, MISC, total;
  int wq, nsc;  // per-head strides of QK / YB and SC
};

// shared_ln: ONE normalised copy of the game's ee for every policy block (net_decode_kernel<true, true>), J x c floats
// where the plan otherwise holds ln2(ee) once per block
__host__ __device__ inline DecPlan dec_plan(const tg_net_config& c, int R, bool shared_ln = false) {
  const int J = 3 * c.S * c.S, hd = c.heads * c.d;
  DecPlan p;
  p.wq = c.W > c.c ? c.W : c.c;
  p.nsc = J > c.n_steps ? J : c.n_steps;
  p.EEN = 0;
  p.CACHE = p.EEN + (shared_ln ? 1 : c.blocks) * J * c.c;
  p.X = p.CACHE + R * c.blocks * c.n_steps * c.W;
  p.XB = p.X + R * c.W;
  p.XN = p.XB + R * c.W;
  p.Q = p.XN + R * c.W;
  p.QK = p.Q + R * hd;
  p.SC = p.QK + R * c.heads * p.wq;
  p.YB = p.SC + R * c.heads * p.nsc;
  p.O = p.YB + R * c.heads * p.wq;
  p.H1 = p.O + R * hd;
  p.M = p.H1 + R * c.W;
  p.F = p.M + R * c.W;
  p.LG = p.F + R * c.ff;
  p.Z0 = p.LG + R * TG_NET_MAX_LOGITS;
  p.V1 = p.Z0 + R * c.W;
  p.V2 = p.V1 + c.n_hidden;
  p.MISC = p.V2 + (c.n_hidden > c.n_quantile ? c.n_hidden : c.n_quantile);
  p.total = p.MISC + 2 * R;  // pp[R], token[R]
  return p;
}

// ---- torso --------------------------------------------------------------------------------------------------------
struct TorsoArgs {
  tg_net_config c;
  Off off;
  const float* w;
  const void* frames;
  int frames_i8;
  const float* scalars;
  float* ee;
  int64_t B;
  const uint8_t* flags;  // (B) or NULL: the row mask (net::active)
  uint8_t need;
};

// The torso of game g over nseq of its S slices: G holds their rows [m][s][j][ch]; a pair (m1, m2) is nseq independent
// sequences of 2S tokens (net::pair_row).  SLICE: one slice per workgroup, blockIdx.x = g*S + i; otherwise the whole
// game.  A compile-time constant, so that with one sequence the row mappings fold away (ee is then one contiguous run).
// Training's mha_fwd (tg_train.hip) is this block once more and stays apart: it starts from H1 = X + li1's bias where
// this adds the bias with head 0 (res + (acc + b)), so a merged body would change one side's result bits.
template <bool SLICE>
__device__ inline void torso(const TorsoArgs& a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int S = c.S, nseq = SLICE ? 1 : S, L = 2 * S, N = nseq * L, C = c.c, cin = S * c.T + 1;
  const int64_t g = SLICE ? blockIdx.x / S : blockIdx.x;
  const int i0 = SLICE ? static_cast<int>(blockIdx.x % S) : 0;
  if (g >= a.B || !active(a.flags, a.need, g)) return;
  const TorsoPlan P = torso_plan(c, nseq);
  float *G = lds + P.G, *X = lds + P.X, *XN = lds + P.XN, *YN = lds + P.YN, *Y = lds + P.Y, *QKV = lds + P.QKV,
        *SC = lds + P.SC;
  float* IN = QKV;
  torso_inputs(c, a.off, a.w, a.frames, a.frames_i8, a.scalars, g, nseq, i0, IN);
  __syncthreads();
  for (int m = 0; m < 3; ++m) {
    const float* Wt = a.w + a.off.t_li2[m];
    mm(IN + m * nseq * S * cin, cin, nseq * S, cin, Wt, C, C, Wt + cin * C, G + m * nseq * S * C, C);
  }
  __syncthreads();
  const int H = c.torso_heads, d = c.torso_d, hd = H * d, ff = c.torso_ff;
  const float sd = sqrtf(static_cast<float>(d));
  float *Q = QKV, *K = QKV + N * d, *V = QKV + 2 * N * d;
  for (int l = 0; l < c.torso_layers; ++l) {
    const Mha mh = mha_at(a.w + a.off.t_layer0 + l * a.off.t_layer, C, C, H, d, ff);
    for (int pr = 0; pr < 3; ++pr) {
      const int m1 = pr, m2 = pr == 2 ? 0 : pr + 1;
      for (int it = threadIdx.x; it < N * C; it += NT) {
        const float v = G[pair_row(it / C, S, nseq, m1, m2) * C + it % C];
        X[it] = v;
        Y[it] = v;
      }
      __syncthreads();
      layernorm(X, C, N, C, mh.ln1w, mh.ln1b, XN, C);
      layernorm(X, C, N, C, mh.ln2w, mh.ln2b, YN, C);
      __syncthreads();
      for (int h = 0; h < H; ++h) {
        mm(XN, C, N, C, mh.q + h * d, hd, d, nullptr, Q, d);
        // keys: K[r][e] = sum_i YN[r][i] * k[h*d+e][i]  (k stored [hd][c])
        for (int it = threadIdx.x; it < N * d; it += NT) {
          const int e = it % d, r = it / d;
          const float* kr = mh.k + (h * d + e) * C;
          float s = 0.f;
#pragma unroll 8
          for (int i = 0; i < C; ++i) s = fmaf(YN[r * C + i], kr[i], s);
          K[it] = s;
        }
        mm(YN, C, N, C, mh.v + h * d, hd, d, nullptr, V, d);
        __syncthreads();
        // scores within a sequence: SC[r][b] = Q[r] . K[seq(r)*L + b] / sqrt(d)
        for (int it = threadIdx.x; it < N * L; it += NT) {
          const int bb = it % L, r = it / L;
          const float* q = Q + r * d;
          const float* k = K + (seq_of(r, L, nseq) * L + bb) * d;
          float s = 0.f;
#pragma unroll 8
          for (int e = 0; e < d; ++e) s = fmaf(q[e], k[e], s);
          SC[it] = s / sd;
        }
        __syncthreads();
        softmax_rows(SC, N, L, L);
        __syncthreads();
        // O (into Q) = A @ V per sequence
        for (int it = threadIdx.x; it < N * d; it += NT) {
          const int e = it % d, r = it / d;
          const float* ar = SC + r * L;
          const float* v = V + seq_of(r, L, nseq) * L * d + e;
          float s = 0.f;
          for (int bb = 0; bb < L; ++bb) s = fmaf(ar[bb], v[bb * d], s);
          Q[it] = s;
        }
        __syncthreads();
        // Y += O_h @ li1[h*d .. h*d+d-1][:] (+ the bias with head 0)
        mm(Q, d, N, d, mh.li1w + h * d * C, C, C, h == 0 ? mh.li1b : nullptr, Y, C, ACT_NONE, Y, nullptr, C);
        __syncthreads();
      }
      layernorm(Y, C, N, C, mh.ln3w, mh.ln3b, XN, C);
      __syncthreads();
      mm(XN, C, N, C, mh.li2w, ff, ff, mh.li2b, QKV, ff, ACT_GELU);
      __syncthreads();
      mm(QKV, ff, N, ff, mh.li3w, C, C, mh.li3b, X, C, ACT_NONE, Y, nullptr, C);
      __syncthreads();
      for (int it = threadIdx.x; it < N * C; it += NT) G[pair_row(it / C, S, nseq, m1, m2) * C + it % C] = X[it];
      __syncthreads();
    }
  }
  float* out = a.ee + (g * S + i0) * 3 * S * C;
  for (int it = threadIdx.x; it < 3 * nseq * S * C; it += NT) out[it] = G[ee_row(it / C, S, nseq) * C + it % C];
}

__global__ void __launch_bounds__(NT) net_torso_kernel(TorsoArgs a) { torso<false>(a); }
__global__ void __launch_bounds__(NT) net_torso_slice_kernel(TorsoArgs a) { torso<true>(a); }

// ---- decoder ------------------------------------------------------------------------------------------------------
// softmax in place over rows of n entries, a team of 32 lanes per row: for the cross-attention's J = 768 keys at
// S = TG_NET_WIDE2_S, where one thread per row (softmax_rows) leaves R * heads threads at work for 3 x 768 steps.  Lane l
// takes entries l, l + 32, ...: its partial sum runs in that order and the 32 partial sums meet in a fixed butterfly, so a
// row's result depends on neither R nor the launch shape.  Rows of at most kTeamSoftmaxFrom entries (J <= 243 at every
// other supported size, and the self-attention's n_steps) keep softmax_rows and its token-order sum.
constexpr int kTeamSoftmaxFrom = 256;

__device__ inline void softmax_rows_team(float* A, int rows, int n, int ld) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5;
  for (int r = team; r < rows; r += NT / 32) {
    float* a = A + r * ld;
    float m = -INFINITY;
    for (int j = lane; j < n; j += 32) m = fmaxf(m, a[j]);
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 32));
    float s = 0.f;
    for (int j = lane; j < n; j += 32) {
      const float e = expf(a[j] - m);
      a[j] = e;
      s += e;
    }
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) s += __shfl_xor(s, x, 32);
    const float inv = 1.f / s;
    for (int j = lane; j < n; j += 32) a[j] *= inv;
  }
}

// The rows of X without a LayerNorm's scale and bias, z = (x - mean) * rstd: layernorm()'s two passes and its lanes.
__device__ inline void normalise_rows(const float* X, int ldx, int R, int n, float* Y, int ldy) {
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
    if (lane < n) Y[r * ldy + lane] = d0 * rstd;
    if (lane + 32 < n) Y[r * ldy + lane + 32] = d1 * rstd;
  }
}

// Y[rh][i] = w[i] * (sum_j A[rh][j] * Z[j][i]) + b[i] for rh < rows, i < C: the cross-attention's weighted sum over the
// shared normalised copy Z (J x C) with the block's LayerNorm scale and bias applied to the sum (the A[rh][.] sum to one).
// A team of 32 lanes per (rh, i), the partial sums in the order of softmax_rows_team, so neither R nor the launch shape
// reaches a row's result.
__device__ inline void weighted_sum_team(const float* A, int lda, int rows, int J, const float* Z, int C,
                                         const float* __restrict__ w, const float* __restrict__ b, float* Y, int ldy) {
  const int lane = threadIdx.x & 31, team = threadIdx.x >> 5;
  for (int o = team; o < rows * C; o += NT / 32) {
    const int i = o % C, rh = o / C;
    const float* a = A + rh * lda;
    float s = 0.f;
    for (int j = lane; j < J; j += 32) s = fmaf(a[j], Z[j * C + i], s);
#pragma unroll
    for (int x = 16; x >= 1; x >>= 1) s += __shfl_xor(s, x, 32);
    if (lane == 0) Y[rh * ldy + i] = fmaf(w[i], s, b[i]);
  }
}

// The tail of an attention block, from the heads' output O and the block's input XB (R rows):
// H1 = XB + li1(O); X = XB + (H1 + li3(gelu(li2(ln3(H1))))).  Ends with a barrier.
__device__ inline void att_tail(const Mha& m, int R, int W, int hd, int ff, const float* O, const float* XB, float* H1,
                                float* M, float* F, float* X) {
  mm(O, hd, R, hd, m.li1w, W, W, m.li1b, H1, W, ACT_NONE, XB, nullptr, W);
  __syncthreads();
  layernorm(H1, W, R, W, m.ln3w, m.ln3b, M, W);
  __syncthreads();
  mm(M, W, R, W, m.li2w, ff, ff, m.li2b, F, ff, ACT_GELU);
  __syncthreads();
  mm(F, ff, R, ff, m.li3w, W, W, m.li3b, X, W, ACT_NONE, H1, XB, W);
  __syncthreads();
}

struct DecArgs {
  tg_net_config c;
  Off off;
  const float* w;
  const float* ee;
  int64_t B;
  int k, R, chunks, teacher;
  const int64_t* rows;      // sampling: game index of each batch row (keys the stream)
  uint32_t seed_lo, seed_hi, call_lo;
  const float* uniforms;    // (B,k,n_steps) or NULL
  int8_t* tokens;           // (B,k,n_steps)
  float* probs;             // (B,k)
  float* q;                 // sampling: (B,) risk value; teacher: (B,n_quantile)
  const int64_t* g_action;  // teacher: (B,n_steps)
  float* oo;                // teacher: (B,n_steps,n_logits)
  float* zz0;               // teacher: (B,W)
  const uint8_t* flags;     // sampling: (B) or NULL, the row mask (net::active)
  uint8_t need;
};

// kTeam: the cross-attention's softmax by teams (the host takes it for J > kTeamSoftmaxFrom); the other instantiation is
// the kernel of every other size, whose registers the team code then does not touch.
// kSharedLn (with kTeam; tensor_game_net_s25.h): EEN holds one copy z of the game's ee, normalised without scale and bias,
// for every block.  Block b's ln2 scale is folded into the QK rows before the scores, its bias adds the same to every
// score of a (row, head) and is left out, and the weighted sum of z takes scale and bias at the end (weighted_sum_team).
template <bool kTeam, bool kSharedLn = false>
__global__ void __launch_bounds__(NT) net_decode_kernel(DecArgs a) {
  static_assert(kTeam || !kSharedLn, "the shared-normalisation decoder runs the team softmax");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const tg_net_config& c = a.c;
  const int64_t g = blockIdx.x / a.chunks;
  if (g >= a.B || !active(a.flags, a.need, g)) return;
  const int s0 = static_cast<int>(blockIdx.x % a.chunks) * a.R;
  const int R = a.k - s0 < a.R ? a.k - s0 : a.R;  // rows of this workgroup: samples s0 .. s0+R-1
  const int W = c.W, C = c.c, H = c.heads, d = c.d, hd = H * d, ff = c.ff, J = 3 * c.S * c.S, NS = c.n_steps;
  const int NL = c.n_logits;
  const DecPlan P = dec_plan(c, a.R, kSharedLn);
  float *EEN = lds + P.EEN, *CACHE = lds + P.CACHE, *X = lds + P.X, *XB = lds + P.XB, *XN = lds + P.XN,
        *Q = lds + P.Q, *QK = lds + P.QK, *SC = lds + P.SC, *YB = lds + P.YB, *O = lds + P.O, *H1 = lds + P.H1,
        *M = lds + P.M, *F = lds + P.F, *LG = lds + P.LG, *Z0 = lds + P.Z0, *V1 = lds + P.V1, *V2 = lds + P.V2;
  float* PP = lds + P.MISC;
  int* TOK = reinterpret_cast<int*>(lds + P.MISC + a.R);
  const int wq = P.wq, nsc = P.nsc;
  const float sd = sqrtf(static_cast<float>(d));
  const float* wb = a.w;
  const float* emb = wb + a.off.emb;
  const float* pos = wb + a.off.pos;
  const int cstride = c.blocks * NS * W;  // cache floats per row

  // ln2 of each block's cross-attention over the game's ee
  const float* eeg = a.ee + g * J * C;
  if (kSharedLn) {
    normalise_rows(eeg, C, J, C, EEN, C);
  } else {
    for (int b = 0; b < c.blocks; ++b) {
      const float* bp = wb + a.off.blk0 + b * a.off.blk;
      const Mha a2 = mha_at(bp + 2 * W + mha_size(W, W, H, d, ff) + 2 * W, W, C, H, d, ff);
      layernorm(eeg, C, J, C, a2.ln2w, a2.ln2b, EEN + b * J * C, C);
    }
  }
  for (int it = threadIdx.x; it < R * W; it += NT) X[it] = emb[NL * W + it % W] + pos[it % W];
  for (int r = threadIdx.x; r < R; r += NT) PP[r] = 1.f;
  __syncthreads();

  for (int t = 0; t < NS; ++t) {
    for (int b = 0; b < c.blocks; ++b) {
      const float* bp = wb + a.off.blk0 + b * a.off.blk;
      const float *bln1w = bp, *bln1b = bp + W;
      const Mha a1 = mha_at(bp + 2 * W, W, W, H, d, ff);
      const float* bln2 = bp + 2 * W + mha_size(W, W, H, d, ff);
      const Mha a2 = mha_at(bln2 + 2 * W, W, C, H, d, ff);
      float* cache = CACHE + b * NS * W;  // row r: + r * cstride; position j: + j * W
      // ---- self-attention: xb = ln1(x); x = xb + att1(xb, xb)
      layernorm(X, W, R, W, bln1w, bln1b, XB, W);
      __syncthreads();
      layernorm(XB, W, R, W, a1.ln1w, a1.ln1b, XN, W);
      layernorm(XB, W, R, W, a1.ln2w, a1.ln2b, cache + t * W, cstride);
      __syncthreads();
      mm(XN, W, R, W, a1.q, hd, hd, nullptr, Q, hd);
      __syncthreads();
      for (int h = 0; h < H; ++h)  // QK[r][h][i] = sum_e q[r][h*d+e] * k[h*d+e][i]
        mm(Q + h * d, hd, R, d, a1.k + h * d * W, W, W, nullptr, QK + h * wq, H * wq);
      __syncthreads();
      for (int it = threadIdx.x; it < R * H * (t + 1); it += NT) {
        const int j = it % (t + 1), rh = it / (t + 1), r = rh / H, h = rh % H;
        const float* qk = QK + (r * H + h) * wq;
        const float* y = cache + r * cstride + j * W;
        float s = 0.f;
        for (int i = 0; i < W; ++i) s = fmaf(qk[i], y[i], s);
        SC[rh * nsc + j] = s / sd;
      }
      __syncthreads();
      softmax_rows(SC, R * H, t + 1, nsc);
      __syncthreads();
      for (int it = threadIdx.x; it < R * H * W; it += NT) {
        const int i = it % W, rh = it / W, r = rh / H;
        const float* sc = SC + rh * nsc;
        const float* y = cache + r * cstride + i;
        float s = 0.f;
        for (int j = 0; j <= t; ++j) s = fmaf(sc[j], y[j * W], s);
        YB[rh * wq + i] = s;
      }
      __syncthreads();
      for (int h = 0; h < H; ++h) mm(YB + h * wq, H * wq, R, W, a1.v + h * d, hd, d, nullptr, O + h * d, hd);
      __syncthreads();
      att_tail(a1, R, W, hd, ff, O, XB, H1, M, F, X);
      // ---- cross-attention: xb = ln2(x); x = xb + att2(xb, ee)
      layernorm(X, W, R, W, bln2, bln2 + W, XB, W);
      __syncthreads();
      layernorm(XB, W, R, W, a2.ln1w, a2.ln1b, XN, W);
      __syncthreads();
      mm(XN, W, R, W, a2.q, hd, hd, nullptr, Q, hd);
      __syncthreads();
      for (int h = 0; h < H; ++h) mm(Q + h * d, hd, R, d, a2.k + h * d * C, C, C, nullptr, QK + h * wq, H * wq);
      __syncthreads();
      if (kSharedLn) {  // QK[r][h][i] *= w_b[i]
        for (int it = threadIdx.x; it < R * H * C; it += NT) QK[(it / C) * wq + it % C] *= a2.ln2w[it % C];
        __syncthreads();
      }
      const float* een = kSharedLn ? EEN : EEN + b * J * C;
      for (int it = threadIdx.x; it < R * H * J; it += NT) {
        const int j = it % J, rh = it / J;
        const float* qk = QK + rh * wq;
        const float* y = een + j * C;
        float s = 0.f;
        for (int i = 0; i < C; ++i) s = fmaf(qk[i], y[i], s);
        SC[rh * nsc + j] = s / sd;
      }
      __syncthreads();
      if (kTeam) softmax_rows_team(SC, R * H, J, nsc);
      else softmax_rows(SC, R * H, J, nsc);
      __syncthreads();
      if (kSharedLn) {
        weighted_sum_team(SC, nsc, R * H, J, een, C, a2.ln2w, a2.ln2b, YB, wq);
      } else {
        for (int it = threadIdx.x; it < R * H * C; it += NT) {
          const int i = it % C, rh = it / C;
          const float* sc = SC + rh * nsc;
          float s = 0.f;
          for (int j = 0; j < J; ++j) s = fmaf(sc[j], een[j * C + i], s);
          YB[rh * wq + i] = s;
        }
      }
      __syncthreads();
      for (int h = 0; h < H; ++h) mm(YB + h * wq, H * wq, R, C, a2.v + h * d, hd, d, nullptr, O + h * d, hd);
      __syncthreads();
      att_tail(a2, R, W, hd, ff, O, XB, H1, M, F, X);
    }
    if (t == 0)
      for (int it = threadIdx.x; it < R * W; it += NT) Z0[it] = X[it];
    // logits = li1(relu(x))
    for (int it = threadIdx.x; it < R * W; it += NT) XN[it] = X[it] > 0.f ? X[it] : 0.f;
    __syncthreads();
    mm(XN, W, R, W, wb + a.off.out, NL, NL, wb + a.off.out + W * NL, LG, TG_NET_MAX_LOGITS);
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += NT) {
      const float* lg = LG + r * TG_NET_MAX_LOGITS;
      const int s = s0 + r;
      int tok;
      if (a.teacher) {
        float* oo = a.oo ? a.oo + (g * NS + t) * NL : nullptr;
        if (oo)
          for (int l = 0; l < NL; ++l) oo[l] = lg[l];
        const int64_t gt = a.g_action[g * NS + t];
        tok = gt >= 0 && gt <= NL ? static_cast<int>(gt) : NL;
      } else {
        float u;
        if (a.uniforms) {
          u = a.uniforms[(g * a.k + s) * NS + t];
        } else {
          const U4 ctr{static_cast<uint32_t>(a.rows[g]), a.call_lo, static_cast<uint32_t>(s),
                       static_cast<uint32_t>(t >> 2)};
          const U4 wv = philox4x32_10(ctr, a.seed_lo, a.seed_hi);
          const uint32_t word = (t & 3) == 0 ? wv.x : (t & 3) == 1 ? wv.y : (t & 3) == 2 ? wv.z : wv.w;
          u = static_cast<float>(word >> 8) * 5.9604644775390625e-8f;
        }
        float mx = lg[0];
        for (int l = 1; l < NL; ++l) mx = fmaxf(mx, lg[l]);
        float sum = 0.f;
        for (int l = 0; l < NL; ++l) sum += expf(lg[l] - mx);
        tok = NL - 1;
        float cum = 0.f, pt = expf(lg[NL - 1] - mx) / sum;
        for (int l = 0; l < NL; ++l) {
          const float p = expf(lg[l] - mx) / sum;
          cum += p;
          if (u < cum) {
            tok = l;
            pt = p;
            break;
          }
        }
        PP[r] *= pt;
        if (a.tokens) a.tokens[(g * a.k + s) * NS + t] = static_cast<int8_t>(tok);
      }
      TOK[r] = tok;
    }
    __syncthreads();
    if (t + 1 < NS) {
      for (int it = threadIdx.x; it < R * W; it += NT) {
        const int r = it / W, i = it % W;
        X[it] = emb[TOK[r] * W + i] + pos[(t + 1) * W + i];
      }
      __syncthreads();
    }
  }
  if (!a.teacher && a.probs)
    for (int r = threadIdx.x; r < R; r += NT) a.probs[g * a.k + s0 + r] = PP[r];
  if (a.teacher && a.zz0)
    for (int i = threadIdx.x; i < W; i += NT) a.zz0[g * W + i] = Z0[i];
  // value head on the position-0 output of sample 0 (every sample's is the same)
  if (s0 != 0 || !a.q) return;
  const int nh = c.n_hidden, nq = c.n_quantile;
  mm(Z0, W, 1, W, wb + a.off.v[0], nh, nh, wb + a.off.v[0] + W * nh, V1, nh, ACT_RELU);
  __syncthreads();
  mm(V1, nh, 1, nh, wb + a.off.v[1], nh, nh, wb + a.off.v[1] + nh * nh, V2, nh, ACT_RELU);
  __syncthreads();
  mm(V2, nh, 1, nh, wb + a.off.v[2], nh, nh, wb + a.off.v[2] + nh * nh, V1, nh, ACT_RELU);
  __syncthreads();
  mm(V1, nh, 1, nh, wb + a.off.v[3], nq, nq, wb + a.off.v[3] + nh * nq, V2, nq);
  __syncthreads();
  if (a.teacher) {
    for (int i = threadIdx.x; i < nq; i += NT) a.q[g * nq + i] = V2[i];
  } else if (threadIdx.x == 0) {
    const int jj = (3 * nq + 3) / 4 - 1;  // ceil(0.75 n) - 1
    float s = 0.f;
    for (int i = jj; i < nq; ++i) s += V2[i];
    a.q[g] = s / static_cast<float>(nq - jj);
  }
}

}  // namespace net
}  // namespace tg

namespace {

// s25: the family of tensor_game_net_s25.h (S = TG_NET_WIDE3_S exactly, its n_steps bound, the slice plan and the
// shared-normalisation decoder plan) instead of tensor_game_net.h's
int check_cfg(const char* fn, const tg_net_config* c, bool s25 = false) {
  if (!c) return tg_internal_fail(TG_ERR_INVALID, "%s: null config", fn);
#define TG_LIM(v, name, M) {c->v, name, M, #M}
  const struct { int32_t v; const char* name; int32_t max; const char* bound; } t[] = {
      TG_LIM(S, "dim_3d", TG_NET_MAX_S), TG_LIM(T, "dim_t", TG_NET_MAX_T), TG_LIM(dim_s, "dim_s", TG_NET_MAX_DIM_S),
      TG_LIM(c, "dim_c", TG_NET_MAX_C), TG_LIM(torso_layers, "torso_layers", TG_NET_MAX_LAYERS),
      TG_LIM(torso_heads, "torso_heads", TG_NET_MAX_HEADS), TG_LIM(torso_d, "torso_d", TG_NET_MAX_D),
      TG_LIM(torso_ff, "torso_ff", TG_NET_MAX_TORSO_FF), TG_LIM(W, "W", TG_NET_MAX_W),
      TG_LIM(heads, "heads", TG_NET_MAX_HEADS), TG_LIM(d, "d", TG_NET_MAX_D), TG_LIM(ff, "ff", TG_NET_MAX_FF),
      TG_LIM(blocks, "blocks", TG_NET_MAX_BLOCKS), TG_LIM(n_steps, "n_steps", TG_NET_MAX_STEPS),
      TG_LIM(n_logits, "n_logits", TG_NET_MAX_LOGITS), TG_LIM(n_hidden, "n_hidden", TG_NET_MAX_HIDDEN),
      TG_LIM(n_quantile, "n_quantile", TG_NET_MAX_QUANTILE)};
#undef TG_LIM
  for (const auto& e : t)
    if (e.v < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: %s=%d < 1", fn, e.name, e.v);
  // S <= TG_NET_MAX_S as for every bound, or exactly TG_NET_WIDE_S or TG_NET_WIDE2_S with their own n_steps bounds instead
  const bool wide1 = !s25 && c->S == TG_NET_WIDE_S, wide2 = !s25 && c->S == TG_NET_WIDE2_S, wide = wide1 || wide2;
  if (s25 && c->S != TG_NET_WIDE3_S)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: dim_3d=%d is not TG_NET_WIDE3_S=%d (tg_net_check serves the other sizes)",
                            fn, c->S, TG_NET_WIDE3_S);
  if (s25 && c->n_steps > TG_NET_WIDE3_MAX_STEPS)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: n_steps=%d above TG_NET_WIDE3_MAX_STEPS=%d (dim_3d=%d)", fn,
                            c->n_steps, TG_NET_WIDE3_MAX_STEPS, c->S);
  if (!s25 && c->S == TG_NET_WIDE3_S)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: dim_3d=%d above TG_NET_MAX_S=%d: the entries of tensor_game_net_s25.h (tg_net_s25_check; "
                            "FusedAlphaTensor25) serve TG_NET_WIDE3_S=%d",
                            fn, c->S, TG_NET_MAX_S, TG_NET_WIDE3_S);
  if (!s25 && c->S > TG_NET_MAX_S && !wide)
    return tg_internal_fail(TG_ERR_UNSUPPORTED,
                            "%s: dim_3d=%d above TG_NET_MAX_S=%d, and not exactly TG_NET_WIDE_S=%d or TG_NET_WIDE2_S=%d",
                            fn, c->S, TG_NET_MAX_S, TG_NET_WIDE_S, TG_NET_WIDE2_S);
  if (wide1 && c->n_steps > TG_NET_WIDE_MAX_STEPS)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: n_steps=%d above TG_NET_WIDE_MAX_STEPS=%d (dim_3d=%d)", fn,
                            c->n_steps, TG_NET_WIDE_MAX_STEPS, c->S);
  if (wide2 && c->n_steps > TG_NET_WIDE2_MAX_STEPS)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: n_steps=%d above TG_NET_WIDE2_MAX_STEPS=%d (dim_3d=%d)", fn,
                            c->n_steps, TG_NET_WIDE2_MAX_STEPS, c->S);
  for (int i = 1; i < 17; ++i) {
    if ((wide || s25) && i == 13) continue;  // n_steps: its bound at a wide S is above
    if (t[i].v > t[i].max)
      return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: %s=%d above %s=%d", fn, t[i].name, t[i].v, t[i].bound, t[i].max);
  }
  // at S = TG_NET_WIDE2_S and TG_NET_WIDE3_S the torso runs by slices (net_torso_slice_kernel) and its term is one
  // slice's plan
  const size_t lt = tg::net::torso_plan(*c, wide2 || s25 ? 1 : c->S).total * sizeof(float),
               ld = tg::net::dec_plan(*c, 1, s25).total * sizeof(float);
  if (lt > tg::kMaxDynamicLds || ld > tg::kMaxDynamicLds)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: the LDS plan needs %zu (torso) / %zu (decoder) bytes > 160 KiB", fn,
                            lt, ld);
  return TG_OK;
}

int check_common(const char* fn, const tg_net_config* c, const float* w, int64_t B, bool s25) {
  if (int rc = check_cfg(fn, c, s25)) return rc;
  if (B < 0 || B > (1LL << 30)) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld out of range", fn, (long long)B);
  if (!w) return tg_internal_fail(TG_ERR_INVALID, "%s: null weights", fn);
  if (!aligned(w, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: weights not 4-byte aligned", fn);
  return TG_OK;
}

// the fields every decode takes; the caller adds its mode's inputs and outputs
tg::net::DecArgs dec_args(const tg_net_config* cfg, const float* w, const float* ee, int64_t B, int k, int teacher) {
  tg::net::DecArgs a{};
  a.c = *cfg;
  a.off = tg::net::offsets(*cfg);
  a.w = w;
  a.ee = ee;
  a.B = B;
  a.k = k;
  a.teacher = teacher;
  return a;
}

// s25: the shared-normalisation decoder of tensor_game_net_s25.h; in the A/B library also where TG_NET_DEC_SHARED_LN is
// set (the sizes of tensor_game_net.h, for comparison)
int launch_decode(const char* fn, tg::net::DecArgs& a, hipStream_t st, bool s25) {
  const bool shared_ln = s25 || TG_SWITCH("TG_NET_DEC_SHARED_LN");
  // rows per workgroup: up to 8 samples of one game, fewer when the plan would not fit in LDS
  int R = a.k < 8 ? a.k : 8;
  while (R > 1 && tg::net::dec_plan(a.c, R, shared_ln).total * sizeof(float) > static_cast<size_t>(tg::kMaxDynamicLds))
    --R;
  a.R = R;
  a.chunks = (a.k + R - 1) / R;
  if (a.B * a.chunks > INT32_MAX)
    return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld x %d workgroups per game is too large a grid", fn,
                            (long long)a.B, a.chunks);
  const size_t lds = tg::net::dec_plan(a.c, R, shared_ln).total * sizeof(float);
  const unsigned grid = static_cast<unsigned>(a.B * a.chunks);
  if (shared_ln) {
    if (int rc = lds_opt_in<tg::net::net_decode_kernel<true, true>>(fn, lds)) return rc;
    return launch(fn, tg::net::net_decode_kernel<true, true>, grid, tg::net::NT, lds, st, a);
  }
  if (3 * a.c.S * a.c.S > tg::net::kTeamSoftmaxFrom) {
    if (int rc = lds_opt_in<tg::net::net_decode_kernel<true>>(fn, lds)) return rc;
    return launch(fn, tg::net::net_decode_kernel<true>, grid, tg::net::NT, lds, st, a);
  }
  if (int rc = lds_opt_in<tg::net::net_decode_kernel<false>>(fn, lds)) return rc;
  return launch(fn, tg::net::net_decode_kernel<false>, grid, tg::net::NT, lds, st, a);
}

// the row mask of the *_masked entries: NULL flags = every row (need is then ignored)
int check_mask(const char* fn, const uint8_t* flags, int need) {
  if (flags && (need < 1 || need > 255))
    return tg_internal_fail(TG_ERR_INVALID, "%s: need=%d with flags given (the bits a row's flags must hold, 1 .. 255)", fn,
                            need);
  return TG_OK;
}

// tg_net_torso, tg_net_torso_masked and tg_net_s25_torso
int torso_entry(const char* fn, const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8,
                const float* scalars, float* ee, int64_t B, const uint8_t* flags, int need, tg_stream_t stream,
                bool s25 = false) {
  if (int rc = check_common(fn, cfg, w, B, s25)) return rc;
  if (frames_is_i8 != 0 && frames_is_i8 != 1)
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames_is_i8=%d (0 float32, 1 int8)", fn, frames_is_i8);
  if (int rc = check_mask(fn, flags, need)) return rc;
  if (B == 0) return TG_OK;
  if (!frames || !scalars || !ee) return tg_internal_fail(TG_ERR_INVALID, "%s: null frames, scalars or ee", fn);
  if (!aligned(frames, frames_is_i8 ? 1 : 4) || !aligned(scalars, 4) || !aligned(ee, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames, scalars or ee not aligned to their elements", fn);
  tg::net::TorsoArgs a{*cfg, tg::net::offsets(*cfg), w, frames, frames_is_i8, scalars, ee, B, flags,
                       static_cast<uint8_t>(flags ? need : 0)};
  // by slices at S = TG_NET_WIDE2_S and TG_NET_WIDE3_S; in the A/B library also where TG_NET_TORSO_SLICES is set (any
  // size, for comparison)
  if (s25 || cfg->S == TG_NET_WIDE2_S || TG_SWITCH("TG_NET_TORSO_SLICES")) {
    if (B * cfg->S > INT32_MAX)
      return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld x %d workgroups per game is too large a grid", fn, (long long)B,
                              cfg->S);
    const size_t lds = tg::net::torso_plan(*cfg, 1).total * sizeof(float);
    if (int rc = lds_opt_in<tg::net::net_torso_slice_kernel>(fn, lds)) return rc;
    return launch(fn, tg::net::net_torso_slice_kernel, static_cast<unsigned>(B * cfg->S), tg::net::NT, lds,
                  static_cast<hipStream_t>(stream), a);
  }
  const size_t lds = tg::net::torso_plan(*cfg, cfg->S).total * sizeof(float);
  if (int rc = lds_opt_in<tg::net::net_torso_kernel>(fn, lds)) return rc;
  return launch(fn, tg::net::net_torso_kernel, static_cast<unsigned>(B), tg::net::NT, lds, static_cast<hipStream_t>(stream), a);
}

// tg_net_sample, tg_net_sample_masked and tg_net_s25_sample
int sample_entry(const char* fn, const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B,
                 int k, uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                 const uint8_t* flags, int need, tg_stream_t stream, bool s25 = false) {
  if (int rc = check_common(fn, cfg, w, B, s25)) return rc;
  if (k < 1 || k > TG_NET_MAX_SAMPLES)
    return tg_internal_fail(TG_ERR_UNSUPPORTED, "%s: k=%d outside [1, TG_NET_MAX_SAMPLES=%d]", fn, k, TG_NET_MAX_SAMPLES);
  if (int rc = check_mask(fn, flags, need)) return rc;
  if (B == 0) return TG_OK;
  if (!ee || (!rows && !uniforms)) return tg_internal_fail(TG_ERR_INVALID, "%s: null ee, or null rows without uniforms", fn);
  if (!aligned(ee, 4) || !aligned(rows, 8) || !aligned(uniforms, 4) || !aligned(probs, 4) || !aligned(q, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: ee, rows, uniforms, probs or q not aligned to their elements", fn);
  tg::net::DecArgs a = dec_args(cfg, w, ee, B, k, 0);
  a.rows = rows;
  a.seed_lo = static_cast<uint32_t>(seed);
  a.seed_hi = static_cast<uint32_t>(seed >> 32);
  a.call_lo = static_cast<uint32_t>(call);
  a.uniforms = uniforms;
  a.tokens = tokens_i8;
  a.probs = probs;
  a.q = q;
  a.flags = flags;
  a.need = static_cast<uint8_t>(flags ? need : 0);
  return launch_decode(fn, a, static_cast<hipStream_t>(stream), s25);
}

// tg_net_logits and tg_net_s25_logits
int logits_entry(const char* fn, const tg_net_config* cfg, const float* w, const float* ee, const int64_t* g_action,
                 int64_t B, float* oo, float* zz0, float* q, tg_stream_t stream, bool s25 = false) {
  if (int rc = check_common(fn, cfg, w, B, s25)) return rc;
  if (B == 0) return TG_OK;
  if (!ee || !g_action) return tg_internal_fail(TG_ERR_INVALID, "%s: null ee or g_action", fn);
  if (!aligned(ee, 4) || !aligned(g_action, 8) || !aligned(oo, 4) || !aligned(zz0, 4) || !aligned(q, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: ee, g_action, oo, zz0 or q not aligned to their elements", fn);
  tg::net::DecArgs a = dec_args(cfg, w, ee, B, 1, 1);
  a.q = q;
  a.g_action = g_action;
  a.oo = oo;
  a.zz0 = zz0;
  return launch_decode(fn, a, static_cast<hipStream_t>(stream), s25);
}

int weights_size(const char* fn, const tg_net_config* cfg, int64_t* floats, bool s25) {
  if (int rc = check_cfg(fn, cfg, s25)) return rc;
  if (!floats) return tg_internal_fail(TG_ERR_INVALID, "%s: null output", fn);
  *floats = tg::net::offsets(*cfg).total;
  return TG_OK;
}

}  // namespace

extern "C" {

// model.py:85-280 (the configuration a state_dict implies)
int tg_net_check(const tg_net_config* cfg) { return check_cfg("tg_net_check", cfg); }

int tg_net_weights_size(const tg_net_config* cfg, int64_t* floats) {
  return weights_size("tg_net_weights_size", cfg, floats, false);
}

// Torso.forward, model.py:97-123
int tg_net_torso(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8, const float* scalars,
                 float* ee, int64_t B, tg_stream_t stream) {
  return torso_entry("tg_net_torso", cfg, w, frames, frames_is_i8, scalars, ee, B, nullptr, 0, stream);
}

int tg_net_torso_masked(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8,
                        const float* scalars, float* ee, int64_t B, const uint8_t* flags, int need, tg_stream_t stream) {
  return torso_entry("tg_net_torso_masked", cfg, w, frames, frames_is_i8, scalars, ee, B, flags, need, stream);
}

// PolicyHead.fwd_infer + ValueHead + value_risk_mgmt, model.py:234-261, 266-280, 322-324 (AlphaTensor.fwd_infer :347-356)
int tg_net_sample(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                  uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                  tg_stream_t stream) {
  return sample_entry("tg_net_sample", cfg, w, ee, rows, B, k, seed, call, uniforms, tokens_i8, probs, q, nullptr, 0,
                      stream);
}

int tg_net_sample_masked(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                         uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                         const uint8_t* flags, int need, tg_stream_t stream) {
  return sample_entry("tg_net_sample_masked", cfg, w, ee, rows, B, k, seed, call, uniforms, tokens_i8, probs, q, flags,
                      need, stream);
}

// the forward of PolicyHead.fwd_train, model.py:219-232, and ValueHead on its zz[:, 0] (AlphaTensor.fwd_train :335-338)
int tg_net_logits(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* g_action, int64_t B,
                  float* oo, float* zz0, float* q, tg_stream_t stream) {
  return logits_entry("tg_net_logits", cfg, w, ee, g_action, B, oo, zz0, q, stream);
}

// ---- include/tensor_game_net_s25.h: the same at S = TG_NET_WIDE3_S, the decoder with one normalised copy of ee --------
int tg_net_s25_check(const tg_net_config* cfg) { return check_cfg("tg_net_s25_check", cfg, true); }

int tg_net_s25_weights_size(const tg_net_config* cfg, int64_t* floats) {
  return weights_size("tg_net_s25_weights_size", cfg, floats, true);
}

int tg_net_s25_torso(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8, const float* scalars,
                     float* ee, int64_t B, const uint8_t* flags, int need, tg_stream_t stream) {
  return torso_entry("tg_net_s25_torso", cfg, w, frames, frames_is_i8, scalars, ee, B, flags, need, stream, true);
}

int tg_net_s25_sample(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                      uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                      const uint8_t* flags, int need, tg_stream_t stream) {
  return sample_entry("tg_net_s25_sample", cfg, w, ee, rows, B, k, seed, call, uniforms, tokens_i8, probs, q, flags, need,
                      stream, true);
}

int tg_net_s25_logits(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* g_action, int64_t B,
                      float* oo, float* zz0, float* q, tg_stream_t stream) {
  return logits_entry("tg_net_s25_logits", cfg, w, ee, g_action, B, oo, zz0, q, stream, true);
}

}  // extern "C"
