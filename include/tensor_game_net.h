/*
 * tensor_game_net.h -- C ABI of libtensorgame.so, part 5: fused eval-mode inference of the AlphaTensor network.
 *
 * Replaces the reference's eager network forward (model.py): the Torso (:85-123), the autoregressive PolicyHead.fwd_infer
 * (:234-261, which reruns the whole prefix at each of the n_steps token steps), the ValueHead (:266-280) with
 * value_risk_mgmt (:322-324), and the forward of PolicyHead.fwd_train (:219-232) -- about 4 000 small torch ops per
 * fwd_infer call -- by two launches per fwd_infer call (torso, then decoder + sampling + value head) and two per
 * teacher-forced call.  Eval mode: dropout is off (the reference calls model.eval() before self-play).
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  The configuration is a HOST
 * struct passed by pointer.  Everything is float32 (fp32 arithmetic, no reduced precision anywhere).
 *
 * Weight blob (tg_net_weights_size floats, one contiguous float32 array, 4-byte aligned).  Every Linear(in, out) is
 * stored TRANSPOSED as Wt[in][out] (row-major, out fastest) followed by its bias[out] when it has one, EXCEPT the key
 * projections, which are stored as torch holds them, K[heads*d][in] (head h's rows h*d .. h*d+d-1).  A LayerNorm(n) is
 * weight[n] then bias[n].  An attention block MHA(c1, c2, heads, d, ff) (model.py:44-67) is, in this order:
 *   ln1(c1), ln2(c2), Q = Wt[c1][heads*d] (head h = columns h*d ..), K[heads*d][c2], V = Wt[c2][heads*d],
 *   li1 = Wt[heads*d][c1] + b[c1], ln3(c1), li2 = Wt[c1][ff] + b[ff], li3 = Wt[ff][c1] + b[c1].
 * The blob is, in this order:
 *   torso:  li1[g] = Wt[dim_s][S*S] + b[S*S] for g = 0,1,2;  li2[g] = Wt[S*T+1][c] + b[c] for g = 0,1,2;
 *           torso_layers x MHA(c, c, torso_heads, torso_d, torso_ff);
 *   policy: emb[n_logits+1][W];  pos[n_steps][W] = pos_enc + pos_enc_fix (summed in float64, rounded once);
 *           blocks x { ln1(W), att1 = MHA(W, W, heads, d, ff), ln2(W), att2 = MHA(W, c, heads, d, ff) };
 *           out = Wt[W][n_logits] + b[n_logits];
 *   value:  Wt[W][n_hidden] + b, Wt[n_hidden][n_hidden] + b, Wt[n_hidden][n_hidden] + b, Wt[n_hidden][n_quantile] + b.
 * mat_mul_amd/net.py packs it from a state_dict.
 *
 * Sampling rule (tg_net_sample).  For game row r (rows[b]), call counter `call`, sample s < k and step t < n_steps the
 * uniform is u = (w >> 8) * 2^-24, w = word (t % 4) of philox4x32_10(counter = (r, call, s, t / 4), the low 32 bits of
 * r and call; key = (seed low 32 bits, seed high 32 bits)) (tg_device.h; oracle/tensor_game.py restates it).  p = the
 * float32 softmax of the step's logits (the maximum subtracted, expf, the sum in token order, then p_t = e_t / sum);
 * c_t = p_0 + ... + p_t summed in float32 in token order; the token is the first t with u < c_t, n_logits - 1 if there
 * is none; pp is the float32 product of the chosen p in step order, starting from 1.  With `uniforms` given, u = uniforms[b][s][t] instead.
 */
#ifndef TENSOR_GAME_NET_H_
#define TENSOR_GAME_NET_H_

#include "tensor_game.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The supported family.  What sets the bounds: every activation of one game (torso) or of one group of R <= 8 samples
 * of one game (decoder, with its self-attention cache of blocks x n_steps x W floats per sample) lives in LDS, at most
 * 160 KiB per workgroup.  With every dimension at its bound the torso takes 74 KiB and the decoder 70 KiB at R = 1 and
 * 157 KiB at R = 4 (R shrinks until the plan fits); the training app's configuration takes 18.5 KiB and 60 KiB (R = 8).
 * LayerNorm runs 32 lanes per row over two elements each (W, dim_c <= 64), and a thread keeps one logit row of at most
 * TG_NET_MAX_LOGITS.  The reference's constructor default (W = 2048, a 2048 -> 8192 MLP) is a GEMM-shaped problem
 * outside this family. */
#define TG_NET_MAX_S 5          /* dim_3d */
#define TG_NET_MAX_T 8          /* dim_t */
#define TG_NET_MAX_DIM_S 4      /* dim_s: scalars per state */
#define TG_NET_MAX_C 32         /* dim_c */
#define TG_NET_MAX_W 64         /* n_feats * n_heads */
#define TG_NET_MAX_HEADS 8      /* heads of every attention block (torso and policy) */
#define TG_NET_MAX_D 64         /* head dimension d */
#define TG_NET_MAX_TORSO_FF 128 /* the torso MLP width (4 * dim_c in the reference) */
#define TG_NET_MAX_FF 256       /* the policy MLP width (4 * W in the reference) */
#define TG_NET_MAX_LAYERS 16    /* torso layers */
#define TG_NET_MAX_BLOCKS 4     /* policy blocks */
#define TG_NET_MAX_STEPS 16     /* n_steps */
#define TG_NET_MAX_LOGITS 8     /* n_logits */
#define TG_NET_MAX_HIDDEN 512   /* n_hidden of the value head */
#define TG_NET_MAX_QUANTILE 16  /* n_quantile */
#define TG_NET_MAX_SAMPLES 64   /* k = n_samples (TG_SEARCH_MAX_K) */

/* One more state size outside S <= TG_NET_MAX_S: the 3x3 matmul tensor, S = 9 exactly, with n_steps up to
 * TG_NET_WIDE_MAX_STEPS (= 3S).  Every other TG_NET_MAX_* bound applies, and so does the LDS plan, which grows with S:
 * at S = 9 the torso holds 3 x 81 rows and the decoder's cross-attention J = 243 keys, so only small c, W and n_steps
 * fit.  The training app's configuration at S = 9 (c 8, W 32, T 2, 8 torso layers, n_steps 27) takes 100 KiB (torso)
 * and 127 KiB (decoder, R = 8). */
#define TG_NET_WIDE_S 9
#define TG_NET_WIDE_MAX_STEPS 27

/* And a second one: the 4x4 matmul tensor, S = 16 exactly, with n_steps up to TG_NET_WIDE2_MAX_STEPS (= 3S); training
 * there goes through tensor_game_train_sliced.h (tg_net_train_check refuses the size).  A whole game's torso does not fit there (344 KiB at the training app's
 * configuration), and does not have to: the first grid index is a batch index through every attention block of the
 * torso, so tg_net_torso runs one workgroup per (game, slice i) on the 3S rows (i, m, j) of the three grids.  The torso
 * term of the LDS check is that slice plan (3S x c grids, four 2S x c buffers, one head's q/k/v or the MLP's hidden
 * rows or the 3S input rows, one head's 2S x 2S scores); the decoder term is the same plan as at every size, with
 * J = 768 keys in the cross-attention.  The training app's configuration at S = 16 (c 8, W 32, T 2, 8 torso layers,
 * n_steps 48) takes 21.5 KiB per slice and 158 KiB in the decoder (R = 4 samples per workgroup; 76 KiB at R = 1).  With
 * J > 256 keys the decoder's cross-attention softmax runs a 32-lane team per row, its partial sums in a fixed order.
 * The 5x5 matmul tensor, S = 25, is not in this family (tg_net_check refuses it): it has entries of its own in
 * tensor_game_net_s25.h, with this header's conventions, configuration, blob and sampling rule. */
#define TG_NET_WIDE2_S 16
#define TG_NET_WIDE2_MAX_STEPS 48

/* The dimensions of one network, all inferred from a state_dict (mat_mul_amd/net.py). */
typedef struct tg_net_config {
  int32_t S, T, dim_s, c;                                     /* dim_3d, dim_t, dim_s, dim_c */
  int32_t torso_layers, torso_heads, torso_d, torso_ff;       /* torso attention blocks */
  int32_t W, heads, d, ff, blocks;                            /* policy width n_feats*n_heads, its blocks */
  int32_t n_steps, n_logits, n_hidden, n_quantile;
} tg_net_config;

/* 0 if the configuration is inside the supported family, TG_ERR_UNSUPPORTED naming the bound otherwise (TG_ERR_INVALID
 * for a null pointer or a dimension < 1).  Host only. */
int tg_net_check(const tg_net_config* cfg);

/* *floats = the size in floats of the packed weight blob of cfg (the layout above).  Host only. */
int tg_net_weights_size(const tg_net_config* cfg, int64_t* floats);

/* Torso.forward (model.py:97-123) for B games in ONE launch: frames (B,T,S,S,S) float32 (frames_is_i8 = 0) or int8
 * (frames_is_i8 = 1, converted exactly), scalars float32 (B,dim_s) -> ee float32 (B,3S^2,c) in the reference's order
 * (row i*3S + m*S + j = grid m, row (i, j)).  One workgroup per game, the three grids in LDS; at S = TG_NET_WIDE2_S one
 * workgroup per (game, i), which computes rows i*3S .. i*3S + 3S - 1. */
int tg_net_torso(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8, const float* scalars,
                 float* ee, int64_t B, tg_stream_t stream);

/* PolicyHead.fwd_infer (model.py:234-261) + ValueHead + value_risk_mgmt (model.py:347-356) for B games x k samples in
 * ONE launch: ee float32 (B,3S^2,c) -> tokens_i8 int8 (B,k,n_steps), probs float32 (B,k) (pp), q float32 (B,) (the
 * mean of the stored quantiles ceil(0.75 n)-1 .. n-1, not sorted).  rows int64 (B) are the game indices that key the
 * random stream, call the caller's counter (advance it every call), uniforms float32 (B,k,n_steps) or NULL (the
 * sampling rule above).  Decodes with a per-block cache of the self-attention inputs instead of rerunning the prefix
 * (equal under the causal mask).  Any of tokens_i8, probs, q may be NULL.  1 <= k <= TG_NET_MAX_SAMPLES. */
int tg_net_sample(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                  uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                  tg_stream_t stream);

/* tg_net_torso and tg_net_sample on the rows a device-side mask selects.  flags uint8 (B): row g is ACTIVE when
 * (flags[g] & need) == need; flags = NULL means every row (need is then ignored) and equals the plain entry bit for bit.
 * Every workgroup of an inactive row returns at once: the row's inputs are not read and its ee, tokens_i8, probs and q
 * are NOT WRITTEN (they keep what they held).  An active row's results are those of the plain entry, bit for bit: a
 * row's result depends on nothing but that row.  The mask is read when the kernel runs, so a captured graph follows the
 * current contents of flags.  need outside 1 .. 255 with flags given is TG_ERR_INVALID; every other check is the plain
 * entry's, in its order.  The self-play driver passes the search's flags (tensor_game_search.h) with
 * need = TG_SEARCH_EXPAND | TG_SEARCH_PENDING, and need = TG_SEARCH_RETRY for a retry. */
int tg_net_torso_masked(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8,
                        const float* scalars, float* ee, int64_t B, const uint8_t* flags, int need, tg_stream_t stream);
int tg_net_sample_masked(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                         uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                         const uint8_t* flags, int need, tg_stream_t stream);

/* The forward of PolicyHead.fwd_train (model.py:219-232) and the ValueHead on its zz[:, 0], in ONE launch: ee float32
 * (B,3S^2,c), g_action int64 (B,n_steps) (tokens in [0, n_logits); the input is START then g_action shifted by one)
 * -> oo float32 (B,n_steps,n_logits), zz0 float32 (B,W), q float32 (B,n_quantile) (the raw quantiles).  Any output may
 * be NULL.  A token outside [0, n_logits] reads as START (n_logits). */
int tg_net_logits(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* g_action, int64_t B,
                  float* oo, float* zz0, float* q, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_NET_H_ */
