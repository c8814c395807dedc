/*
 * tensor_game_net_s25.h -- C ABI of libtensorgame.so, part 5c: the fused eval-mode inference of tensor_game_net.h at the
 * 5x5 matmul tensor, S = 25 exactly (the largest state size the environment serves), with n_steps up to 3S = 75.
 *
 * tensor_game_net.h's entries keep their family (S <= TG_NET_MAX_S, 9 and 16) and refuse this size; the entries here take
 * this size only.  Conventions, configuration struct, weight blob and sampling rule are tensor_game_net.h's, unchanged
 * (mat_mul_amd/net.py's pack_weights serves as it is).  Inference only: training at S = 25 is tensor_game_train_s25.h's.
 *
 * What differs from the other sizes is the decoder's LDS plan.  The torso runs by slices as at S = 16
 * (net_torso_slice_kernel, one workgroup per (game, slice i), B * 25 workgroups; 37.1 KiB at the training app's
 * configuration).  The decoder of tensor_game_net.h keeps ln2(ee) of the game in LDS once per policy block, blocks x J x c
 * floats with J = 3 * 25^2 = 1875 keys: 117 KiB of a 169.5 KiB plan at the training app's configuration (c 8, W 32, two
 * blocks), above the 160 KiB a workgroup has.  The LayerNorm statistics of a row of ee do not depend on the block, only
 * the scale w_b and the bias b_b do, so the decoder here keeps ONE normalised copy z[J][c] = (ee - mean) * rstd and
 * applies each block's w_b, b_b where the row is consumed:
 *   scores:  (Wk_h^T q_h) . (w_b * z_j + b_b) = ((Wk_h^T q_h) * w_b) . z_j + const -- the scale is folded into the
 *            QK row of (sample, head), and the bias term is the same for every key j, so the softmax drops it;
 *   output:  sum_j a_j (w_b * z_j + b_b) = w_b * (sum_j a_j z_j) + b_b, the a_j summing to one.
 * The plan is the other sizes' with J x c floats in place of blocks x J x c: 110.9 KiB at the training app's
 * configuration with R = 1 sample per workgroup (162.3 KiB at R = 2, so it runs R = 1 and one workgroup per CU), 104.2
 * KiB at three blocks, two heads.  The softmax over the 1875 keys runs a 32-lane team per row and so does the weighted sum
 * of z (lane l takes keys l, l + 32, ..., the partial sums meet in a fixed butterfly), so a row's result depends on
 * neither R nor the launch shape.  Everything else -- step loop, self-attention cache, MLPs, sampling, value head -- is
 * the code of the other sizes.
 */
#ifndef TENSOR_GAME_NET_S25_H_
#define TENSOR_GAME_NET_S25_H_

#include "tensor_game_net.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_NET_WIDE3_S 25
#define TG_NET_WIDE3_MAX_STEPS 75

/* 0 if the configuration is inside this header's family: S == TG_NET_WIDE3_S exactly (any other S is
 * TG_ERR_UNSUPPORTED with a message that points to tg_net_check), n_steps <= TG_NET_WIDE3_MAX_STEPS, every other
 * TG_NET_MAX_* bound of tensor_game_net.h, and both LDS plans -- one torso slice, and the decoder above at R = 1 --
 * within 160 KiB (the refusal prints both byte counts).  TG_ERR_INVALID for a null pointer or a dimension < 1.
 * Host only. */
int tg_net_s25_check(const tg_net_config* cfg);

/* *floats = the size in floats of the packed weight blob of cfg (tensor_game_net.h's layout).  Host only. */
int tg_net_s25_weights_size(const tg_net_config* cfg, int64_t* floats);

/* tg_net_torso_masked at S = 25: arguments, checks and their order are that entry's (flags = NULL means every row, need
 * is then ignored).  One launch of B * 25 workgroups; workgroup (g, i) computes rows i*75 .. i*75 + 74 of ee[g]. */
int tg_net_s25_torso(const tg_net_config* cfg, const float* w, const void* frames, int frames_is_i8, const float* scalars,
                     float* ee, int64_t B, const uint8_t* flags, int need, tg_stream_t stream);

/* tg_net_sample_masked at S = 25: the same contract, sampling rule (Philox counter (row, call, sample, t / 4): at 75
 * steps 18 whole blocks and three words of the 19th) and mask rule (an inactive row's workgroups return before any load
 * and write nothing).  An active row's result depends on nothing but that row, and not on R or the launch shape.
 * R = the largest number of samples <= min(k, 8) whose plan fits in 160 KiB. */
int tg_net_s25_sample(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* rows, int64_t B, int k,
                      uint64_t seed, uint64_t call, const float* uniforms, int8_t* tokens_i8, float* probs, float* q,
                      const uint8_t* flags, int need, tg_stream_t stream);

/* tg_net_logits at S = 25: the same contract. */
int tg_net_s25_logits(const tg_net_config* cfg, const float* w, const float* ee, const int64_t* g_action, int64_t B,
                      float* oo, float* zz0, float* q, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_NET_S25_H_ */
