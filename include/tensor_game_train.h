/*
 * tensor_game_train.h -- C ABI of libtensorgame.so, part 6: the training loss of the AlphaTensor network and its gradient.
 *
 * Replaces the reference's eager train step (training.py:419-445): AlphaTensor.fwd_train (model.py:326-345) in train
 * mode, the combined loss weight_pol * l_pol + weight_val * l_val, and loss.backward() -- several thousand small torch
 * ops per batch -- by four launches whose number does not depend on B:
 *   1. the torso forward, one workgroup per game, saving the input of each of its 3 * torso_layers attention pairs;
 *   2. the teacher-forced decoder forward, both losses and the decoder's backward (value head included), producing
 *      dL/dee, on P workgroups (below) that each take a contiguous run of games in order;
 *   3. the torso backward on the same P workgroups, recomputing each pair's forward from its saved input;
 *   4. the fixed-order sum of the P partial gradients, the two losses and the status word.
 * Launch 3 is skipped, and launch 2 stops after the losses, for a loss-only call (grad NULL).
 *
 * Conventions: those of tensor_game.h and tensor_game_net.h (device pointers, asynchronous on `stream`, no allocation,
 * no host sync, capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  Everything is
 * float32.  The gradient is bitwise reproducible: no float atomics anywhere; workgroup p accumulates the gradients of its
 * games, in game order, into its own partial slab (a full-size float32 gradient in the workspace), and launch 4 sums the
 * slabs in the order p = 0 .. P-1.  P = min(B, TG_NET_TRAIN_PARTIALS).
 *
 * Parameter vector theta: exactly the weight blob of tensor_game_net.h, except that the `pos` slot holds pos_enc ONLY.
 * pos_fix (n_steps x W floats, the reference's buffer pos_enc_fix) is passed separately and added inside the kernel, so
 * that an optimizer decays pos_enc and never pos_enc_fix, as the reference's does.  grad has theta's layout (key
 * projections untransposed, as in the blob).  The inference blob is theta with pos_fix added into its pos slot.
 *
 * The loss (AlphaTensor.fwd_train):  the decoder runs teacher-forced on START followed by g_action shifted by one; the
 * value head runs on its position-0 output.
 *   l_pol = sum over the B * n_steps positions of the cross entropy of the logits against g_action;
 *   l_val = mean over B * n_quantile of huber(g_value - q_j) * |tau_j - 1[g_value - q_j > 0]| (huber with delta 1,
 *           tau_j = (j + 0.5) / n_quantile);
 *   L = weight_pol * l_pol + weight_val * l_val.   losses[0] = l_pol, losses[1] = l_val; grad = dL/dtheta.
 * A row holding a token outside [0, n_logits) adds nothing to l_pol (nor to its gradient), reads as START where it is a
 * decoder input, and sets TG_TRAIN_STATUS_BAD_TOKEN in *status; status is written by every call.
 *
 * Dropout (PredictBlock's dropout1 on att1's output and dropout2 on att2's, element-wise on (n_steps, W)): a kept element
 * is scaled by 1 / (1 - p) (float32), a dropped one is 0.  p = 0 is eval mode (every element kept, scale 1).  Keep rule:
 * for batch row r, call counter `call`, policy block blk, which = 0 (dropout1) or 1 (dropout2), position t and feature
 * i < W, let w = word (i % 4) of philox4x32_10(counter = (r, call, blk * 2 + which, t * ceil(W / 4) + i / 4), the low 32
 * bits of r and call; key = (seed low 32 bits, seed high 32 bits)) (tg_device.h) and u = (w >> 8) * 2^-24: the element
 * is kept iff u >= p.  keep_in, when given, replaces the rule (non-zero = kept); keep_out, when given, receives the mask
 * used (1 kept, 0 dropped).  Both are uint8 (B, blocks, 2, n_steps, W).
 */
#ifndef TENSOR_GAME_TRAIN_H_
#define TENSOR_GAME_TRAIN_H_

#include "tensor_game.h"
#include "tensor_game_net.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partial gradient slabs: P = min(B, TG_NET_TRAIN_PARTIALS) workgroups run launches 2 and 3, each with one slab. */
#define TG_NET_TRAIN_PARTIALS 256

/* Status bits. */
#define TG_TRAIN_STATUS_BAD_TOKEN 1u /* some g_action token lies outside [0, n_logits) */

/* 0 if cfg is inside the training family, TG_ERR_UNSUPPORTED naming the bound otherwise (TG_ERR_INVALID for a null
 * pointer or a dimension < 1).  The family is tg_net_check's, narrowed by LDS: the torso workgroup holds the three grids,
 * the pair's activations and one attention head's forward and backward buffers; the decoder workgroup holds the game's
 * ee and dL/dee, the inputs of every block, the mask and one attention block's buffers; each must fit in 160 KiB.
 * At S = TG_NET_WIDE_S the whole pair and the cross-attention's keys and values do not fit (263 and 272 KiB at the
 * training app's configuration), so there the torso runs each pair's attention block over a chunk of its S independent
 * sequences at a time (the fewest chunks that fit: 3 of 3 sequences, 116 KiB, at that configuration), and the decoder's
 * cross-attention keeps no keys or values (scores (Wk_h^T q) . y_j, output Wv_h (sum_j a_j y_j), 148 KiB); a
 * configuration fits when one sequence at a time does.  S = TG_NET_WIDE2_S is inside tg_net_check's family, and every
 * configuration of that size is refused here: training there goes through tensor_game_train_sliced.h.  Host only. */
int tg_net_train_check(const tg_net_config* cfg);

/* *bytes = the workspace tg_net_loss_grad needs for B >= 1 games (grad or not):
 *   4 * (2 * B * 3S^2 * c            ee and dL/dee
 *        + B * torso_layers * 3 * 2S^2 * c   the saved attention-pair inputs
 *        + 2 * B + B                  per-game losses and flags
 *        + P * n_theta)               the partial slabs, P = min(B, TG_NET_TRAIN_PARTIALS)
 * plus alignment padding (each part starts on 256 bytes).  Host only. */
int tg_net_train_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes);

/* The loss and gradient above for B >= 1 games:
 *   theta float32 (tg_net_weights_size), pos_fix float32 (n_steps, W), frames (B,T,S,S,S) float32 (frames_is_i8 = 0) or
 *   int8 (1), scalars float32 (B, dim_s), g_action int8 (B, n_steps), g_value float32 (B, 1);
 *   weight_pol, weight_val, dropout_p in [0, 1), seed and call (the keep rule), keep_in / keep_out (or NULL);
 *   workspace of workspace_bytes >= tg_net_train_workspace_size bytes (256-byte aligned), grad float32 like theta or
 *   NULL (loss only), losses float32 [2], status uint32 [1]. */
int tg_net_loss_grad(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                     int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value, int64_t B,
                     float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                     const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, float* grad,
                     float* losses, uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_TRAIN_H_ */
