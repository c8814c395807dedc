/*
 * tensor_game_train_sliced.h -- C ABI of libtensorgame.so, part 6b: the training loss of the AlphaTensor network and its
 * gradient at the 4x4 matmul tensor (S = TG_NET_WIDE2_S = 16), the one size tensor_game_train.h's entries refuse.
 *
 * Everything tensor_game_train.h states holds here unchanged and is not repeated: the conventions, theta's and grad's
 * layout with pos_fix kept apart, the two losses, the bad-token rows and the status word written by every call, the
 * dropout keep rule with keep_in / keep_out, the loss-only call with grad == NULL, float32 everywhere, no allocation, no
 * host sync, capturable into a hipGraph, bitwise reproducible with no float atomics.  What differs is how the work is cut,
 * because neither a whole game's torso (226 KiB at the training app's configuration, c 8, W 32, T 2, 8 torso layers,
 * n_steps 48) nor its decoder (514 KiB) fits a workgroup's 160 KiB of LDS:
 *
 *   1. the torso forward, one workgroup per (game, slice i), B * S of them.  The first grid index is a batch index
 *      through every attention block of the torso (as in tg_net_torso at this size), so a workgroup holds the 3S rows
 *      (i, m, j) of the three grids, their 3S input rows, three buffers of a pair's 2S tokens and one attention block's
 *      scratch for one sequence: 58 KiB at that configuration.  It saves each pair's 2S x c input rows at the place
 *      tensor_game_train.h's torso keeps them and writes its 3S rows of ee.
 *   2. the decoder forward, both losses and the decoder's backward on Pd = min(B, TG_NET_TRAIN_PARTIALS) workgroups, each
 *      taking a contiguous run of games in order.  A game's ee and dL/dee stay in the workspace (ee read through the
 *      cache; dL/dee read-modify-written by the owning workgroup only, between barriers) and so do the saved block inputs
 *      (one set per workgroup).  LDS holds the per-game rows (five n_steps x W buffers, logits, value head, keep mask,
 *      tokens) and one attention block's scratch.  The self-attention block runs on all n_steps positions.  The
 *      cross-attention block, every step of which is row-wise in the decoder positions given ee, runs forward and backward
 *      over chunks of Nq positions, without keys and values (scores (Wk_h^T q) . y_j, as at S = TG_NET_WIDE_S) and with a
 *      32-lane team per softmax row of J = 768 keys.  Nq comes from the plan: the largest count whose plan fits gives the
 *      fewest chunks, and Nq = ceil(n_steps / chunks) evens them out (Nq = 8, six chunks, 150 KiB at that configuration).
 *      The chunks add their weight gradients and their part of dL/dee one after another, in position order.
 *   3. the torso backward on Pt = min(B * S, TG_NET_TRAIN_PARTIALS) workgroups.  Workgroup p takes the units u = g * S + i
 *      in [B*S*p/Pt, B*S*(p+1)/Pt) in order (a run may straddle games), each pair recomputed from its saved input.  The
 *      gradient of the scalar projections li1 of a slice touches only its columns i*S .. i*S + S - 1.  Skipped for a
 *      loss-only call.
 *   4. the fixed-order sum of tensor_game_train.h's launch 4 over Pt slabs, p = 0 .. Pt - 1.
 *
 * The slabs: there are Pt >= Pd of them.  Slab p holds the torso part of the gradient (the blob up to the policy's emb)
 * of workgroup p of launch 3 and, for p < Pd, the policy and value part of workgroup p of launch 2; for p >= Pd that part
 * is zero (written by launch 3).  grad[i] is the float32 sum of slab 0 .. Pt - 1's element i in that order.
 *
 * The family is tg_net_check's at S = TG_NET_WIDE2_S, narrowed by LDS: the slice plan of launch 1 and the decoder plan of
 * launch 2 at Nq = 1 must each fit 160 KiB.  dim_c sets the decoder plan (two J x c buffers, the layer-normed ee and its
 * gradient): c = 8 leaves room for W = 32 with n_steps = 48, c above 24 fits nothing.
 */
#ifndef TENSOR_GAME_TRAIN_SLICED_H_
#define TENSOR_GAME_TRAIN_SLICED_H_

#include "tensor_game.h"
#include "tensor_game_net.h"
#include "tensor_game_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tg_net_check plus: S == TG_NET_WIDE2_S (any other S is TG_ERR_UNSUPPORTED with a pointer to tg_net_loss_grad), and both
 * LDS plans above at most 160 KiB (TG_ERR_UNSUPPORTED naming the two byte counts otherwise).  Host only. */
int tg_net_train_sliced_check(const tg_net_config* cfg);

/* *bytes = the workspace tg_net_loss_grad_sliced needs for B >= 1 games (grad or not):
 *   4 * (2 * B * 3S^2 * c                      ee and dL/dee
 *        + B * torso_layers * 3 * 2S^2 * c     the saved attention-pair inputs
 *        + 2 * B + B                           per-game losses and flags
 *        + Pd * blocks * 2 * n_steps * W       the saved decoder block inputs, Pd = min(B, TG_NET_TRAIN_PARTIALS)
 *        + Pt * n_theta)                       the partial slabs, Pt = min(B * S, TG_NET_TRAIN_PARTIALS)
 * plus alignment padding (each part starts on 256 bytes).  From B = 16 on Pt is 256: at the training app's configuration
 * (167 739 parameters) the slabs alone are 256 x 167 739 x 4 B = 172 MB.  Host only. */
int tg_net_train_sliced_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes);

/* tg_net_loss_grad (tensor_game_train.h: the same arguments, rules and results) by the launches above. */
int tg_net_loss_grad_sliced(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                            int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value,
                            int64_t B, float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                            const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes,
                            float* grad, float* losses, uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_TRAIN_SLICED_H_ */
