/*
 * tensor_game_train_s25.h -- C ABI of libtensorgame.so, part 6c: the training loss of the AlphaTensor network and its
 * gradient at the 5x5 matmul tensor (S = TG_NET_WIDE3_S = 25), the size tensor_game_train.h's and
 * tensor_game_train_sliced.h's entries refuse.
 *
 * Everything tensor_game_train.h states holds here unchanged and is not repeated: the conventions, theta's and grad's
 * layout with pos_fix kept apart, the two losses, the bad-token rows and the status word written by every call, the
 * dropout keep rule with keep_in / keep_out, the loss-only call with grad == NULL, float32 everywhere, no allocation, no
 * host sync, capturable into a hipGraph, bitwise reproducible with no float atomics.  The four launches are
 * tensor_game_train_sliced.h's, and launches 1, 3 and 4 (the torso forward by slices on B * S workgroups, the torso
 * backward on Pt = min(B * S, TG_NET_TRAIN_PARTIALS) workgroups, the fixed-order sum of the Pt slabs) are the same
 * kernels, which take S at run time: a slice's plan is 103.1 KiB at the training app's configuration (a25: c 8, W 32,
 * T 2, 8 torso layers, n_steps 75) and 95.8 KiB at b25.  What differs is launch 2, the decoder forward, both losses and
 * the decoder's backward on Pd = min(B, TG_NET_TRAIN_PARTIALS) workgroups, because at n_steps = 75 positions and
 * J = 3S^2 = 1875 keys neither attention block fits a workgroup's 160 KiB of LDS beside the per-game rows (five
 * n_steps x W buffers, logits, value head, keep mask, tokens: 60.7 KiB at a25, 64.2 KiB at b25): the self-attention block
 * on all 75 positions needs 185.2 KiB by itself, the cross-attention block at one position, with ln2(ee) and its
 * gradient, 147.5 KiB.  Both are cut:
 *
 *   - The self-attention block runs forward and backward over chunks of Ns query positions.  Everything in it is
 *     row-wise in the positions but the keys and values; attention is causal, so the chunk of rows r0 .. r0 + n - 1 is
 *     the block on those n rows against the keys and values of rows 0 .. r0 + n - 1, computed anew for the chunk.  Its
 *     scratch is tensor_game_train.h's attention scratch for n queries and n_steps keys.  The chunks add their weight
 *     gradients (ln2's included: queries and keys are the same rows under two LayerNorms) and their part of the
 *     gradient of the block's input one after another, in position order.
 *   - The cross-attention block runs over chunks of Nx query positions, without keys and values and with a 32-lane team
 *     per softmax row, as at S = TG_NET_WIDE2_S.  One copy of ln2(ee) (J x c) stays in LDS for all the chunks of a block.
 *     dL/d ln2(ee) is a J x c accumulator of the workgroup's own in the workspace: the workgroup zeroes it before the
 *     first chunk, every chunk adds to it (read-modify-written by the owning workgroup only, between barriers, as dL/dee
 *     is), and after the last chunk ln2's backward takes it into dL/dee and the gradient of ln2's weights over tiles of
 *     256 keys, in key order.
 *
 * The two blocks run one after the other and share the room behind the rows, ln2(ee) included.  Ns and Nx come from one
 * plan function: per block the largest count that fits gives the fewest chunks, and ceil(n_steps / chunks) evens them
 * out.  Decoder plan and chunks:
 *
 *            rows       self-attention (Ns, chunks)     ln2(ee)    cross-attention (Nx, chunks)     launch 2
 *   a25    60.7 KiB     89.3 KiB (19, 4)               58.6 KiB    31.3 KiB (2, 38)               150.6 KiB
 *   b25    64.2 KiB     89.3 KiB (19, 4)               58.6 KiB    31.3 KiB (2, 38)               154.1 KiB
 *
 * The family is tg_net_s25_check's (S == TG_NET_WIDE3_S exactly, n_steps <= TG_NET_WIDE3_MAX_STEPS, every TG_NET_MAX_*
 * bound), narrowed by LDS: the slice plan of launch 1 and the decoder plan of launch 2 with Ns = 1 and with Nx = 1 must
 * each fit 160 KiB (119.3 and 135.0 KiB at a25, 122.7 and 138.4 KiB at b25).  dim_c sets the resident ln2(ee): at a25's
 * other dimensions c = 8 fits and c = 12 does not.
 */
#ifndef TENSOR_GAME_TRAIN_S25_H_
#define TENSOR_GAME_TRAIN_S25_H_

#include "tensor_game.h"
#include "tensor_game_net.h"
#include "tensor_game_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tg_net_s25_check plus the three LDS plans above at most 160 KiB (TG_ERR_UNSUPPORTED naming the three byte counts
 * otherwise).  Any S other than TG_NET_WIDE3_S that tg_net_check accepts is TG_ERR_UNSUPPORTED with a pointer to
 * tg_net_loss_grad and tg_net_loss_grad_sliced.  Host only. */
int tg_net_train_s25_check(const tg_net_config* cfg);

/* *bytes = the workspace tg_net_loss_grad_s25 needs for B >= 1 games (grad or not): tensor_game_train_sliced.h's parts
 * and the accumulators,
 *   4 * (2 * B * 3S^2 * c                      ee and dL/dee
 *        + B * torso_layers * 3 * 2S^2 * c     the saved attention-pair inputs
 *        + 2 * B + B                           per-game losses and flags
 *        + Pd * blocks * 2 * n_steps * W       the saved decoder block inputs, Pd = min(B, TG_NET_TRAIN_PARTIALS)
 *        + Pt * n_theta                        the partial slabs, Pt = min(B * S, TG_NET_TRAIN_PARTIALS)
 *        + Pd * 3S^2 * c)                      dL/d ln2(ee) of each decoder workgroup
 * plus alignment padding (each part starts on 256 bytes).  From B = 11 on Pt is 256: at a25 (171 249 parameters) the
 * slabs alone are 256 x 171 249 x 4 B = 175 MB, the whole 194 MB at B = 16 and 477 MB at B = 256.  Host only. */
int tg_net_train_s25_workspace_size(const tg_net_config* cfg, int64_t B, int64_t* bytes);

/* tg_net_loss_grad (tensor_game_train.h: the same arguments, rules and results) by the launches above. */
int tg_net_loss_grad_s25(const tg_net_config* cfg, const float* theta, const float* pos_fix, const void* frames,
                         int frames_is_i8, const float* scalars, const int8_t* g_action, const float* g_value, int64_t B,
                         float weight_pol, float weight_val, float dropout_p, uint64_t seed, uint64_t call,
                         const uint8_t* keep_in, uint8_t* keep_out, void* workspace, int64_t workspace_bytes, float* grad,
                         float* losses, uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_TRAIN_S25_H_ */
