/*
 * tensor_game_demos.h -- C ABI of libtensorgame.so, part 2: items of a synthetic-demonstration set.
 *
 * Replaces SyntheticDemoDataset.__getitem__ (reference datasets.py:78-122) as the shuffling
 * DataLoader of SyntheticDemoTrainingApp.init_dl (training.py:243-246) calls it: one call gathers a
 * whole batch of items, each with its own (demo, action index), on the GPU in one launch.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host
 * sync, capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).
 */
#ifndef TENSOR_GAME_DEMOS_H_
#define TENSOR_GAME_DEMOS_H_

#include "tensor_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_DEMO_MAX_ACTIONS 4096 /* R (max_actions) per demo */
#define TG_DEMO_MAX_T 4096       /* T (dim_t) history frames per item */

/* Items of a demo set, in the flat reference indexing of datasets.py:80-81: item n is demo d = idx[n] / R at action
 * index k = idx[n] % R.  Its outputs are those of __getitem__:
 *   frames[n][0]    = targets[d] - sum_{j > k} tensor(a_j)             (the suffix replay, datasets.py:90-92; exact)
 *   frames[n][f]    = tensor(a_{k+m+1-f}) for f = 1..m, m = min(T-1, R-1-k)  (reversed(action_seq[k+1:k+T]), :97-102)
 *   frames[n][f]    = 0 for f > m                                      (zero padding, :105-114)
 *   scalars_out[n]  = R - k,  actions_out[n] = tokens[d][k],  rewards_out[n] = -(k+1)             (:116-122)
 * tokens: int8 (n_demos,R,3S), C-contiguous; targets: int8 (S,S,S) per demo at targets + d*target_stride_bytes
 * (>= S^3).  idx: int64 (N).  frames_out: C-contiguous (N,T,S,S,S) of out_dtype 0 = float32, 1 = float16,
 * 2 = bfloat16 (the int8 value, exact in all three, as tg_emit_frames) or 3 = int8, aligned to its element size.
 * scalars_out, rewards_out: float32 (N,1); actions_out: int8 (N,3S); each may be NULL.
 * Every frame entry is the int8 (two's-complement wrap) of its exact value; overflow[n] (uint8, may be NULL) is SET
 * when any exact value of the item's frames leaves [-128,127], sticky.  Unlike tg_step_many_i8, which narrows after
 * every step and flags intermediate states, the suffix is summed without intermediate narrowing -- the reference's
 * float arithmetic -- so only the final values count.
 * An index outside [0, n_demos*R) gives an all-zero item (frames, scalar, action, reward) and sets bit 0 of
 * *status (uint32, may be NULL); nothing outside tokens / targets is read and the other items are unaffected.
 * Repeated indices are allowed; N = 0 is a no-op.  Sizes: 1 <= S <= TG_MAX_S, 1 <= R <= TG_DEMO_MAX_ACTIONS,
 * 1 <= T <= TG_DEMO_MAX_T.  One kernel launch. */
int tg_demo_items(const int8_t* tokens, const int8_t* targets, int64_t n_demos, int R, int S,
                  int64_t target_stride_bytes, const int64_t* item_idx, int64_t N, int T, int out_dtype,
                  void* frames_out, float* scalars_out, int8_t* actions_out, float* rewards_out,
                  uint8_t* overflow, uint32_t* status, int shift, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_DEMOS_H_ */
