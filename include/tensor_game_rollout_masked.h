/*
 * tensor_game_rollout_masked.h -- C ABI of libtensorgame.so, part 7b: the solution search that stops solved groups.
 * Included by tensor_game_rollout.h; conventions and layout are that header's.
 */
#ifndef TENSOR_GAME_ROLLOUT_MASKED_H_
#define TENSOR_GAME_ROLLOUT_MASKED_H_

#include "tensor_game_net.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tg_rollout_advance for the groups that are not solved yet, in ONE launch; unlike there, the rows of a solved group
 * are NOT stepped any more.
 *   A group g is ACTIVE in a launch iff solved_step[g] < 0 when the launch starts (the workgroup that owns the group
 *   reads this before it writes any record; no other workgroup touches the record).
 *   Active groups: everything tg_rollout_advance does, bit for bit (frames in place, the history shift, scalars += 1,
 *   nnz, overflow, the four records, actions[b][step]); then active[b] (uint8 (B), may be NULL) = 1 for the rows of a
 *   group that is still unsolved after this step, 0 for the rows of a group this step solved.
 *   Inactive groups: nothing of the group is read but solved_step[g] -- its tokens in particular are not -- and nothing
 *   is written: not frames, scalars, nnz, overflow, records, actions or active.  A workgroup none of whose groups is
 *   active returns before its first barrier.
 * The caller initialises `active` to 1 before step 0, as it initialises the records.  `active` is then the uint8 row
 * mask of tg_net_torso_masked / tg_net_sample_masked with need = 1, so the next network call skips the same rows.
 * hits[g] ends as 0 or 1; frames, scalars and nnz of a solved group stay as the solving step left them (the winning
 * row's head is zero); actions beyond solved_step keep what the caller put there.
 * Sizes, checks and their order are those of tg_rollout_advance. */
int tg_rollout_advance_masked(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz, uint8_t* overflow,
                              int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                              int8_t* actions, uint8_t* active, int64_t B, int n, int S, int T, int dim_s, int step,
                              int max_actions, int shift, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_ROLLOUT_MASKED_H_ */
