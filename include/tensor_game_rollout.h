/*
 * tensor_game_rollout.h -- C ABI of libtensorgame.so, part 7: sampled policy rollouts (the solution search).
 *
 * Replaces what the reference's SyntheticDemoTrainingApp does between two network calls of its solution search
 * (training.py:325-352): `_take_action` minus the model call (:253-268: the action tensor, the new head, the history
 * shift, scalar_batch + 1, rank_ubs and the best sample of every group) and the running statistics of the loop
 * (:343-346: lowest_rank, num_solutions_found) -- a dozen torch ops and two host-visible reductions per step -- by ONE
 * launch per step that leaves the model input of the next step in place.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).
 *
 * Layout.  B = G * n rows, GROUP-major: row g*n + s is sample s of start state g.  A row's state is its T frames,
 * int8 (T,S,S,S), C-contiguous, newest first -- exactly a frames_is_i8 = 1 input of tg_net_torso, so no float copy of
 * the state is ever made.  tokens int8 (B,3S) = cat(u,v,w) + shift is what tg_net_sample writes for k = 1.
 */
#ifndef TENSOR_GAME_ROLLOUT_H_
#define TENSOR_GAME_ROLLOUT_H_

#include "tensor_game_net.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step (index `step`) of every row, in ONE launch:
 *   frames    int8 (B,T,S,S,S), IN PLACE: new head = head - u(x)v(x)w of tokens[b], frame t -> t + 1, the oldest
 *             dropped (training.py:255-258).  The new head is computed in 32 bits and narrowed with wrap exactly as
 *             tg_step_i8 does; overflow[b] (uint8, may be NULL) is SET when an entry left int8, never cleared.
 *   tokens    int8 (B,3S).
 *   scalars   float32 (B,dim_s) += 1 (:268), or NULL (then dim_s is ignored).
 *   nnz       int32 (B): non-zero entries of the new head (rank_ubs, :266).
 *   per group (G = B / n entries each, int32, updated from this step's nnz; one writer per record, no atomics; rows
 *   keep being stepped after their group is solved, as in the reference; tg_rollout_advance_masked stops them).  The
 *   caller initialises them before step 0: best_nnz to any upper bound (S^3: the reference's lowest_rank starts there,
 *   training.py:329), hits to 0, solved_step and solved_sample to -1.
 *     best_nnz       running minimum of nnz over the steps so far and the n samples (:343-345 per group);
 *     hits           number of steps so far at which the group's minimum was 0; summed over the groups this is the
 *                    reference's num_solutions_found (:346);
 *     solved_step    -1 until the first such step, then that step's index, fixed;
 *     solved_sample  at that step, the LOWEST sample index with nnz == 0 (-1 before).
 *   actions   int8 (B,max_actions,3S) or NULL: actions[b][step] = tokens[b]; needs 0 <= step < max_actions.
 * Sizes: 1 <= S <= TG_MAX_S, 1 <= T <= TG_NET_MAX_T, 1 <= n <= TG_NET_MAX_SAMPLES, B % n == 0, 0 <= dim_s <= 64; B = 0
 * returns 0 at once.  Everything else is refused before any launch with a message naming the argument.  Any alignment
 * of frames is accepted; 16-byte aligned frames with S % 4 == 0 take 16-byte accesses. */
int tg_rollout_advance(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz, uint8_t* overflow,
                       int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample, int8_t* actions,
                       int64_t B, int n, int S, int T, int dim_s, int step, int max_actions, int shift,
                       tg_stream_t stream);

/* The size checks of tg_rollout_advance alone (no pointers, no device).  Host only. */
int tg_rollout_check(int64_t B, int n, int S, int T, int dim_s, int step, int max_actions, int with_actions);

#ifdef __cplusplus
}
#endif

/* tg_rollout_advance_masked: the same step for the groups that are not solved yet (solved groups are left alone) */
#include "tensor_game_rollout_masked.h"

#endif /* TENSOR_GAME_ROLLOUT_H_ */
