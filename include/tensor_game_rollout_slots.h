/*
 * tensor_game_rollout_slots.h -- C ABI of libtensorgame.so, part 7c: the solution search over a QUEUE of start states.
 *
 * tg_rollout_advance_masked stops a solved group, but its rows stay idle until the caller starts a new batch.  Here the
 * B = R * n rows are R SLOTS of n rows (laid out exactly as the groups of tensor_game_rollout.h): a slot holds one state
 * of a device-resident queue of N start states, is stepped until it is solved or max_actions steps have run, is then
 * flushed to dense per-state outputs and takes the next state of the queue -- all on the device, so every network
 * launch stays full until the queue is drained and the host only reads one word (`live`) now and then.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error(); sizes are checked before
 * pointers, pointers before alignment, all before any launch).  No global atomics: the assignment of states to slots
 * is a scan in slot order, so two runs are equal bit for bit.
 *
 * Per slot, besides the four group records, there are two words:
 *   slot_state  int64 (R): the index of the queue state the slot holds, < 0 when it is empty;
 *   slot_step   int32 (R): the number of steps this state has been advanced.
 * A row's random stream is keyed by (first_state + slot_state) * n + sample and by slot_step: by the state and the
 * row's OWN step, never by the tick or the slot, so a state's search does not depend on R or on its neighbours.
 */
#ifndef TENSOR_GAME_ROLLOUT_SLOTS_H_
#define TENSOR_GAME_ROLLOUT_SLOTS_H_

#include "tensor_game_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_ROLLOUT_MAX_SLOTS 65536 /* R = B / n of both entries */

/* tg_rollout_advance_masked with every slot at its own step, in ONE launch.
 *   A slot g is LIVE in a launch iff, when the launch starts, slot_state[g] >= 0, solved_step[g] < 0 and
 *   slot_step[g] < max_actions (the workgroup that owns the slot reads the three words before it writes any of them).
 *   Live slots: bit for bit what tg_rollout_advance_masked gives an active group with step := slot_step[g] (frames in
 *   place, scalars += 1, nnz, overflow, the four records with solved_step = slot_step[g], actions[b][slot_step[g]],
 *   active[b]); then slot_step[g] += 1, by the thread that writes the group's records.
 *   Slots that are not live: nothing but those three words is read -- the tokens in particular are not -- and nothing
 *   is written.  A workgroup none of whose slots is live returns before its first barrier.
 * slot_state int64 (R) is only read.  actions int8 (B,max_actions,3S) may be NULL; max_actions >= 1 is needed either
 * way.  Sizes as tg_rollout_advance, and B / n <= TG_ROLLOUT_MAX_SLOTS; B = 0 returns 0 at once. */
int tg_rollout_advance_slots(int8_t* frames, const int8_t* tokens, float* scalars, int32_t* nnz, uint8_t* overflow,
                             int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                             int8_t* actions, uint8_t* active, const int64_t* slot_state, int32_t* slot_step, int64_t B,
                             int n, int S, int T, int dim_s, int max_actions, int shift, tg_stream_t stream);

/* Flush the finished slots, hand the next queue states to the finished and the empty ones, and prepare the next network
 * call, in TWO launches (a one-workgroup plan, then one workgroup per slot).
 *   queue:   q_states int8 (N,T,S,S,S), q_scalars float32 (N,dim_s) (NULL iff scalars is NULL), head int64 [1]: the
 *            next state to hand out (the caller sets it to 0 before the first call).
 *   1. A slot is FINISHED iff slot_state >= 0 and (solved_step >= 0 or slot_step >= max_actions).  Every finished slot
 *      is flushed to its state q = slot_state: out_best_nnz, out_hits, out_solved_step, out_solved_sample int32 (N)
 *      receive the four records, out_overflow uint8 (N) the OR of the rows' overflow flags, out_tokens int8
 *      (N,max_actions,3S) the winning row's actions[.][0 .. solved_step] with zeros beyond (all zeros for a state
 *      that was not solved: all max_actions rows are written).
 *   2. The j-th finished-or-empty slot in slot order takes state head + j if that is < N, else it becomes or stays
 *      empty (slot_state = -1); then head += min(their number, N - head).
 *   3. A slot that takes state q: the T frames of q into each of its n rows, its scalars n times, fresh records
 *      (S^3, 0, -1, -1), slot_state = q, slot_step = 0, nnz = 0 and overflow = 0 on its rows, and
 *      rows[g*n + s] = (first_state + q) * n + s (int64 (B): the stream keys).  The rows of a slot that becomes or
 *      stays empty get rows = -1; a slot that is kept keeps its rows.
 *   4. active[b] (uint8 (B), may be NULL) = 1 on the rows of every slot that now holds an unfinished state, else 0;
 *      live[0] (int32) = the number of such slots.
 *   5. uniforms float32 (B,1,n_uniforms) or NULL (then n_uniforms is ignored; else n_uniforms = 3S): for the rows of
 *      those slots, uniforms[b][0][t] = the sampling rule of tensor_game_net.h at (row key rows[b], call = the slot's
 *      slot_step, sample 0, t) under `seed`: what tg_net_sample draws itself with call = the row's own step.  Other
 *      rows keep what they held.
 * With every slot empty the call is the initial fill.  16-byte copies when S % 4 == 0 and q_states and frames are
 * 16-byte aligned, else unaligned dwords with a byte tail.  Sizes as tg_rollout_advance_slots, N >= 0, first_state
 * >= 0; B = 0 and N = 0 return 0 at once, after the size checks (nothing is flushed, head and live are not written). */
int tg_rollout_refill(const int8_t* q_states, const float* q_scalars, int64_t N, int64_t* head, int64_t first_state,
                      uint64_t seed, int n_uniforms, int8_t* frames, float* scalars, int32_t* nnz, uint8_t* overflow,
                      int32_t* best_nnz, int32_t* hits, int32_t* solved_step, int32_t* solved_sample,
                      const int8_t* actions, uint8_t* active, int64_t* slot_state, int32_t* slot_step,
                      int32_t* out_best_nnz, int32_t* out_hits, int32_t* out_solved_step, int32_t* out_solved_sample,
                      uint8_t* out_overflow, int8_t* out_tokens, int64_t* rows, float* uniforms, int32_t* live,
                      int64_t B, int n, int S, int T, int dim_s, int max_actions, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_ROLLOUT_SLOTS_H_ */
