/*
 * tensor_game_replay.h -- C ABI of libtensorgame.so, part 4: replay buffers of played games and mixed training batches.
 *
 * Replaces the reference's PlayedGamesDataset ring (datasets.py:161-230: three torch.save pickles per game, a Python
 * walk over game_lengths per __getitem__) by a ring of finished games in caller-owned device memory, and the item
 * gathering of TensorGameDataset (datasets.py:233-359: synthetic demos, played games and best games mixed in fixed
 * fractions) by ONE launch per batch.  The self-play search (tensor_game_search.h) -> buffer -> training batch loop
 * then needs no host round trip.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  The buffer descriptor is a
 * HOST struct passed by pointer; every pointer inside it is a device pointer.  An add and a gather that use the same
 * buffer must be ordered (one stream, or events): an add rewrites slots and offsets in place.
 */
#ifndef TENSOR_GAME_REPLAY_H_
#define TENSOR_GAME_REPLAY_H_

#include "tensor_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_REPLAY_MAX_CAPACITY 65536 /* games per buffer: the offset scan of tg_replay_add is one workgroup */
#define TG_REPLAY_MAX_ACTIONS 4096   /* L: moves per slot */
#define TG_REPLAY_MAX_T 16           /* frames per stored state */
#define TG_REPLAY_MAX_LOGITS 128     /* n_logits of the policy (a stored token is its int8 argmax) */

/* kinds of a dataset row (tg_replay_items) */
#define TG_REPLAY_SYNTH 0  /* a synthetic demo item (tg_demo_items' flat index) */
#define TG_REPLAY_PLAYED 1 /* a move of the played-games buffer */
#define TG_REPLAY_BEST 2   /* a move of the best-games buffer */

/* A ring of C finished games of up to L moves (PlayedGamesDataset).  Slot s holds a game of length[s] moves, 0 = empty;
 * its move m (m < length[s]) is frames[s][m] (the T frames of the state the move was played from), tokens[s][m]
 * (the argmax tokens of the move's policy) and rewards[s][m].  offset[s] = length[0] + ... + length[s-1] (offset[C]
 * = every stored move): flat move index i lies in the slot s with offset[s] <= i < offset[s+1], in SLOT order, as the
 * reference walks game_lengths.  ring[0] = the next slot to write, ring[1] = games ever added.  Every entry that
 * stores games leaves ring[0] in [0, C) and takes any other value it finds there modulo C, so no slot index leaves the
 * buffer.  Create it zeroed (lengths, offsets, ring); contents past a slot's length are unspecified. */
typedef struct tg_replay_buffer {
  int32_t C, L, T, S;     /* capacity (1..TG_REPLAY_MAX_CAPACITY), moves per slot, frames per state, state size */
  int8_t* frames;         /* [C][L][T][S^3] */
  int8_t* tokens;         /* [C][L][3S] */
  float* rewards;         /* [C][L] */
  int32_t* length;        /* [C] */
  int64_t* offset;        /* [C+1] */
  int64_t* ring;          /* [2] */
} tg_replay_buffer;

/* Store finished games -- what search.actor_prediction returns -- in the ring, as PlayedGamesDataset.add_game
 * (datasets.py:210-230) does once per game, in batch order:
 *   states  int8 (B,L,T,S,S,S), policy float32 (B,L,3S,n_logits), rewards float32 (B,L), lengths int64 (B),
 * L, T, S those of the buffer.  Move m < lengths[b] of game b is stored as frames = states[b][m], tokens =
 * argmax over n_logits of policy[b][m] (datasets.py:206: the first maximal index, NaN counts as the maximum, as torch's
 * argmax) and rewards[b][m]; the float policy is not kept.
 *   select = 0: every game with 1 <= length <= L, into consecutive slots modulo C; when one call brings more than C
 *               such games only the last C are written, which is what sequential add_game calls leave;
 *   select = 1: only the FIRST game with the greatest final reward rewards[b][length_b - 1] (act_step's best-game rule,
 *               training.py:468-483: strict > from -1e6, so the first maximum wins; a NaN never wins; nothing is
 *               stored when no final reward exceeds -1e6).
 * A game with length 0 or length > L is not stored and sets bit 0 of *status (uint32, may be NULL).  offset and ring
 * are brought up to date by the same call.  Three launches (plan, copy, offset scan; the scan is one workgroup over
 * C).  1 <= n_logits <= TG_REPLAY_MAX_LOGITS, B >= 0 (0 is a no-op), select 0 or 1. */
int tg_replay_add(const tg_replay_buffer* buf, const int8_t* states, const float* policy, int n_logits,
                  const float* rewards, const int64_t* lengths, int64_t B, int select, uint32_t* status,
                  tg_stream_t stream);

/* Items of a mixed dataset (TensorGameDataset.__getitem__, datasets.py:286-303) for a batch of dataset indices, in ONE
 * kernel launch, in exactly the layout of tg_demo_items: frames_out (N,T,S,S,S) of out_dtype (0 float32, 1 float16,
 * 2 bfloat16, 3 int8; aligned to its element size), scalars_out and rewards_out float32 (N,1), actions_out int8 (N,3S),
 * overflow uint8 (N) (set, sticky), status uint32; every output but frames_out may be NULL.
 * Sources: the synthetic set (tokens, targets, n_demos, R, target_stride_bytes, shift: as tg_demo_items; n_demos may be
 * 0 with NULL tokens / targets), the played buffer and the best buffer (each may be NULL: it then holds nothing).
 * Row n: dataset index x = item_idx[n].  With an epoch table (kind uint8 [len_data], src int64 [len_data]) the row is of
 * kind[x] at source index src[x]; with kind == NULL every row is of kind direct_kind at source index x (src unused).
 *   TG_REPLAY_SYNTH  : byte-identical to tg_demo_items at flat index src (overflow flag included);
 *   TG_REPLAY_PLAYED, TG_REPLAY_BEST: PlayedGamesDataset.__getitem__ (datasets.py:189-208) at flat move index src of
 *                      that buffer as it is when the kernel runs: frames = the stored T frames, scalar = the move index
 *                      m (get_scalars(state, idx, batch_size=False), NOT R - k as for demos), action = the stored
 *                      tokens, reward = the stored reward.  overflow is not touched (stored frames are exact).
 * A kind outside 0..2, a dataset index outside [0, len_data) or a source index outside its source gives an all-zero
 * item and sets bit 0 of *status; nothing outside the sources is read.  Sizes: the synthetic limits of tg_demo_items;
 * each buffer's S and T must equal S and T (refused here otherwise).  The kernel is the one tg_demo_items picks for
 * (S, R); the branch on a row's kind is per workgroup (per 16 lanes at S = 4). */
int tg_replay_items(const int8_t* tokens, const int8_t* targets, int64_t n_demos, int R, int S,
                    int64_t target_stride_bytes, int shift, const tg_replay_buffer* played,
                    const tg_replay_buffer* best, const uint8_t* kind, const int64_t* src, int64_t len_data,
                    int direct_kind, const int64_t* item_idx, int64_t N, int T, int out_dtype, void* frames_out,
                    float* scalars_out, int8_t* actions_out, float* rewards_out, uint8_t* overflow,
                    uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_REPLAY_H_ */
