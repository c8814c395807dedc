/*
 * tensor_game_replay_io.h -- C ABI of libtensorgame.so, part 4b: a replay buffer's stored moves as dense arrays, out of
 * the ring and back into one.
 *
 * A ring (tensor_game_replay.h) is [C][L][T][S^3] bytes, most of it past the games' lengths.  To save it, move it to
 * another capacity or hand it to the reference's PlayedGamesDataset it has to leave the device as its stored moves
 * only, and come back without a float policy: tg_replay_add takes (B,L,3S,n_logits) float32 and keeps the argmax.  The
 * two entries here are that pack and that add.
 *
 * Conventions: those of tensor_game_replay.h (the descriptor is a host struct of device pointers; asynchronous on
 * `stream`, no allocation, no host sync, capturable; 0 or a negative TG_ERR_* with a message in tg_last_error(); sizes
 * are checked before pointers, both before any launch).  A call here and any other call on the same buffer must be
 * ordered (one stream, or events).
 *
 * The dense form of G games with M moves in all:
 *   lengths int32 [G]      (moves of game r)
 *   rewards float32 [M],  tokens int8 [M][3S],  frames int8 [M][T][S^3]
 * where move m of game r is row (lengths[0] + ... + lengths[r-1]) + m.
 */
#ifndef TENSOR_GAME_REPLAY_IO_H_
#define TENSOR_GAME_REPLAY_IO_H_

#include "tensor_game_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of *status */
#define TG_REPLAY_IO_BAD_LENGTH 1u /* tg_replay_add_packed: a game with length < 1 or > L (bit 0, as tg_replay_add) */
#define TG_REPLAY_IO_TRUNCATED 2u  /* a game whose rows would pass max_moves (pack) or M (add_packed): not copied */

/* Write the stored games of a buffer densely, in AGE order: age position j = 0 .. C-1 is slot (ring[0] + j) mod C, the
 * stored games are the positions with length > 0, in increasing j (for a ring filled by tg_replay_add: oldest first).
 * With G stored games of M moves in all:
 *   lengths_out     int32 [C]    : its first G entries are set (the game lengths);
 *   move_offset_out int64 [C+1]  : its first G+1 entries are set: the exclusive prefix sums of those lengths,
 *                                  move_offset_out[G] = M;
 *   counts_out      int64 [2]    : (G, M);
 *   rewards_out float32 [max_moves], tokens_out int8 [max_moves][3S], frames_out int8 [max_moves][T][S^3]:
 *                                  move m of the game of rank r goes to row move_offset_out[r] + m.
 * max_moves is what the three row outputs hold (they may be NULL when it is 0).  A game whose rows would pass it is
 * not written and sets bit 1 of *status (uint32, may be NULL); counts_out still reports the full G and M, so a caller
 * can size a second call.  Nothing at or past row M is written and nothing of the buffer is modified.
 * Two launches: a plan (one workgroup: a block scan over ceil(C / 1024) consecutive age positions per thread) and a
 * copy (one workgroup per age rank; frames move by 16 bytes when source and destination are both 16-byte aligned, by
 * dwords when both are 4-byte aligned, else by bytes).  Between the two launches lengths_out[r] holds the SLOT of
 * rank r (the plan parks it there; the copy replaces it by the length), so lengths_out is valid only after the call's
 * work has completed, like every other output.  Every output word's final value has one writer: two runs agree bit for
 * bit. */
int tg_replay_pack(const tg_replay_buffer* buf, int64_t max_moves, int32_t* lengths_out, int64_t* move_offset_out,
                   int64_t* counts_out, float* rewards_out, int8_t* tokens_out, int8_t* frames_out, uint32_t* status,
                   tg_stream_t stream);

/* Store G games given in the dense form above: lengths int32 [G], and M rows of rewards float32 [M], tokens int8
 * [M][3S], frames int8 [M][T][S^3] (T, S those of the buffer; the three may be NULL when M is 0).  Game g's rows start
 * at the exclusive prefix sum of max(lengths, 0).
 *   - A game with length < 1 or length > L is not stored and sets bit 0 of *status, as tg_replay_add does; its rows
 *     are skipped.  A game (of a good length) whose rows would pass M is not stored and sets bit 1.  Nothing at or past
 *     row M is read.
 *   - first_slot = -1 continues at ring[0]; 0 <= first_slot < C places the first stored game there.  The stored games
 *     go to consecutive slots modulo C; when a call brings more than C only the last C are written.
 *   - offset and ring[0] are brought up to date; ring[1] grows by the stored count, or is set to games_added when that
 *     is >= 0 (-1: grow).
 * With first_slot = -1 and games_added = -1 the call leaves every valid byte of the buffer (frames, tokens and rewards
 * below each slot's length; length, offset and ring) equal to tg_replay_add(select = 0) of the same games in padded
 * form with one-hot policies.
 * Three launches: a plan (one workgroup; block scans over the G lengths in chunks of 1024; it parks each stored game's
 * first row in offset[slot], which the scan rebuilds), a copy (one workgroup per stored game, the access width chosen
 * per game as in tg_replay_pack) and the offset scan.  0 <= G <= 2^31 (0 is a no-op), M >= 0. */
int tg_replay_add_packed(const tg_replay_buffer* buf, const int8_t* frames, const int8_t* tokens, const float* rewards,
                         const int32_t* lengths, int64_t G, int64_t M, int64_t first_slot, int64_t games_added,
                         uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_REPLAY_IO_H_ */
