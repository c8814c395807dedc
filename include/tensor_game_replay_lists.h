/*
 * tensor_game_replay_lists.h -- C ABI of libtensorgame.so: move lists of the solution search, stored as games.
 *
 * The solution search (tensor_game_rollout*.h, tensor_game_solutions.h, tensor_game_bases.h) ends with move lists that
 * take a start state to zero: a start state per group and int8 tokens (M,K,3S).  tg_replay_add wants what the self-play
 * search returns instead: the padded states of every move, a float policy of which only the argmax is kept, and the
 * rewards.  This entry replays a list from its start state on the device and writes the game it describes -- frames,
 * tokens, rewards -- straight into a ring of tensor_game_replay.h, so the factorisations the network found can be trained
 * on (the reference's act_step keeps its best game for the same reason, training.py:468-483).
 *
 * Conventions: those of tensor_game_replay.h (a host descriptor of device pointers, asynchronous on `stream`, no
 * allocation, no host sync, capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error(); every
 * refusal is made before any launch and names the argument; sizes are checked before pointers).
 */
#ifndef TENSOR_GAME_REPLAY_LISTS_H_
#define TENSOR_GAME_REPLAY_LISTS_H_

#include "tensor_game_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of *status: why a list was not stored (bit 0 is the bit tg_replay_add sets for a game it does not store) */
#define TG_REPLAY_LISTS_BAD_LENGTH 1u /* lengths[m] < 1, > K or > buf.L */
#define TG_REPLAY_LISTS_BAD_GROUP 4u  /* groups[m] < 0 or >= G */
#define TG_REPLAY_LISTS_BAD_RANGE 8u  /* an entry of some head_1 .. head_L lies outside [-128,127] */
#define TG_REPLAY_LISTS_NOT_ZERO 16u  /* head_L has a non-zero entry */
#define TG_REPLAY_LISTS_MAX_SHIFT 64

/* Replay M move lists from their start states and store the games in the ring `buf`.
 *   starts  int8 (G,T,S,S,S), T and S the buffer's: frame 0 of starts[g] is the tensor to factorise, frames 1 .. T-1 the
 *           history before it (newest first), as a state of the search holds them;
 *   groups  int64 (M) or NULL: list m starts from starts[groups[m]]; with NULL from starts[m], and M <= G is required;
 *   tokens  int8 (M,K,3S) = cat(u,v,w) + shift of every move, any alignment;   lengths int64 (M);
 *   stored  uint8 (M) or NULL;   status uint32 (1) or NULL: bits are ORed in and never cleared.
 * For list m, with g = groups[m] (or m) and L = lengths[m]:
 *   Replay, in 32-bit integers (wrapping, should a sum leave them): head_0 = starts[g][0], head_{t+1} = head_t - u (x) v
 *   (x) w with (u,v,w) = tokens[m][t] - shift.  Rows t >= L of the list are not read.
 *   The list is VALID when all four hold:
 *     1 <= L <= min(K, buf.L)                                      else TG_REPLAY_LISTS_BAD_LENGTH;
 *     0 <= g < G                                                   else TG_REPLAY_LISTS_BAD_GROUP;
 *     every entry of every head_1 .. head_L lies in [-128,127]     else TG_REPLAY_LISTS_BAD_RANGE (the int8 steppers
 *                                                                  wrap there; this entry does not);
 *     head_L is zero everywhere                                    else TG_REPLAY_LISTS_NOT_ZERO.
 *   The length and the group index are checked first, each on its own, and before either addresses anything: a list that
 *   fails one of them is not replayed and sets only those bits.  A replayed list sets each of the last two bits it has
 *   earned (a list whose wrapped int8 replay ends at zero and whose exact one does not sets both).  An invalid list
 *   stores nothing and leaves every other list untouched.  Lists that do not end at zero are out of scope (the
 *   reference's end reward for them is -get_rank).
 *   The stored game, in the layout of tensor_game_replay.h: move t < L has
 *     frames[slot][t][f] = head_{t-f} for f <= t, and starts[g][f-t] for t < f < T -- what get_child_states
 *                          (act.py:266-275) leaves after t moves from starts[g];
 *     tokens[slot][t]    = the list's token bytes tokens[m][t];
 *     rewards[slot][t]   = -(t+1) as float32: reward_seq of act.py:59-62 with an end state of rank 0.
 *   select = 0: every valid list, in list order, into consecutive slots modulo C from ring[0]; when more than C are valid
 *               only the last C are written, as sequential add_game calls leave it;
 *   select = 1: only the FIRST valid list with the least L, i.e. the greatest final reward -L, the first maximum winning
 *               (tg_replay_add's select rule); nothing is stored when no list is valid.
 *   stored[m] = 1 where list m was stored by this call, else 0: with select = 0 every valid list, also one that a later
 *   list of the same call overwrote; with select = 1 the winner only.
 * length, offset and ring are brought up to date by the same call.  Afterwards every valid byte of the buffer (frames,
 * tokens and rewards below each slot's length; length, offset, ring) equals what tg_replay_add(select) leaves when given,
 * for the valid lists only, the padded states defined above, the one-hot policies of the tokens and these rewards.
 * Every output byte has one writer, so two runs agree bit for bit; no floating point is used beyond writing the reward.
 * Nothing outside [slot][t < L] of frames, tokens and rewards is written.
 *
 * Limits: M >= 0 (0 returns 0 at once, before any pointer is looked at), G >= 0, 1 <= K <= TG_REPLAY_MAX_ACTIONS,
 * 0 <= shift <= TG_REPLAY_LISTS_MAX_SHIFT, select 0 or 1; C, L, T, S as tg_replay_add accepts them.  lengths, groups and
 * status must be aligned to their elements.
 *
 * Launches: FOUR with `stored`, three without, no host sync between them:
 *   validity (one workgroup per list: the replay row by row in registers, nothing stored but stored[m] and the
 *   status bits), plan (one workgroup: slots, lengths, ring words, the final stored[]), emit (per stored game one
 *   workgroup, or one per 2048 entries of the tensor when S^3 > 1024), offset scan (one workgroup over C).
 * With stored == NULL there is nowhere to keep the validity of M lists, so the plan replays the lists itself, one thread
 * per list, twice: correct but slow -- pass `stored` where M is large. */
int tg_replay_add_lists(const tg_replay_buffer* buf, const int8_t* starts, int64_t G, const int64_t* groups,
                        const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int shift, int select,
                        uint8_t* stored, uint32_t* status, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_REPLAY_LISTS_H_ */
