/*
 * tensor_game_search.h -- C ABI of libtensorgame.so, part 3: batched Monte Carlo tree search held in HBM.
 *
 * Replaces the reference's self-play search (act.py:8-301: actor_prediction -> mc_ts -> extend_tree ->
 * backward_pass / select_next_state / get_improved_policy), which plays ONE game in Python with the tree in host
 * dicts, by a forest of B independent trees -- one per game -- in caller-owned device memory.  One call runs one
 * simulation step for every game; the policy network stays a caller-supplied function between select and commit.
 *
 * Conventions: those of tensor_game.h (device pointers, asynchronous on `stream`, no allocation, no host sync,
 * capturable into a hipGraph, 0 or a negative TG_ERR_* with a message in tg_last_error()).  The forest descriptor
 * itself is a HOST struct passed by pointer; every pointer inside it is a device pointer.  No call touches another
 * game's memory, so games never synchronise with each other.
 *
 * Semantics (the reference's, with the two deviations marked DEVIATION):
 *   - nodes are keyed by the tg_hash_u64 key of the HEAD frame only (state_to_str(get_head_state(.))); a node keeps the
 *     T frames of the state it was expanded from and its children are [frames[0] - tensor(a_j), frames[0..T-2]]
 *     (get_child_states, act.py:266-275), so a node reached through a transposition yields its expansion-time frames;
 *   - select: from the root, follow the child of maximal Q (first maximal index wins, NaN counts as the maximum:
 *     select_next_state with its always-empty `reps`, act.py:240-263) while the key is a node; depth d gives
 *     idx = move + d.  The leaf is expanded when idx <= min(max_actions, move + horizon) and its head is not zero;
 *     past that bound it is only backed up (act.py:175-216);
 *   - commit: children of the leaf head from the model's k candidates, null candidates (child head == leaf head,
 *     remove_null_actions) and candidates whose key is already a node dropped, survivors kept in order (duplicates
 *     stay); none left = the game is flagged for a retry and nothing changes (the reference asks the model again);
 *   - backup (backward_pass, act.py:219-237) in float32, operation by operation as torch does it: reward = 0
 *     (+ leaf_q when the leaf was expanded); per path entry from the leaf up: reward -= 1;
 *     Q = (N*Q + reward) / (N + 1); N += 1.  Past the horizon the reference computes -get_rank but never adds it;
 *     neither does this;
 *   - DEVIATION 1: a leaf whose head is all zero inside the horizon makes the reference raise (UnboundLocalError on
 *     leaf_q_val, act.py:213); here its value is 0 = -rank(0);
 *   - DEVIATION 2: a descent that revisits nodes forever loops in the reference; here a descent longer than
 *     max_depth sets status bit 1 and the game skips that simulation;
 *   - move (mc_ts, act.py:67-112): the root's argmax-Q child (with its frames) becomes the next root; the next move
 *     runs n_sim minus the new root's visit sum simulations (at least 0); the game is done after max_actions moves
 *     or when the new root's head is all zero (the reference's loop ends the same way wherever it does not raise);
 *   - improved policy (get_improved_policy, act.py:278-301) over the roots of all moves played.
 *
 * Per-game status word (uint32): bit 0 = the node pool or the index was full (that simulation's expansion AND backup
 * were dropped), bit 1 = a descent exceeded max_depth, bit 2 = a token >= n_logits (or < 0) met by tg_search_policy.
 * overflow (uint8 per game) is SET when a child head left int8 (two's-complement wrap, as tensor_game.h), sticky.
 * The children that count are all k candidate children tg_search_commit forms for an EXPAND leaf, on every attempt,
 * including the candidates it then drops as null or as already a node; only tg_search_reset clears the flag.
 */
#ifndef TENSOR_GAME_SEARCH_H_
#define TENSOR_GAME_SEARCH_H_

#include "tensor_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_SEARCH_MAX_K 64     /* candidates per expansion (one per lane of a wavefront) */
#define TG_SEARCH_MAX_T 16     /* frames per state */
#define TG_SEARCH_MAX_DEPTH 4096
#define TG_SEARCH_MAX_ACTIONS 4096 /* moves per game */

/* flags[g] written by tg_search_select, updated by tg_search_commit */
#define TG_SEARCH_EXPAND 1u   /* the leaf is to be expanded: the model's output for it is needed */
#define TG_SEARCH_TERMINAL 2u /* the leaf head is all zero inside the horizon (backed up with value 0) */
#define TG_SEARCH_HORIZON 4u  /* the leaf lies past the horizon (backed up with no leaf value) */
#define TG_SEARCH_RETRY 8u    /* commit found no surviving candidate: ask the model again (attempt[g] counts) */
#define TG_SEARCH_PENDING 128u /* selected this simulation, not yet committed */

/* The forest: structure-of-arrays, caller-owned, B games of M nodes each.  FB = frame bytes = S^3 rounded up to a
 * multiple of 16 (the padding bytes are zero); every pointer 16-byte aligned.  [g][n] means g*M + n. */
typedef struct tg_search_forest {
  int64_t B;              /* games */
  int32_t S, T, k;        /* state size, frames per state (1..TG_SEARCH_MAX_T), candidates per expansion (1..64) */
  int32_t M;              /* nodes per game */
  int64_t index_capacity; /* slots of each game's key -> node index, a power of two (keep it >= 2 M) */
  int32_t max_actions;    /* moves per game, 1..TG_SEARCH_MAX_ACTIONS */
  int32_t horizon;        /* expansion bound: idx <= min(max_actions, move + horizon) */
  int32_t max_depth;      /* path entries per descent, 1..TG_SEARCH_MAX_DEPTH */
  int32_t shift;          /* factor value = token - shift */
  /* node pool */
  uint64_t* node_key;     /* [g][n] */
  int8_t* node_frames;    /* [g][n] T x FB bytes: the frames the node was expanded from */
  int32_t* node_nchild;   /* [g][n] */
  int8_t* child_tokens;   /* [g][n] k x 3S */
  uint64_t* child_key;    /* [g][n] k */
  float* child_n;         /* [g][n] k */
  float* child_q;         /* [g][n] k */
  float* child_prior;     /* [g][n] k, or NULL: NULL selects by Q alone (the reference) */
  /* per-game index: open addressing, linear probing from key & (capacity-1), empty slot = 0, a key equal to 0 is
   * stored as 0x9E3779B97F4A7C15 (the rule of tg_seen_u64) */
  uint64_t* index_key;    /* [g] capacity */
  int32_t* index_node;    /* [g] capacity */
  /* per-game state */
  int32_t* node_count;    /* [g] */
  int8_t* root_frames;    /* [g] T x FB */
  uint64_t* root_key;     /* [g] */
  int32_t* move;          /* [g] moves played */
  uint8_t* done;          /* [g] */
  int32_t* sims_left;     /* [g] simulations left in this move */
  uint32_t* status;       /* [g] */
  uint8_t* overflow;      /* [g] */
  /* per-simulation outputs of select (inputs of commit) */
  int8_t* leaf_frames;    /* [g] T x FB */
  uint64_t* leaf_key;     /* [g] */
  int32_t* path_node;     /* [g] max_depth */
  int32_t* path_slot;     /* [g] max_depth */
  int32_t* depth;         /* [g] */
  uint8_t* flags;         /* [g] TG_SEARCH_* */
  int32_t* attempt;       /* [g] model calls so far for this leaf (0 on select, +1 per retry) */
  /* trajectory: one row per move played */
  int8_t* traj_frames;    /* [g][m] T x FB: the root at the start of move m (actor_prediction's state_seq) */
  int32_t* traj_node;     /* [g][m] the root's node id, -1 where no move was played */
  int32_t* traj_choice;   /* [g][m] the child slot that became the next root */
} tg_search_forest;

/* Load the roots (states: int8 (B,T,S,S,S), C-contiguous, frame 0 = head) and empty every tree: index cleared, node
 * counts, moves, status, overflow and trajectory rows reset, sims_left = n_sim (>= 0), done = head all zero. */
int tg_search_reset(const tg_search_forest* f, const int8_t* states, int n_sim, tg_stream_t stream);

/* One descent per active game (sims_left > 0, not done): writes leaf_frames, leaf_key, path_node/path_slot, depth,
 * attempt = 0 and flags (PENDING | EXPAND, TERMINAL or HORIZON; 0 for inactive games and for a descent over
 * max_depth, which also sets status bit 1 and uses up the simulation).  model_in (may be NULL): the leaf frames as
 * (B,T,S,S,S) of out_dtype 0 = float32, 1 = float16, 2 = bfloat16 (rows of games not selected are not written);
 * scalars (float32 (B,1), may be NULL) = move + depth (get_scalars(state, idx)).  With child_prior the descent maximises
 * Q + (1.25 + log((sum N + 19653)/19652)) * prior * sqrt(sum N) / (1 + N) (select_next_state's c1, c2). */
int tg_search_select(const tg_search_forest* f, void* model_in, int out_dtype, float* scalars, tg_stream_t stream);

/* Finish the simulation of every game with flags & PENDING (and mask[g] != 0 where mask, uint8 (B), is given).
 * tokens: int8 (B,k,3S); leaf_q: float32 (B); prior: float32 (B,k) or NULL (stored when child_prior is set).
 * EXPAND games: children, keys (== tg_hash_u64 of the child head), both filters, compaction; no survivor -> RETRY,
 * attempt += 1, nothing else changes; otherwise a node is created (pool or index full: status bit 0, the expansion
 * and the backup are dropped) and the path is backed up with leaf_q.  TERMINAL / HORIZON games: backup only.  A
 * finished simulation clears PENDING and RETRY and decrements sims_left. */
int tg_search_commit(const tg_search_forest* f, const int8_t* tokens, const float* leaf_q, const float* prior,
                     const uint8_t* mask, tg_stream_t stream);

/* End the move of every game that is not done: record trajectory row `move` (root frames, root node, chosen slot),
 * make the root's argmax-Q child the root, move += 1, done when its head is all zero or move == max_actions,
 * sims_left = max(n_sim - visit sum of the new root's node, 0) (0 when done).  A root that never became a node (its
 * expansion was dropped) ends the game: status bit 0, done. */
int tg_search_advance(const tg_search_forest* f, int n_sim, tg_stream_t stream);

/* The improved policy of every (game, move < move[g]) into policy: float32 (B, max_actions, 3S, n_logits), zero
 * elsewhere.  sum = visit sum of the move's root; tau = log(sum)/log(n_bar) in float32 when sum > n_bar, else 1;
 * p_j = N_j^(1/tau) / sum; p_j is added to policy[g][m][s][token_j[s]] for every step s, samples in order.  A token
 * outside [0, n_logits) is skipped and sets status bit 2.  1 <= n_logits <= 256, n_bar >= 1. */
int tg_search_policy(const tg_search_forest* f, float* policy, int n_logits, int n_bar, tg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_GAME_SEARCH_H_ */
