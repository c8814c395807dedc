// A replay buffer's stored moves as dense arrays, out of the ring and back in (include/tensor_game_replay_io.h).  gfx950
// only; part of libtensorgame.so.
//
// tg_replay_pack: two launches, no host sync.
//   - pack_plan_kernel (one workgroup of 1024): every thread takes ceil(C / 1024) consecutive AGE positions (position j
//     is slot (ring[0] + j) mod C), counts its stored games and their moves, two block scans give each stored game its
//     rank and its first row; the plan writes the row to move_offset_out[rank], parks the slot in lengths_out[rank] and
//     writes (G, M);
//   - pack_copy_kernel (one workgroup per possible rank): reads its slot, replaces it by the length, and copies the
//     game's frames, tokens and rewards to its rows unless they would pass max_moves.
// tg_replay_add_packed: the three launches of the ring protocol (tg_ring.h).
//   - unpack_plan_kernel (one workgroup of 1024): walks the G lengths in chunks of 1024, twice: the first walk counts
//     the games that will be stored (a good length and rows inside M), the second is the plan; the parked index is the
//     game's first row;
//   - unpack_copy_kernel (one workgroup per stored game): frames, tokens and rewards from the rows into the slot;
//   - the rebuild of offset (tg_internal_ring_rebuild).
// Every copy picks its access width per game from the two addresses (copy_bytes, tg_ring.h).
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_replay_io.h"
#include "tg_host.h"
#include "tg_ring.h"

namespace tg {
namespace rio {

// the three arrays of one game: `len` moves from (frames, tokens, rewards) at sf/st/sr to df/dt/dr
__device__ __forceinline__ void copy_game(const tg_replay_buffer& b, int len, int8_t* df, const int8_t* sf, int8_t* dt,
                                          const int8_t* st, float* dr, const float* sr, int t) {
  const int64_t fb = static_cast<int64_t>(b.T) * b.S * b.S * b.S;  // bytes per state
  copy_bytes(df, sf, len * fb, t, kBlock);
  copy_bytes(dt, st, static_cast<int64_t>(len) * 3 * b.S, t, kBlock);
  for (int m = t; m < len; m += kBlock) dr[m] = sr[m];
}

// ---- tg_replay_pack -------------------------------------------------------------------------------------------------
struct PackArgs {
  tg_replay_buffer b;
  int64_t max_moves;
  int32_t* lengths;      // [C]
  int64_t* move_offset;  // [C+1]
  int64_t* counts;       // [2]
  float* rewards;
  int8_t* tokens;
  int8_t* frames;
  uint32_t* status;
};

// the moves slot s holds: 0 = empty; a length above L (an inconsistent buffer) counts as L
__device__ __forceinline__ int stored_len(const tg_replay_buffer& b, int64_t s) {
  const int len = b.length[s];
  return len < 0 ? 0 : (len > b.L ? b.L : len);
}

__global__ __launch_bounds__(kRingScanBlock) void pack_plan_kernel(PackArgs p) {
  __shared__ int64_t sh[kRingScanBlock];
  const int t = threadIdx.x;
  const int64_t C = p.b.C, next = ring_next(p.b);
  const int64_t per = (C + kRingScanBlock - 1) / kRingScanBlock;
  const int64_t lo = t * per < C ? t * per : C, hi = lo + per < C ? lo + per : C;
  int64_t cnt = 0, sum = 0;
  for (int64_t j = lo; j < hi; ++j) {
    const int len = stored_len(p.b, (next + j) % C);
    cnt += len > 0;
    sum += len;
  }
  int64_t G, M;
  int64_t rank = block_exclusive_scan(cnt, sh, &G);
  int64_t row = block_exclusive_scan(sum, sh, &M);
  for (int64_t j = lo; j < hi; ++j) {
    const int64_t slot = (next + j) % C;
    const int len = stored_len(p.b, slot);
    if (len > 0) {
      p.lengths[rank] = static_cast<int32_t>(slot);  // parked for the copy, which writes the length
      p.move_offset[rank] = row;
      ++rank;
      row += len;
    }
  }
  if (t == 0) {
    p.move_offset[G] = M;
    p.counts[0] = G;
    p.counts[1] = M;
    if (M > p.max_moves && p.status) atomicOr(p.status, TG_REPLAY_IO_TRUNCATED);  // the last game ends at M
  }
}

__global__ __launch_bounds__(kBlock) void pack_copy_kernel(PackArgs p) {
  const int64_t r = blockIdx.x;
  if (r >= p.counts[0]) return;
  const int t = threadIdx.x, L = p.b.L, A3 = 3 * p.b.S;
  const int64_t slot = p.lengths[r], row = p.move_offset[r];
  const int len = stored_len(p.b, slot);
  __syncthreads();  // every thread has read the parked slot
  if (t == 0) p.lengths[r] = len;
  if (row + len > p.max_moves) return;
  const int64_t fb = static_cast<int64_t>(p.b.T) * p.b.S * p.b.S * p.b.S;
  copy_game(p.b, len, p.frames + row * fb, p.b.frames + slot * L * fb, p.tokens + row * A3,
            p.b.tokens + slot * L * A3, p.rewards + row, p.b.rewards + slot * L, t);
}

// ---- tg_replay_add_packed -------------------------------------------------------------------------------------------
struct UnpackArgs {
  tg_replay_buffer b;
  const int8_t* frames;
  const int8_t* tokens;
  const float* rewards;
  const int32_t* lengths;
  int64_t G, M, first_slot, games_added;
  uint32_t* status;
};

// Game g0 + t of a chunk: its length (0 past G), its first row, and whether it is stored (a good length and rows inside
// M).  *base is the first row of the chunk and moves to the next chunk's.  flags collects the status bits.
__device__ __forceinline__ bool chunk_game(const UnpackArgs& p, int64_t g0, int64_t* sh, int64_t* base, int* len_out,
                                           int64_t* row_out, int* flags) {
  const int64_t g = g0 + threadIdx.x;
  const int len = g < p.G ? p.lengths[g] : 0;
  int64_t chunk;
  const int64_t row = *base + block_exclusive_scan(len > 0 ? len : 0, sh, &chunk);
  *base += chunk;
  const bool good = len >= 1 && len <= p.b.L, fits = row + len <= p.M;
  if (g < p.G && !good) *flags |= TG_REPLAY_IO_BAD_LENGTH;
  if (good && !fits) *flags |= TG_REPLAY_IO_TRUNCATED;
  *len_out = len;
  *row_out = row;
  return good && fits;
}

__global__ __launch_bounds__(kRingScanBlock) void unpack_plan_kernel(UnpackArgs p) {
  __shared__ int64_t sh[kRingScanBlock];
  const int t = threadIdx.x;
  const int64_t next = p.first_slot >= 0 ? p.first_slot : ring_next(p.b);
  int64_t cnt = 0, base = 0;  // base: the first row of the chunk a walk is at
  int flags = 0;
  const auto game = [&](int64_t g0, int32_t* len, int64_t* row) {
    return chunk_game(p, g0, sh, &base, len, row, &flags);
  };
  int32_t len;
  int64_t row;
  for (int64_t g0 = 0; g0 < p.G; g0 += kRingScanBlock) cnt += game(g0, &len, &row);
  const int bad = __syncthreads_or(flags & TG_REPLAY_IO_BAD_LENGTH), cut = __syncthreads_or(flags & TG_REPLAY_IO_TRUNCATED);
  if (t == 0 && p.status && (bad || cut))
    atomicOr(p.status, (bad ? TG_REPLAY_IO_BAD_LENGTH : 0u) | (cut ? TG_REPLAY_IO_TRUNCATED : 0u));
  int64_t V, n_surv;
  base = 0;  // the second walk starts at row 0 again
  ring_plan_all(p.b, next, p.G, cnt, sh, game, &V, &n_surv);
  ring_commit(p.b, next, V, n_surv, p.games_added);
}

__global__ __launch_bounds__(kBlock) void unpack_copy_kernel(UnpackArgs p) {
  int64_t slot, row;
  int len;
  if (!ring_survivor(p.b, blockIdx.x, &slot, &row, &len)) return;
  const int t = threadIdx.x, L = p.b.L, A3 = 3 * p.b.S;
  const int64_t fb = static_cast<int64_t>(p.b.T) * p.b.S * p.b.S * p.b.S;
  copy_game(p.b, len, p.b.frames + slot * L * fb, p.frames + row * fb, p.b.tokens + slot * L * A3,
            p.tokens + row * A3, p.b.rewards + slot * L, p.rewards + row, t);
}

}  // namespace rio
}  // namespace tg

extern "C" int tg_replay_pack(const tg_replay_buffer* buf, int64_t max_moves, int32_t* lengths_out,
                              int64_t* move_offset_out, int64_t* counts_out, float* rewards_out, int8_t* tokens_out,
                              int8_t* frames_out, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_replay_pack";
  if (!buf) return tg_internal_fail(TG_ERR_INVALID, "%s: null buffer", fn);
  if (int rc = check_ring_sizes(fn, "", buf)) return rc;
  if (max_moves < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: max_moves=%lld < 0", fn, (long long)max_moves);
  if (int rc = check_ring_arrays(fn, "", buf)) return rc;
  if (!lengths_out || !move_offset_out || !counts_out)
    return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths_out, move_offset_out or counts_out", fn);
  if (max_moves > 0 && (!rewards_out || !tokens_out || !frames_out))
    return tg_internal_fail(TG_ERR_INVALID, "%s: null rewards_out, tokens_out or frames_out", fn);
  if (!aligned(lengths_out, 4) || !aligned(move_offset_out, 8) || !aligned(counts_out, 8) || !aligned(rewards_out, 4) ||
      !aligned(status, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: lengths_out, move_offset_out, counts_out, rewards_out or status not "
                            "aligned to their elements", fn);
  const tg::rio::PackArgs p{*buf, max_moves, lengths_out, move_offset_out, counts_out, rewards_out, tokens_out,
                            frames_out, status};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = launch(fn, tg::rio::pack_plan_kernel, 1, tg::kRingScanBlock, 0, st, p)) return rc;
  return launch(fn, tg::rio::pack_copy_kernel, static_cast<unsigned>(buf->C), tg::kBlock, 0, st, p);
}

extern "C" int tg_replay_add_packed(const tg_replay_buffer* buf, const int8_t* frames, const int8_t* tokens,
                                    const float* rewards, const int32_t* lengths, int64_t G, int64_t M,
                                    int64_t first_slot, int64_t games_added, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_replay_add_packed";
  if (!buf) return tg_internal_fail(TG_ERR_INVALID, "%s: null buffer", fn);
  if (int rc = check_ring_sizes(fn, "", buf)) return rc;
  if (M < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld < 0", fn, (long long)M);
  if (G < 0 || G > (int64_t{1} << 31))
    return tg_internal_fail(TG_ERR_INVALID, "%s: G=%lld outside [0,2^31]", fn, (long long)G);
  if (first_slot < -1 || first_slot >= buf->C)
    return tg_internal_fail(TG_ERR_INVALID, "%s: first_slot=%lld outside [-1,%d)", fn, (long long)first_slot, buf->C);
  if (games_added < -1)
    return tg_internal_fail(TG_ERR_INVALID, "%s: games_added=%lld < -1", fn, (long long)games_added);
  if (int rc = check_ring_arrays(fn, "", buf)) return rc;
  if (G == 0) return TG_OK;
  if (!lengths) return tg_internal_fail(TG_ERR_INVALID, "%s: null lengths", fn);
  if (M > 0 && (!frames || !tokens || !rewards))
    return tg_internal_fail(TG_ERR_INVALID, "%s: null frames, tokens or rewards", fn);
  if (!aligned(lengths, 4) || !aligned(rewards, 4) || !aligned(status, 4))
    return tg_internal_fail(TG_ERR_INVALID, "%s: lengths, rewards or status not aligned to their elements", fn);
  const tg::rio::UnpackArgs p{*buf, frames, tokens, rewards, lengths, G, M, first_slot, games_added, status};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t copies = G < buf->C ? G : buf->C;
  if (int rc = launch(fn, tg::rio::unpack_plan_kernel, 1, tg::kRingScanBlock, 0, st, p)) return rc;
  if (int rc = launch(fn, tg::rio::unpack_copy_kernel, static_cast<unsigned>(copies), tg::kBlock, 0, st, p)) return rc;
  return tg_internal_ring_rebuild(buf, st);
}
