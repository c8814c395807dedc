// Batched device-resident MCTS (include/tensor_game_search.h): a forest of B independent search trees in HBM, one
// wavefront per game in every kernel.  gfx950 only; part of libtensorgame.so.
//
// Kernels (each launch covers every game; games never touch each other's memory, so no cross-game atomics):
//   reset   -- roots in, index cleared;
//   select  -- one descent per game: at each level the children's Q values sit one per lane and the argmax is a
//              butterfly reduction with a first-index tie-break; each level's index lookup probes 64 consecutive slots
//              at once (one per lane) and ballots the hit / the first empty slot;
//   commit  -- the k children of the leaf head are formed chunk-parallel, child by child, their keys reduced across the
//              wave and kept in lane j's registers; both filters and the ballot/mbcnt compaction follow; the backup
//              walks the path serially in lane 0 with the float32 operations of torch, in torch's order;
//   advance -- the move: argmax child of the root becomes the root;
//   policy  -- the improved policy, one wavefront per (game, move), one lane per token step.
// The work per descent level is a chain of dependent loads (index slot, node row, child key): latency-bound.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cmath>

#include "../../include/tensor_game.h"
#include "../../include/tensor_game_search.h"
#include "tg_device.h"
#include "tg_host.h"

namespace tg {
namespace search {

constexpr uint64_t kZeroKey = 0x9E3779B97F4A7C15ull;  // the stored form of key 0 (tg_seen_u64's rule)
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ int64_t frame_bytes(int S) { return ((static_cast<int64_t>(S) * S * S + 15) / 16) * 16; }

// ---- the per-game index ---------------------------------------------------------------------------------------

// Node id of `key` in game g's index, or -1.  Wave-uniform key and result; every lane must call.  64 consecutive
// probe slots per round, one per lane: the first hit before the first empty slot decides.
__device__ int index_lookup(const tg_search_forest& f, int64_t g, uint64_t key) {
  const int lane = lane_id();
  const uint64_t k = key ? key : kZeroKey;
  const int64_t cap = f.index_capacity;
  const uint64_t mask = static_cast<uint64_t>(cap - 1);
  const uint64_t* tab = f.index_key + g * cap;
  for (int64_t base = 0; base < cap; base += 64) {
    const bool in = base + lane < cap;
    const uint64_t slot = (k + static_cast<uint64_t>(base + lane)) & mask;
    const uint64_t t = in ? tab[slot] : 1ull;  // lanes past the capacity: neither hit nor empty (k is never 1 here ...
    const uint64_t hit = __ballot(in && t == k);  // ... unless it is, which `in` excludes)
    const uint64_t empty = __ballot(in && t == 0);
    if (hit | empty) {
      const int fh = hit ? __builtin_ctzll(hit) : 64;
      const int fe = empty ? __builtin_ctzll(empty) : 64;
      if (fh < fe) return f.index_node[g * cap + static_cast<int64_t>((k + static_cast<uint64_t>(base + fh)) & mask)];
      return -1;
    }
  }
  return -1;
}

// The same for one lane on its own key (divergent callers allowed): a plain linear probe.
__device__ bool index_contains_lane(const tg_search_forest& f, int64_t g, uint64_t key) {
  const uint64_t k = key ? key : kZeroKey;
  const int64_t cap = f.index_capacity;
  const uint64_t mask = static_cast<uint64_t>(cap - 1);
  const uint64_t* tab = f.index_key + g * cap;
  uint64_t slot = k & mask;
  for (int64_t p = 0; p < cap; ++p) {
    const uint64_t t = tab[slot];
    if (t == k) return true;
    if (t == 0) return false;
    slot = (slot + 1) & mask;
  }
  return false;
}

// Record key -> node in game g's index; false when the index is full.  Wave-uniform; every lane must call.
__device__ bool index_insert(const tg_search_forest& f, int64_t g, uint64_t key, int node) {
  const int lane = lane_id();
  const uint64_t k = key ? key : kZeroKey;
  const int64_t cap = f.index_capacity;
  const uint64_t mask = static_cast<uint64_t>(cap - 1);
  uint64_t* tab = f.index_key + g * cap;
  for (int64_t base = 0; base < cap; base += 64) {
    const bool in = base + lane < cap;
    const uint64_t slot = (k + static_cast<uint64_t>(base + lane)) & mask;
    const uint64_t t = in ? tab[slot] : 1ull;
    const uint64_t free_or_same = __ballot(in && (t == 0 || t == k));
    if (free_or_same) {
      const int first = __builtin_ctzll(free_or_same);
      if (lane == first) {
        tab[slot] = k;
        f.index_node[g * cap + static_cast<int64_t>(slot)] = node;
      }
      return true;
    }
  }
  return false;
}

// ---- wave reductions ------------------------------------------------------------------------------------------

// a better than b under torch.argmax: NaN is the maximum, ties go to the lower index; index 64 = no candidate
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) {
  if (ai >= 64) return false;
  if (bi >= 64) return true;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && bn ? ai < bi : an;
  if (av != bv) return av > bv;
  return ai < bi;
}

// first index of the maximum of v over the lanes with `valid` (wave-uniform result; 64 if none)
__device__ int wave_argmax(float v, bool valid) {
  float bv = v;
  int bi = valid ? lane_id() : 64;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  return __builtin_amdgcn_readfirstlane(bi);
}

// wave total of a float whose values are integers below 2^24 (visit counts): exact in any order
__device__ __forceinline__ float wave_sum_counts(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// ---- frames ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ int byte_of(const uint4& q, int t) {
  const uint32_t w = t < 4 ? q.x : t < 8 ? q.y : t < 12 ? q.z : q.w;
  return sbyte(w, t & 3);
}

// The 3S <= 96 factor values of one action, token t - shift in lane t (lo) or lane t - 64 (hi)
struct Factors {
  int lo, hi;
};
__device__ __forceinline__ Factors load_factors(const int8_t* tok, int S, int shift) {
  const int lane = lane_id();
  return Factors{lane < 3 * S ? static_cast<int>(tok[lane]) - shift : 0,
                 lane + 64 < 3 * S ? static_cast<int>(tok[lane + 64]) - shift : 0};
}
// factor value t (every lane must call: cross-lane reads)
__device__ __forceinline__ int factor(const Factors& fv, int t) {
  const int a = __shfl(fv.lo, t & 63), b = __shfl(fv.hi, t & 63);
  return t < 64 ? a : b;
}

// Chunk c (16 bytes) of child head = parent head chunk p - u (x) v (x) w of the factors fv.
// Every lane of the wave must call (the factors are fetched with cross-lane reads); bytes at e >= N are zero.
// ovf |= an exact value left int8.
__device__ uint4 child_chunk(const uint4& p, int64_t c, int N, int S, const Factors& tokv, bool& ovf) {
  uint32_t w[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    int v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t e64 = 16 * c + 4 * m + t;
      const bool in = e64 < N;
      const int e = in ? static_cast<int>(e64) : N - 1;
      const int i = e / (S * S), r = e - i * S * S, j = r / S, l = r - j * S;
      const int u = factor(tokv, i), vv = factor(tokv, S + j), ww = factor(tokv, 2 * S + l);
      const int x = byte_of(p, 4 * m + t) - u * vv * ww;
      ovf |= in && (x < -128 || x > 127);
      v[t] = in ? x : 0;
    }
    w[m] = pack4(v[0], v[1], v[2], v[3]);
  }
  return uint4{w[0], w[1], w[2], w[3]};
}

// this chunk's share of the tg_hash_u64 sum (words 2c, 2c+1 where they exist)
__device__ __forceinline__ uint64_t hash_part(const uint4& q, int64_t c, int N) {
  const int64_t nword = (N + 7) / 8;
  const uint64_t w0 = static_cast<uint64_t>(q.x) | (static_cast<uint64_t>(q.y) << 32);
  const uint64_t w1 = static_cast<uint64_t>(q.z) | (static_cast<uint64_t>(q.w) << 32);
  uint64_t h = 0;
  if (2 * c < nword) h += fmix64(w0 + static_cast<uint64_t>(2 * c + 1) * 0x9E3779B97F4A7C15ull);
  if (2 * c + 1 < nword) h += fmix64(w1 + static_cast<uint64_t>(2 * c + 2) * 0x9E3779B97F4A7C15ull);
  return h;
}

__device__ __forceinline__ bool nonzero(const uint4& q) { return (q.x | q.y | q.z | q.w) != 0; }

template <typename OutT>
__device__ __forceinline__ OutT to_out(int x) {
  if constexpr (std::is_same<OutT, float>::value) return static_cast<float>(x);
  else if constexpr (std::is_same<OutT, __half>::value) return __int2half_rn(x);
  else return __float2bfloat16(static_cast<float>(x));
}

// model-input row: the 16 bytes of chunk c of frame fr, game g, into the dense (B,T,S,S,S) output
__device__ void emit_chunk(void* out, int dtype, int64_t g, int T, int fr, int64_t c, int N, const uint4& q) {
  const int64_t base = (g * T + fr) * N;
  for (int t = 0; t < 16; ++t) {
    const int64_t e = 16 * c + t;
    if (e >= N) break;
    const int x = byte_of(q, t);
    if (dtype == 0) static_cast<float*>(out)[base + e] = to_out<float>(x);
    else if (dtype == 1) static_cast<__half*>(out)[base + e] = to_out<__half>(x);
    else static_cast<__hip_bfloat16*>(out)[base + e] = to_out<__hip_bfloat16>(x);
  }
}

// dst frames = child (node frames `src`, token row `tok`): head - tensor(tok), then src frames 0..T-2.  Returns
// whether the new head has a non-zero byte (wave-uniform).  model_in (may be NULL) receives the frames of game g.
__device__ bool write_child_frames(const tg_search_forest& f, const int8_t* src, const int8_t* tok, int8_t* dst,
                                   void* model_in, int dtype, int64_t g, bool& ovf) {
  const int lane = lane_id();
  const int S = f.S, N = S * S * S, T = f.T;
  const int64_t FB = frame_bytes(S), NC = FB / 16;
  const Factors tokv = load_factors(tok, S, f.shift);
  bool nz = false;
  for (int64_t base = 0; base < NC; base += 64) {  // wave-uniform loop: child_chunk reads across lanes
    const int64_t c = base + lane;
    const bool in = c < NC;
    const uint4 p = in ? *reinterpret_cast<const uint4*>(src + 16 * c) : uint4{0, 0, 0, 0};
    const uint4 q = child_chunk(p, in ? c : 0, N, S, tokv, ovf);
    if (in) {
      *reinterpret_cast<uint4*>(dst + 16 * c) = q;
      nz |= nonzero(q);
      if (model_in) emit_chunk(model_in, dtype, g, T, 0, c, N, q);
    }
  }
  for (int fr = 1; fr < T; ++fr)
    for (int64_t c = lane; c < NC; c += 64) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + (fr - 1) * FB + 16 * c);
      *reinterpret_cast<uint4*>(dst + fr * FB + 16 * c) = q;
      if (model_in) emit_chunk(model_in, dtype, g, T, fr, c, N, q);
    }
  return __ballot(nz) != 0;
}

// dst frames = src frames (T x FB); returns whether frame 0 has a non-zero byte
__device__ bool copy_frames(const tg_search_forest& f, const int8_t* src, int8_t* dst, void* model_in, int dtype,
                            int64_t g) {
  const int lane = lane_id();
  const int S = f.S, N = S * S * S, T = f.T;
  const int64_t FB = frame_bytes(S), NC = FB / 16;
  bool nz = false;
  for (int fr = 0; fr < T; ++fr)
    for (int64_t c = lane; c < NC; c += 64) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + fr * FB + 16 * c);
      *reinterpret_cast<uint4*>(dst + fr * FB + 16 * c) = q;
      if (fr == 0) nz |= nonzero(q);
      if (model_in) emit_chunk(model_in, dtype, g, T, fr, c, N, q);
    }
  return __ballot(nz) != 0;
}

// ---- kernels --------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void reset_kernel(tg_search_forest f, const int8_t* states, int n_sim) {
  const int lane = lane_id();
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (g >= f.B) return;
  const int S = f.S, N = S * S * S, T = f.T;
  const int64_t FB = frame_bytes(S), NC = FB / 16;
  int8_t* rf = f.root_frames + g * T * FB;
  uint64_t h = 0;
  bool nz = false;
  for (int fr = 0; fr < T; ++fr) {
    const int8_t* src = states + (g * T + fr) * N;
    for (int64_t c = lane; c < NC; c += 64) {
      int v[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) v[t] = 16 * c + t < N ? src[16 * c + t] : 0;
      const uint4 q{pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]), pack4(v[8], v[9], v[10], v[11]),
                    pack4(v[12], v[13], v[14], v[15])};
      *reinterpret_cast<uint4*>(rf + fr * FB + 16 * c) = q;
      if (fr == 0) {
        h += hash_part(q, c, N);
        nz |= nonzero(q);
      }
    }
  }
  h = wave_sum_u64(h);
  const bool zero = __ballot(nz) == 0;
  for (int64_t i = lane; i < f.index_capacity; i += 64) f.index_key[g * f.index_capacity + i] = 0;
  for (int m = lane; m < f.max_actions; m += 64) {
    f.traj_node[g * f.max_actions + m] = -1;
    f.traj_choice[g * f.max_actions + m] = -1;
  }
  if (lane == 0) {
    f.root_key[g] = hash_finish(h, N);
    f.node_count[g] = 0;
    f.move[g] = 0;
    f.done[g] = zero ? 1 : 0;
    f.sims_left[g] = zero ? 0 : n_sim;
    f.status[g] = 0;
    f.overflow[g] = 0;
    f.flags[g] = 0;
    f.attempt[g] = 0;
    f.depth[g] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void select_kernel(tg_search_forest f, void* model_in, int dtype, float* scalars) {
  const int lane = lane_id();
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (g >= f.B) return;
  if (f.done[g] || f.sims_left[g] <= 0) {
    if (lane == 0) f.flags[g] = 0;
    return;
  }
  const int S = f.S, T = f.T, k = f.k;
  const int64_t FB = frame_bytes(S);
  const int64_t gM = g * f.M;
  uint64_t key = f.root_key[g];
  int depth = 0, last_node = -1, last_slot = -1;
  for (;;) {
    const int node = index_lookup(f, g, key);
    if (node < 0) break;
    if (depth >= f.max_depth) {  // DEVIATION 2: the reference descends forever
      if (lane == 0) {
        f.status[g] |= 2u;
        f.sims_left[g] -= 1;
        f.flags[g] = 0;
        f.depth[g] = depth;
      }
      return;
    }
    const int64_t nb = (gM + node) * k;
    const int nc = f.node_nchild[gM + node];
    if (nc < 1 || nc > k) {  // never written by commit; guards the reads below against a corrupted forest
      if (lane == 0) {
        f.status[g] |= 1u;
        f.sims_left[g] -= 1;
        f.flags[g] = 0;
      }
      return;
    }
    const bool valid = lane < nc;
    const float q = valid ? f.child_q[nb + lane] : 0.f;
    float score = q;
    if (f.child_prior) {  // PUCT (select_next_state with a prior): wave-uniform branch
      const float n = valid ? f.child_n[nb + lane] : 0.f;
      const float sum = wave_sum_counts(n);
      const float c_explore = 1.25f + logf((sum + 19652.0f + 1.0f) / 19652.0f);
      const float pr = valid ? f.child_prior[nb + lane] : 0.f;
      score = q + c_explore * pr * sqrtf(sum) / (1.0f + n);
    }
    const int j = wave_argmax(score, valid);
    if (lane == 0) {
      f.path_node[g * f.max_depth + depth] = node;
      f.path_slot[g * f.max_depth + depth] = j;
    }
    key = f.child_key[nb + j];
    last_node = node;
    last_slot = j;
    ++depth;
  }
  const int m = f.move[g];
  const int idx = m + depth;
  const int bound = min(f.max_actions, m + f.horizon);
  int8_t* lf = f.leaf_frames + g * T * FB;
  bool head_nz, ovf = false;
  if (depth == 0) {
    head_nz = copy_frames(f, f.root_frames + g * T * FB, lf, model_in, dtype, g);
  } else {
    const int64_t row = (gM + last_node) * k + last_slot;
    head_nz = write_child_frames(f, f.node_frames + (gM + last_node) * T * FB, f.child_tokens + row * 3 * S, lf,
                                 model_in, dtype, g, ovf);
  }
  const uint32_t fl = TG_SEARCH_PENDING | (idx <= bound ? (head_nz ? TG_SEARCH_EXPAND : TG_SEARCH_TERMINAL) : TG_SEARCH_HORIZON);
  if (lane == 0) {
    f.leaf_key[g] = key;
    f.depth[g] = depth;
    f.attempt[g] = 0;
    f.flags[g] = static_cast<uint8_t>(fl);
    if (scalars) scalars[g] = static_cast<float>(idx);
  }
}

// N*Q rounded on its own: one v_mul_f32 the compiler cannot fuse with the following add (the __fmul_rn / __fadd_rn
// wrappers are plain operators in this toolchain, and hipcc contracted them into a v_fma_f32 -- one ulp off torch)
__device__ __forceinline__ float mul_rounded(float a, float b) {
  float r;
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// Q/N along the path, leaf to root (backward_pass, act.py:219-237): the float32 operations of torch in its order,
// each rounded on its own (no contraction into an FMA; '/' is the correctly rounded division)
__device__ void backup(const tg_search_forest& f, int64_t g, int depth, float reward) {
#pragma clang fp contract(off)
  for (int d = depth - 1; d >= 0; --d) {
    reward = reward - 1.0f;
    const int node = f.path_node[g * f.max_depth + d], slot = f.path_slot[g * f.max_depth + d];
    const int64_t at = (g * f.M + node) * f.k + slot;
    const float n = f.child_n[at], q = f.child_q[at];
    f.child_q[at] = (mul_rounded(n, q) + reward) / (n + 1.0f);
    f.child_n[at] = n + 1.0f;
  }
}

__global__ __launch_bounds__(kBlock) void commit_kernel(tg_search_forest f, const int8_t* tokens, const float* leaf_q,
                                                        const float* prior, const uint8_t* mask) {
  const int lane = lane_id();
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (g >= f.B) return;
  const uint32_t fl = f.flags[g];
  if (!(fl & TG_SEARCH_PENDING) || (mask && !mask[g])) return;
  const int depth = f.depth[g];
  const uint32_t kind = fl & (TG_SEARCH_EXPAND | TG_SEARCH_TERMINAL | TG_SEARCH_HORIZON);
  float reward = 0.0f;  // DEVIATION 1 for TERMINAL; no leaf term past the horizon (the reference's too)
  if (fl & TG_SEARCH_EXPAND) {
    const int S = f.S, N = S * S * S, T = f.T, k = f.k;
    const int64_t FB = frame_bytes(S), NC = FB / 16;
    const int8_t* lf = f.leaf_frames + g * T * FB;
    const int8_t* tk = tokens + g * k * 3 * S;
    uint64_t my_key = 0;
    bool my_changed = false, ovf = false;
    for (int j = 0; j < k; ++j) {  // child j: chunk-parallel over the wave, key and "changed" reduced into lane j
      const Factors tokv = load_factors(tk + j * 3 * S, S, f.shift);
      uint64_t h = 0;
      bool chg = false;
      for (int64_t base = 0; base < NC; base += 64) {
        const int64_t c = base + lane;
        const bool in = c < NC;
        const uint4 p = in ? *reinterpret_cast<const uint4*>(lf + 16 * c) : uint4{0, 0, 0, 0};
        const uint4 q = child_chunk(p, in ? c : 0, N, S, tokv, ovf);
        if (in) {
          h += hash_part(q, c, N);
          chg |= (q.x != p.x) | (q.y != p.y) | (q.z != p.z) | (q.w != p.w);
        }
      }
      h = wave_sum_u64(h);
      const bool changed = __ballot(chg) != 0;
      if (lane == j) {
        my_key = hash_finish(h, N);
        my_changed = changed;
      }
    }
    if (__ballot(ovf) && lane == 0) f.overflow[g] = 1;
    // remove_null_actions, then `c not in new_mc_tree` against the tree as it is before this expansion
    const bool fresh = lane < k && my_changed && !index_contains_lane(f, g, my_key);
    const uint64_t surv = __ballot(fresh);
    if (surv == 0) {  // the reference asks the model again for the same leaf
      if (lane == 0) {
        f.flags[g] = static_cast<uint8_t>(fl | TG_SEARCH_RETRY);
        f.attempt[g] += 1;
      }
      return;
    }
    const int nid = f.node_count[g];
    const bool ok = nid < f.M && index_insert(f, g, f.leaf_key[g], nid);
    if (!ok) {  // pool or index full: the expansion and the backup are dropped
      if (lane == 0) {
        f.status[g] |= 1u;
        f.flags[g] = static_cast<uint8_t>(kind);
        f.sims_left[g] -= 1;
      }
      return;
    }
    const int64_t node = g * f.M + nid;
    const int64_t nb = node * k;
    for (int fr = 0; fr < T; ++fr)
      for (int64_t c = lane; c < NC; c += 64)
        *reinterpret_cast<uint4*>(f.node_frames + node * T * FB + fr * FB + 16 * c) =
            *reinterpret_cast<const uint4*>(lf + fr * FB + 16 * c);
    if (fresh) {
      const int pos = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(surv >> 32),
                                                __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(surv), 0u));
      f.child_key[nb + pos] = my_key;
      f.child_n[nb + pos] = 0.0f;
      f.child_q[nb + pos] = 0.0f;
      if (f.child_prior) f.child_prior[nb + pos] = prior ? prior[g * k + lane] : 0.0f;
      int8_t* dst = f.child_tokens + (nb + pos) * 3 * S;
      const int8_t* src = tk + lane * 3 * S;
      for (int s = 0; s < 3 * S; ++s) dst[s] = src[s];
    }
    if (lane == 0) {
      f.node_key[node] = f.leaf_key[g];
      f.node_nchild[node] = __popcll(surv);
      f.node_count[g] = nid + 1;
    }
    reward = 0.0f + leaf_q[g];  // reward = 0; reward += leaf_q_val
  }
  if (lane == 0) {
    backup(f, g, depth, reward);
    f.flags[g] = static_cast<uint8_t>(kind);
    f.sims_left[g] -= 1;
  }
}

__global__ __launch_bounds__(kBlock) void advance_kernel(tg_search_forest f, int n_sim) {
  const int lane = lane_id();
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (g >= f.B) return;
  if (f.done[g]) return;
  const int S = f.S, T = f.T, k = f.k;
  const int64_t FB = frame_bytes(S), NC = FB / 16;
  const int m = f.move[g];
  const int node = index_lookup(f, g, f.root_key[g]);
  if (node < 0) {  // the root's expansion was dropped (status bit 0 already set): the game ends here
    if (lane == 0) {
      f.status[g] |= 1u;
      f.done[g] = 1;
      f.sims_left[g] = 0;
    }
    return;
  }
  int8_t* rf = f.root_frames + g * T * FB;
  int8_t* tr = f.traj_frames + (g * f.max_actions + m) * T * FB;
  for (int fr = 0; fr < T; ++fr)
    for (int64_t c = lane; c < NC; c += 64)
      *reinterpret_cast<uint4*>(tr + fr * FB + 16 * c) = *reinterpret_cast<const uint4*>(rf + fr * FB + 16 * c);
  const int64_t gM = g * f.M;
  const int64_t nb = (gM + node) * k;
  const int nc = f.node_nchild[gM + node];
  if (nc < 1 || nc > k) {  // (as in select)
    if (lane == 0) {
      f.status[g] |= 1u;
      f.done[g] = 1;
      f.sims_left[g] = 0;
    }
    return;
  }
  const int j = wave_argmax(lane < nc ? f.child_q[nb + lane] : 0.f, lane < nc);
  bool ovf = false;
  // (each lane rewrites exactly the root chunks it copied above: same lane mapping, program order)
  const bool nz = write_child_frames(f, f.node_frames + (gM + node) * T * FB, f.child_tokens + (nb + j) * 3 * S, rf,
                                     nullptr, 0, g, ovf);
  const uint64_t key = f.child_key[nb + j];
  const int m1 = m + 1;
  const bool dn = !nz || m1 >= f.max_actions;
  int left = 0;
  if (!dn) {
    const int nn = index_lookup(f, g, key);
    float visits = 0.f;
    if (nn >= 0) {
      const int64_t b2 = (gM + nn) * k;
      const int c2 = min(f.node_nchild[gM + nn], k);
      visits = wave_sum_counts(lane < c2 ? f.child_n[b2 + lane] : 0.f);
    }
    left = max(n_sim - static_cast<int>(visits), 0);
  }
  if (lane == 0) {
    f.traj_node[g * f.max_actions + m] = node;
    f.traj_choice[g * f.max_actions + m] = j;
    f.root_key[g] = key;
    f.move[g] = m1;
    f.done[g] = dn ? 1 : 0;
    f.sims_left[g] = left;
  }
}

__global__ __launch_bounds__(kBlock) void policy_kernel(tg_search_forest f, float* policy, int n_logits, int n_bar) {
  const int lane = lane_id();
  const int64_t gm = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (gm >= f.B * f.max_actions) return;
  const int64_t g = gm / f.max_actions;
  const int m = static_cast<int>(gm - g * f.max_actions);
  const int S = f.S, k = f.k, steps = 3 * S;
  float* out = policy + gm * steps * n_logits;
  const int node = m < f.move[g] ? f.traj_node[gm] : -1;
  const int64_t nb = (g * f.M + (node < 0 ? 0 : node)) * k;
  const int nc = node < 0 ? 0 : min(max(f.node_nchild[g * f.M + node], 0), k);
  float p = 0.f;
  if (node >= 0) {
    const float n = lane < nc ? f.child_n[nb + lane] : 0.f;
    const float sum = wave_sum_counts(n);
    float pw = n;
    if (sum > static_cast<float>(n_bar)) {
      // tau = (sum.log() / n_bar.log()).item() in float32; visit_count ** (1 / tau) with the exponent as float.  The
      // logarithms and the power are evaluated in double and rounded once (the host's logf/powf are within half an
      // ulp of that nearly always; the exponent's rounding matches torch's)
      const float tau = static_cast<float>(log(static_cast<double>(sum))) / static_cast<float>(log(static_cast<double>(n_bar)));
      const float e = static_cast<float>(1.0 / static_cast<double>(tau));
      pw = e == 0.5f ? sqrtf(n) : static_cast<float>(pow(static_cast<double>(n), static_cast<double>(e)));
    }
    p = pw / sum;
  }
  bool bad = false;
  for (int base = 0; base < steps; base += 64) {  // wave-uniform: the samples' p are broadcast by cross-lane reads
    const int s = base + lane;
    const bool in = s < steps;
    if (in)
      for (int t = 0; t < n_logits; ++t) out[s * n_logits + t] = 0.f;
    for (int j = 0; j < nc; ++j) {  // samples in order, each row owned by one lane
      const float pj = __shfl(p, j);
      if (in) {
        const int tok = f.child_tokens[(nb + j) * steps + s];
        if (tok < 0 || tok >= n_logits) bad = true;
        else out[s * n_logits + tok] += pj;
      }
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(f.status + g, 4u);
}

}  // namespace search
}  // namespace tg

namespace {

int check_forest(const char* fn, const tg_search_forest* f) {
  if (!f) return tg_internal_fail(TG_ERR_INVALID, "%s: null forest", fn);
  if (f->B < 0 || f->S < 1 || f->S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: bad B=%lld or S=%d", fn, (long long)f->B, f->S);
  if (f->T < 1 || f->T > TG_SEARCH_MAX_T) return tg_internal_fail(TG_ERR_INVALID, "%s: T=%d outside 1..%d", fn, f->T, TG_SEARCH_MAX_T);
  if (f->k < 1 || f->k > TG_SEARCH_MAX_K) return tg_internal_fail(TG_ERR_INVALID, "%s: k=%d outside 1..%d", fn, f->k, TG_SEARCH_MAX_K);
  if (f->M < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: M=%d < 1", fn, f->M);
  if (f->index_capacity < 2 || (f->index_capacity & (f->index_capacity - 1)))
    return tg_internal_fail(TG_ERR_INVALID, "%s: index_capacity=%lld must be a power of two >= 2", fn, (long long)f->index_capacity);
  if (f->max_actions < 1 || f->max_actions > TG_SEARCH_MAX_ACTIONS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: max_actions=%d outside 1..%d", fn, f->max_actions, TG_SEARCH_MAX_ACTIONS);
  if (f->horizon < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: horizon=%d < 0", fn, f->horizon);
  if (f->max_depth < 1 || f->max_depth > TG_SEARCH_MAX_DEPTH)
    return tg_internal_fail(TG_ERR_INVALID, "%s: max_depth=%d outside 1..%d", fn, f->max_depth, TG_SEARCH_MAX_DEPTH);
  const void* need[] = {f->node_key, f->node_frames, f->node_nchild, f->child_tokens, f->child_key, f->child_n, f->child_q,
                        f->index_key, f->index_node, f->node_count, f->root_frames, f->root_key, f->move, f->done,
                        f->sims_left, f->status, f->overflow, f->leaf_frames, f->leaf_key, f->path_node, f->path_slot,
                        f->depth, f->flags, f->attempt, f->traj_frames, f->traj_node, f->traj_choice};
  for (const void* p : need)
    if (!p) return tg_internal_fail(TG_ERR_INVALID, "%s: null forest array", fn);
  if (!aligned(f->node_frames, 16) || !aligned(f->root_frames, 16) || !aligned(f->leaf_frames, 16) ||
      !aligned(f->traj_frames, 16))
    return tg_internal_fail(TG_ERR_INVALID, "%s: frame arrays must be 16-byte aligned", fn);
  if (!aligned(f->node_key, 8) || !aligned(f->child_key, 8) || !aligned(f->index_key, 8) || !aligned(f->root_key, 8) ||
      !aligned(f->leaf_key, 8))
    return tg_internal_fail(TG_ERR_INVALID, "%s: key arrays must be 8-byte aligned", fn);
  return TG_OK;
}

// one wavefront per game (or per (game, move) for the policy)
template <typename K, typename... A>
int launch_games(const char* fn, K kernel, int64_t n, tg_stream_t stream, const A&... args) {
  return launch(fn, kernel, static_cast<unsigned>((n + tg::search::kWaves - 1) / tg::search::kWaves), tg::kBlock, 0,
                static_cast<hipStream_t>(stream), args...);
}

}  // namespace

extern "C" {

int tg_search_reset(const tg_search_forest* f, const int8_t* states, int n_sim, tg_stream_t stream) {
  const char* fn = "tg_search_reset";
  if (int rc = check_forest(fn, f)) return rc;
  if (n_sim < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: n_sim=%d < 0", fn, n_sim);
  if (f->B == 0) return TG_OK;
  if (!states) return tg_internal_fail(TG_ERR_INVALID, "%s: null states", fn);
  return launch_games(fn, tg::search::reset_kernel, f->B, stream, *f, states, n_sim);
}

int tg_search_select(const tg_search_forest* f, void* model_in, int out_dtype, float* scalars, tg_stream_t stream) {
  const char* fn = "tg_search_select";
  if (int rc = check_forest(fn, f)) return rc;
  if (model_in && (out_dtype < 0 || out_dtype > 2))
    return tg_internal_fail(TG_ERR_INVALID, "%s: out_dtype must be 0 (f32), 1 (f16) or 2 (bf16)", fn);
  if (f->B == 0) return TG_OK;
  return launch_games(fn, tg::search::select_kernel, f->B, stream, *f, model_in, out_dtype, scalars);
}

int tg_search_commit(const tg_search_forest* f, const int8_t* tokens, const float* leaf_q, const float* prior,
                     const uint8_t* mask, tg_stream_t stream) {
  const char* fn = "tg_search_commit";
  if (int rc = check_forest(fn, f)) return rc;
  if (f->B == 0) return TG_OK;
  if (!tokens || !leaf_q) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens or leaf_q", fn);
  return launch_games(fn, tg::search::commit_kernel, f->B, stream, *f, tokens, leaf_q, prior, mask);
}

int tg_search_advance(const tg_search_forest* f, int n_sim, tg_stream_t stream) {
  const char* fn = "tg_search_advance";
  if (int rc = check_forest(fn, f)) return rc;
  if (n_sim < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: n_sim=%d < 0", fn, n_sim);
  if (f->B == 0) return TG_OK;
  return launch_games(fn, tg::search::advance_kernel, f->B, stream, *f, n_sim);
}

int tg_search_policy(const tg_search_forest* f, float* policy, int n_logits, int n_bar, tg_stream_t stream) {
  const char* fn = "tg_search_policy";
  if (int rc = check_forest(fn, f)) return rc;
  if (n_logits < 1 || n_logits > 256) return tg_internal_fail(TG_ERR_INVALID, "%s: n_logits=%d outside 1..256", fn, n_logits);
  if (n_bar < 1) return tg_internal_fail(TG_ERR_INVALID, "%s: n_bar=%d < 1", fn, n_bar);
  if (f->B == 0) return TG_OK;
  if (!policy) return tg_internal_fail(TG_ERR_INVALID, "%s: null policy", fn);
  return launch_games(fn, tg::search::policy_kernel, f->B * f->max_actions, stream, *f, policy, n_logits, n_bar);
}

}  // extern "C"
