// tg_items.h -- the item gatherers shared by tg_items.hip (tg_demo_items) and tg_replay.hip (tg_replay_items): the
// three per-size item bodies, templated over a row-resolution policy (Rows), and the host-side kernel choice.
//
// Per item: frame 0 = target[d] - sum_{j > k} tensor(a_j) (the suffix replay, summed exactly, no intermediate narrowing),
// frames 1..m = tensor(a_j), j = k+m .. k+1, the rest zero; scalar, action and reward beside them.  Three bodies:
//   - S = 4 (items_s4_body): 16 lanes per item, one (i,j) row of 4 entries per lane, the suffix summed on the VALU
//     straight from the tokens (R = 7 at BASELINE scale: 6 rows); each lane stores its 4 entries of every frame (one
//     16-byte store for float32);
//   - S = 16, 25 with R <= 256 (items_mfma_body): frame 0 is a masked dense contraction, the generator's
//     (tg_mfma.h): the item's K = R-1-k suffix rows are staged transposed into LDS, compacted to rows 0..K-1 and
//     zero-filled up to Kp = roundup32(K), and the column tiles of tg_mfma_tiles.h run v_mfma_i32_32x32x32_i8 over Kp.
//     The epilogue subtracts the int32 sums from the item's target bytes (staged in an LDS image) before the range
//     check and the narrowing.  An item whose factors break |u|, |v| <= 11 (or w outside int8) takes the exact VALU
//     form below instead (demos in a random GL(S,Z) basis).  Several items per workgroup;
//   - every other S or R (items_exact_body): the exact VALU form, int64 sums, one item per workgroup at a time.
// Frames leave in the output dtype through 16-byte stores wherever the frame's address allows (write_frame).
// Every __global__ kernel is a thin wrapper that declares the LDS and calls one body with its policy (tg_items.hip:
// DemoRows; tg_replay.hip: the played / best rows of a mixed batch), so the bodies are compiled once per policy and the
// kernel code of tg_demo_items does not depend on the other policies.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_demos.h"
#include "tg_device.h"
#include "tg_emit.h"
#include "tg_host.h"

namespace tg {

#include "tg_mfma_tiles.h"

struct ItemArgs {
  const int8_t* tokens;   // (n_demos, R, 3S)
  const int8_t* targets;  // demo d at targets + d * tstride
  int64_t n_demos, tstride;
  const int64_t* idx;     // (N) flat indices
  int64_t N;
  void* frames;           // (N, T, S, S, S) of OutT
  float* scalars;
  int8_t* actions;
  float* rewards;
  uint8_t* overflow;
  uint32_t* status;
  int R, S, T, shift;
  int RS;                 // items_mfma_kernel: bytes per row of the transposed factors
  int vec;                // frames 16-byte aligned (items_s4_kernel) / targets 16-byte aligned (items_mfma_kernel)
};

struct Item {
  int64_t d;
  int k;
  bool valid;
};

__device__ __forceinline__ Item decode_item(const ItemArgs& a, int64_t n) {
  const int64_t x = a.idx[n];
  Item it;
  it.valid = x >= 0 && x < a.n_demos * a.R;  // (n_demos * R < 2^63: checked on the host)
  it.d = it.valid ? x / a.R : 0;
  it.k = it.valid ? static_cast<int>(x - it.d * a.R) : 0;
  return it;
}

// scalar, reward, action of item n (zeros for a bad index, which also sets bit 0 of *status)
__device__ __forceinline__ void write_meta(const ItemArgs& a, int64_t n, const Item& it, int t, int nthr) {
  if (t == 0) {
    if (a.scalars) a.scalars[n] = it.valid ? static_cast<float>(a.R - it.k) : 0.f;
    if (a.rewards) a.rewards[n] = it.valid ? static_cast<float>(-(it.k + 1)) : 0.f;
    if (!it.valid && a.status) atomicOr(a.status, 1u);
  }
  if (a.actions) {
    const int A3 = 3 * a.S;
    if (it.valid) {
      const int8_t* src = a.tokens + (it.d * a.R + it.k) * A3;
      for (int x = t; x < A3; x += nthr) a.actions[n * A3 + x] = src[x];
    } else {
      for (int x = t; x < A3; x += nthr) a.actions[n * A3 + x] = 0;
    }
  }
}

template <typename OutT>
__device__ __forceinline__ void store1(OutT* p, int v) {
  int y[16 / sizeof(OutT)] = {v};
  emit_store_one(p, emit_pack<OutT>(y), 0);
}

// One frame of N3 entries at dst (aligned to sizeof(OutT)), entry e = get(e) (an int8 value): the entries before the
// first 16-byte boundary and after the last one one by one, everything between as 16-byte stores.
template <typename OutT, typename F>
__device__ __forceinline__ void write_frame(OutT* dst, int N3, int t, int nthr, F get) {
  constexpr int PER = 16 / sizeof(OutT);
  int head = static_cast<int>(((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(OutT));
  head = head < N3 ? head : N3;
  const int nbody = (N3 - head) / PER;
  for (int e = t; e < head; e += nthr) store1(dst + e, get(e));
  OutT* body = dst + head;
  for (int c = t; c < nbody; c += nthr) {
    int x[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) x[q] = get(head + c * PER + q);
    *reinterpret_cast<uint4*>(body + c * PER) = emit_pack<OutT>(x);
  }
  for (int e = head + nbody * PER + t; e < N3; e += nthr) store1(dst + e, get(e));
}

// frames 1..T-1 of an item (workgroup-wide): tensor(a_{k+m+1-f}) for f <= m, zero after.  rk: 3S ints of LDS.
template <int S_, typename OutT>
__device__ __forceinline__ void write_action_frames(const ItemArgs& a, OutT* out, const Item& it, int t, int* rk,
                                                    int& ov) {
  const int S = S_ ? S_ : a.S, S2 = S * S, N3 = S2 * S, A3 = 3 * S;
  const int m = it.valid ? min(a.T - 1, a.R - 1 - it.k) : 0;
  for (int f = 1; f < a.T; ++f) {
    OutT* dst = out + static_cast<int64_t>(f) * N3;
    if (f > m) {
      write_frame(dst, N3, t, kBlock, [](int) { return 0; });
      continue;
    }
    __syncthreads();  // the previous frame's readers of rk are done
    if (t < A3) rk[t] = a.tokens[(it.d * a.R + it.k + m + 1 - f) * A3 + t] - a.shift;
    __syncthreads();
    write_frame(dst, N3, t, kBlock, [&](int e) {
      const int i = e / S2, r = e - i * S2, j = r / S, l = r - j * S;
      const int64_t v = static_cast<int64_t>(rk[i]) * rk[S + j] * rk[2 * S + l];
      ov |= v < -128 || v > 127;
      return static_cast<int>(static_cast<int8_t>(v));
    });
  }
}

// Frame 0 in exact arithmetic on the VALU (workgroup-wide): img holds the item's target bytes and receives the int8 of
// target - sum over the K suffix rows (int64 sums of int64 products: exact for any token and shift).  The rows pass
// through LDS (fac) kRch at a time; every thread keeps EPT entries in registers per pass over the frame.  Thread t
// reads and writes only the entries e = t mod kBlock of img.
constexpr int kRch = 32;
template <int S_>
__device__ void exact_frame0(const int8_t* suffix, int K, int S, int shift, uint8_t* img, int* fac, int t, int& ov) {
  constexpr int EPT = 8;
  if (S_) S = S_;
  const int S2 = S * S, N3 = S2 * S, A3 = 3 * S;
  for (int e0 = 0; e0 < N3; e0 += EPT * kBlock) {
    int64_t acc[EPT];
    int fi[EPT], fj[EPT], fl[EPT];
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = e0 + t + q * kBlock, ee = e < N3 ? e : 0;
      const int i = ee / S2, r = ee - i * S2, j = r / S;
      fi[q] = i;
      fj[q] = S + j;
      fl[q] = 2 * S + r - j * S;
      acc[q] = 0;
    }
    for (int r0 = 0; r0 < K; r0 += kRch) {
      const int nr = min(kRch, K - r0);
      __syncthreads();  // the previous rows are consumed
      for (int q = t; q < nr * A3; q += kBlock) fac[q] = suffix[static_cast<int64_t>(r0) * A3 + q] - shift;
      __syncthreads();
      for (int r = 0; r < nr; ++r) {
        const int* f = fac + r * A3;
#pragma unroll
        for (int q = 0; q < EPT; ++q) acc[q] += static_cast<int64_t>(f[fi[q]]) * f[fj[q]] * f[fl[q]];
      }
    }
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int e = e0 + t + q * kBlock;
      if (e < N3) {
        const int64_t v = static_cast<int64_t>(static_cast<int8_t>(img[e])) - acc[q];
        ov |= v < -128 || v > 127;
        img[e] = static_cast<uint8_t>(v);
      }
    }
  }
}

__device__ __forceinline__ void set_overflow(const ItemArgs& a, int64_t n, int ov, int t) {
  if (__syncthreads_or(ov) && t == 0 && a.overflow) a.overflow[n] = 1;  // (also the end-of-item barrier)
}

// ---- row resolution policies ---------------------------------------------------------------------------------------
// A body below asks its Rows policy what item n is.  DemoRows: a synthetic item at the flat index idx[n] (tg_demo_items);
// kMixed = false compiles the question away, so the tg_demo_items kernels are the code they were before the policies.
// Every policy provides Item item(a, n), the synthetic item (valid or not) that row n is when it is not a stored move.
// A kMixed policy (tg_replay.hip) also provides bool write_stored(a, n, OutT* out, int t, int nthr): when row n is a
// stored move it writes the whole row itself (threads t of nthr, no barrier, no LDS) and returns true.  The branch is
// uniform over the threads that serve one item (a workgroup, or 16 lanes at S = 4).
struct DemoRows {
  static constexpr bool kMixed = false;
};

template <typename Rows>
__device__ __forceinline__ Item row_item(const ItemArgs& a, const Rows& rows, int64_t n) {
  if constexpr (Rows::kMixed) return rows.item(a, n);
  else return decode_item(a, n);
}

// ---- any S, any R: exact VALU form, one item per workgroup at a time --------------------------------------------
template <typename Rows, typename OutT, typename... X>
__global__ __launch_bounds__(kBlock) void items_exact_kernel(ItemArgs a, X... x) {
  extern __shared__ __attribute__((aligned(16))) uint8_t img[];  // S^3 bytes
  __shared__ int fac[kRch * 3 * TG_MAX_S];
  __shared__ int rk[3 * TG_MAX_S];
  const Rows rows{x...};
  const int t = threadIdx.x, S = a.S, N3 = S * S * S, A3 = 3 * S;
  for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
    if constexpr (Rows::kMixed) {
      if (rows.write_stored(a, n, static_cast<OutT*>(a.frames) + n * a.T * N3, t, kBlock)) continue;
    }
    const Item it = row_item(a, rows, n);
    OutT* out = static_cast<OutT*>(a.frames) + n * a.T * N3;
    write_meta(a, n, it, t, kBlock);
    int ov = 0;
    if (it.valid) {
      const int8_t* tgt = a.targets + it.d * a.tstride;
      for (int e = t; e < N3; e += kBlock) img[e] = static_cast<uint8_t>(tgt[e]);
      exact_frame0<0>(a.tokens + (it.d * a.R + it.k + 1) * A3, a.R - 1 - it.k, S, a.shift, img, fac, t, ov);
      __syncthreads();
      write_frame(out, N3, t, kBlock, [&](int e) { return static_cast<int>(static_cast<int8_t>(img[e])); });
    } else {
      write_frame(out, N3, t, kBlock, [](int) { return 0; });
    }
    write_action_frames<0>(a, out, it, t, rk, ov);
    set_overflow(a, n, ov, t);
  }
}

// ---- S = 4: 16 lanes per item, lane g owns the row (i, j) = (g / 4, g % 4): entries 4g .. 4g+3 of every frame -------
// Acc = int32 when (R-1) * max|factor|^3 + 128 < 2^31 (the host decides), int64 otherwise.
template <typename OutT>
__device__ __forceinline__ void store4(OutT* p, const int (&x)[4], bool vec) {
  int y[16 / sizeof(OutT)];
#pragma unroll
  for (int q = 0; q < static_cast<int>(16 / sizeof(OutT)); ++q) y[q] = q < 4 ? x[q] : 0;
  const uint4 o = emit_pack<OutT>(y);
  if (vec) {
    if constexpr (sizeof(OutT) == 4) *reinterpret_cast<uint4*>(p) = o;
    else if constexpr (sizeof(OutT) == 2) *reinterpret_cast<uint2*>(p) = uint2{o.x, o.y};
    else *reinterpret_cast<uint32_t*>(p) = o.x;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) emit_store_one(p + q, o, q);
  }
}

template <typename Rows, typename OutT, typename Acc, typename... X>
__global__ __launch_bounds__(kBlock) void items_s4_kernel(ItemArgs a, X... x) {
  const Rows rows{x...};
  constexpr int IPB = kBlock / 16;  // items per workgroup and pass
  const int g = threadIdx.x & 15, i = g >> 2, j = g & 3;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * IPB + (threadIdx.x >> 4); n < a.N;
       n += static_cast<int64_t>(gridDim.x) * IPB) {
    if constexpr (Rows::kMixed) {
      if (rows.write_stored(a, n, static_cast<OutT*>(a.frames) + n * a.T * 64, g, 16)) continue;  // uniform over the item's 16 lanes
    }
    const Item it = row_item(a, rows, n);
    write_meta(a, n, it, g, 16);
    OutT* out = static_cast<OutT*>(a.frames) + n * a.T * 64 + 4 * g;
    const int8_t* tk = a.tokens + it.d * a.R * 12;
    int x[4] = {0, 0, 0, 0}, ov = 0, m = 0;
    if (it.valid) {
      const int8_t* tgt = a.targets + it.d * a.tstride + 4 * g;
      Acc acc[4] = {0, 0, 0, 0};
      for (int r = it.k + 1; r < a.R; ++r) {
        const int8_t* row = tk + r * 12;
        const Acc p = static_cast<Acc>(row[i] - a.shift) * (row[4 + j] - a.shift);
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[l] += p * (row[8 + l] - a.shift);
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const Acc v = static_cast<Acc>(tgt[l]) - acc[l];
        ov |= v < -128 || v > 127;
        x[l] = static_cast<int8_t>(v);
      }
      m = min(a.T - 1, a.R - 1 - it.k);
    }
    store4(out, x, a.vec);
    for (int f = 1; f < a.T; ++f) {
      int y[4] = {0, 0, 0, 0};
      if (f <= m) {
        const int8_t* row = tk + (it.k + m + 1 - f) * 12;
        const int64_t p = static_cast<int64_t>(row[i] - a.shift) * (row[4 + j] - a.shift);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const int64_t v = p * (row[8 + l] - a.shift);
          ov |= v < -128 || v > 127;
          y[l] = static_cast<int8_t>(v);
        }
      }
      store4(out + static_cast<int64_t>(f) * 64, y, a.vec);
    }
    if (ov && a.overflow) a.overflow[n] = 1;  // (lanes of one item race to store the same 1)
  }
}

// ---- S = 16, 25, R <= 256: frame 0 on the matrix cores -------------------------------------------------------------
template <int S>
constexpr int items_mfma_lds_bytes(int RS) { return MGeo<S>::TROWS * RS + MGeo<S>::IMG; }

template <typename Rows, int S, typename OutT, typename... X>
__global__ __launch_bounds__(kBlock) void items_mfma_kernel(ItemArgs a, X... x) {
  using G = MGeo<S>;
  using TM = TileMap<S>;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ int fac[kRch * G::A3];  // the exact form's rows
  __shared__ int rk[G::A3];
  const Rows rows{x...};
  const int RS = a.RS;
  int8_t* const Tf = reinterpret_cast<int8_t*>(lds);  // row x < 3S: factor x of the suffix rows; rows 3S..2S+31: zero
  uint8_t* const img = lds + G::TROWS * RS;           // frame 0, S^3 bytes
  const int t = threadIdx.x, wave = t >> 6, col = t & 31, h = (t >> 5) & 1;
  for (int q = t; q < (G::TROWS - G::A3) * RS; q += kBlock) Tf[G::A3 * RS + q] = 0;  // the w rows past S, for good
  TM tm;
  make_tile_map(tm, RS, wave, col, h);
  for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
    if constexpr (Rows::kMixed) {
      if (rows.write_stored(a, n, static_cast<OutT*>(a.frames) + n * a.T * G::N, t, kBlock)) continue;
    }
    const Item it = row_item(a, rows, n);
    OutT* out = static_cast<OutT*>(a.frames) + n * a.T * G::N;
    write_meta(a, n, it, t, kBlock);
    int ov = 0;
    if (it.valid) {
      const int K = a.R - 1 - it.k, Kp = (K + 31) & ~31;
      const int8_t* suffix = a.tokens + (it.d * a.R + it.k + 1) * G::A3;
      const int8_t* tgt = a.targets + it.d * a.tstride;
      if (a.vec) {
        for (int c = t; c < G::N / 16; c += kBlock)
          *reinterpret_cast<uint4*>(img + 16 * c) = *reinterpret_cast<const uint4*>(tgt + 16 * c);
        if (G::TAIL && t < G::TAIL) img[G::N - G::TAIL + t] = static_cast<uint8_t>(tgt[G::N - G::TAIL + t]);
      } else {
        for (int e = t; e < G::N; e += kBlock) img[e] = static_cast<uint8_t>(tgt[e]);
      }
      // the suffix rows, transposed: Tf[x][r] = factor x of row k+1+r, zero for K <= r < Kp
      int bad = 0;
      for (int q = t; q < Kp * G::A3; q += kBlock) {
        const int r = q / G::A3, x = q - r * G::A3;
        const int v = r < K ? suffix[q] - a.shift : 0;
        bad |= x < 2 * S ? (v > G::UVLIM || v < -G::UVLIM) : (v > 127 || v < -128);
        Tf[x * RS + r] = static_cast<int8_t>(v);
      }
      if (!__syncthreads_or(bad)) {
        if (K > 0) {
          int hi = -128, lo = 127;
#pragma unroll
          for (int k = 0; k < TM::TPW; ++k) {
            if (G::NT % TM::NW != 0 && wave + TM::NW * k >= G::NT) break;  // wave-uniform
            v16i acc;
#pragma unroll
            for (int t2 = 0; t2 < 16; ++t2) acc[t2] = 0;
            for (int k0 = 0; k0 < Kp; k0 += 32) {
              const v4i w = *reinterpret_cast<const v4i*>(Tf + tm.woff + k0);
              const v4i p = bytemul16(*reinterpret_cast<const v4i*>(Tf + tm.uoff[k] + k0),
                                      *reinterpret_cast<const v4i*>(Tf + tm.voff[k] + k0));
              acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, p, acc, 0, 0, 0);
            }
            if (tm.ncol[k] >= 0) {  // acc[t2] = row l = (t2 & 3) + 8 (t2 >> 2) + 4 h of column ncol: entry ncol * S + l
              uint8_t* dst = img + tm.ncol[k] * S + 4 * h;
#pragma unroll
              for (int t2 = 0; t2 < 16; ++t2) {
                const int o = (t2 & 3) + 8 * (t2 >> 2);
                if (o + 4 * h < S) {
                  const int v = static_cast<int>(static_cast<int8_t>(dst[o])) - acc[t2];
                  hi = max(hi, v);
                  lo = min(lo, v);
                  dst[o] = static_cast<uint8_t>(v);
                }
              }
            }
          }
          ov |= hi > 127 || lo < -128;
        }
      } else {
        exact_frame0<S>(suffix, K, S, a.shift, img, fac, t, ov);
      }
      __syncthreads();
      write_frame(out, G::N, t, kBlock, [&](int e) { return static_cast<int>(static_cast<int8_t>(img[e])); });
    } else {
      write_frame(out, G::N, t, kBlock, [](int) { return 0; });
    }
    write_action_frames<S>(a, out, it, t, rk, ov);
    set_overflow(a, n, ov, t);
  }
}

}  // namespace tg

namespace {

template <typename K, typename... X>
int launch_items(K kernel, const char* fn, const tg::ItemArgs& a, int64_t items, int lds, int per_cu, hipStream_t st,
                 const X&... x) {
  const int64_t resident = static_cast<int64_t>(per_cu) * device_cu_count();
  const int64_t grid = items < resident ? items : resident;  // several items per workgroup beyond one wave of them
  return launch(fn, kernel, static_cast<unsigned>(grid), tg::kBlock, lds, st, a, x...);
}

// The per-size kernel choice of every items entry.  Kn names the entry (kName) and its __global__ instantiations
// (s4<OutT, Acc>(), mfma<S, OutT>(), exact<OutT>()); x... are the kernels' arguments after the ItemArgs.
template <typename OutT, typename Kn, typename... X>
int dispatch_items(const tg::ItemArgs& a0, hipStream_t st, const X&... x) {
  tg::ItemArgs a = a0;
  const int S = a.S;
  if (S == 4) {
    a.vec = aligned(a.frames, 16);
    const double fmax = 128.0 + (a.shift < 0 ? -static_cast<double>(a.shift) : a.shift);
    const bool narrow = (a.R - 1) * fmax * fmax * fmax + 128.0 < 2147483647.0;
    const int64_t wgs = (a.N + tg::kBlock / 16 - 1) / (tg::kBlock / 16);
    if (narrow) return launch_items(Kn::template s4<OutT, int32_t>(), Kn::kName, a, wgs, 0, 8, st, x...);
    return launch_items(Kn::template s4<OutT, int64_t>(), Kn::kName, a, wgs, 0, 8, st, x...);
  }
  if ((S == 16 || S == 25) && a.R <= 256) {
    a.RS = ((a.R - 1 + 31) & ~31) + 16;
    a.vec = aligned(a.targets, 16) && a.tstride % 16 == 0;
    if (S == 16) {
      constexpr auto k = Kn::template mfma<16, OutT>();
      const int lds = tg::items_mfma_lds_bytes<16>(a.RS);
      return launch_items(k, Kn::kName, a, a.N, lds, resident_per_cu<k>(lds), st, x...);
    }
    constexpr auto k = Kn::template mfma<25, OutT>();
    const int lds = tg::items_mfma_lds_bytes<25>(a.RS);
    return launch_items(k, Kn::kName, a, a.N, lds, resident_per_cu<k>(lds), st, x...);
  }
  constexpr auto k = Kn::template exact<OutT>();
  const int lds = (S * S * S + 15) & ~15;
  return launch_items(k, Kn::kName, a, a.N, lds, resident_per_cu<k>(lds), st, x...);
}

// An items entry after its own checks: the checks on the item list and the output, then the launch in the output dtype.
template <typename Kn, typename... X>
int run_items(const tg::ItemArgs& a, int out_dtype, hipStream_t st, const X&... x) {
  const char* fn = Kn::kName;
  const int64_t N3 = static_cast<int64_t>(a.S) * a.S * a.S;
  if (a.N < 0 || a.N > INT64_MAX / (a.T * N3))
    return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)a.N);
  if (a.N == 0) return TG_OK;
  if (!a.idx || !a.frames) return tg_internal_fail(TG_ERR_INVALID, "%s: null item_idx or frames_out", fn);
  if (a.n_demos > 0 && (!a.tokens || !a.targets)) return tg_internal_fail(TG_ERR_INVALID, "%s: null tokens or targets", fn);
  const int esize = out_dtype == 3 ? 1 : out_dtype == 0 ? 4 : 2;
  if (!aligned(a.frames, esize))
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames_out not aligned to its %d-byte elements", fn, esize);
  switch (out_dtype) {
    case 0: return dispatch_items<float, Kn>(a, st, x...);
    case 1: return dispatch_items<__half, Kn>(a, st, x...);
    case 2: return dispatch_items<__hip_bfloat16, Kn>(a, st, x...);
    default: return dispatch_items<int8_t, Kn>(a, st, x...);
  }
}

// The checks every items entry makes first: the demonstration set and the item shape.
int check_items(const char* fn, int64_t n_demos, int R, int S, int64_t target_stride_bytes, int T, int out_dtype) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (R < 1 || R > TG_DEMO_MAX_ACTIONS)
    return tg_internal_fail(TG_ERR_INVALID, "%s: R=%d outside [1,%d]", fn, R, TG_DEMO_MAX_ACTIONS);
  if (T < 1 || T > TG_DEMO_MAX_T) return tg_internal_fail(TG_ERR_INVALID, "%s: T=%d outside [1,%d]", fn, T, TG_DEMO_MAX_T);
  if (n_demos < 0 || n_demos > INT64_MAX / R)
    return tg_internal_fail(TG_ERR_INVALID, "%s: n_demos=%lld out of range", fn, (long long)n_demos);
  const int64_t N3 = static_cast<int64_t>(S) * S * S;
  if (target_stride_bytes < N3)
    return tg_internal_fail(TG_ERR_INVALID, "%s: target_stride_bytes=%lld < S^3=%lld", fn, (long long)target_stride_bytes,
                            (long long)N3);
  if (out_dtype < 0 || out_dtype > 3)
    return tg_internal_fail(TG_ERR_INVALID, "%s: out_dtype=%d (0 f32, 1 f16, 2 bf16, 3 int8)", fn, out_dtype);
  return TG_OK;
}

}  // namespace
