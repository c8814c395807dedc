// Symmetry augmentation of training items (include/tensor_game_symmetry.h): tg_symmetry_apply applies one signed
// permutation per mode and one mode permutation to every frame and to the action of an item, tg_symmetry_sample draws
// the group elements.  gfx950 only; part of libtensorgame.so.
//
// The apply kernel, per item: a TEAM of threads (a 256-thread workgroup at S >= 6, 16 lanes at S <= 5, sixteen items
// per workgroup there) checks the item's sym row, decodes it into three LDS tables, and then per frame stages the S^3
// input bytes into LDS with 16-byte loads (head and tail bytes one by one: a frame starts at any byte) and produces the
// output in output order, 16 bytes per store through the head / body / tail split of write_frame (tg_items.h).
//   tab[m][a] = pi_m[a] * S^(2 - rho[m])  |  (s_m[a] < 0) << 16
// so entry (a0,a1,a2) is  x = tab[0][a0] + tab[1][a1] + tab[2][a2]:  the input offset in the low 15 bits (< S^3 <= 2^15)
// and the parity of the three signs in bit 16.  A thread walks (a0,a1,a2) incrementally -- within its 16 bytes and from
// one 16 bytes to its next -- so an entry costs the table reads, the adds and one LDS byte read, and no division.
// The permutation costs LDS traffic only: global memory sees one contiguous read and one contiguous write per frame.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_symmetry.h"
#include "tg_items.h"
#include "tg_sym_code.h"

namespace tg {

struct SymArgs {
  const int8_t* fin;   // (N, T, S, S, S)
  const int8_t* ain;   // (N, 3S) or null
  const uint8_t* sym;  // (N, 3S+1)
  int64_t N;
  void* fout;          // (N, T, S, S, S) of OutT
  int8_t* aout;        // (N, 3S) or null
  uint8_t* overflow;
  uint32_t* status;
  int T, S, shift;
  int img;             // bytes of LDS per team: S^3 + 16, rounded up to 16
};

// One input frame (N3 bytes at src, any alignment) into LDS: 16-byte loads between the first and the last 16-byte
// boundary of src, bytes before and after.  img is 16-byte aligned with N3 + 16 bytes; entry e lands at img[pad + e],
// pad = src mod 16, which keeps the 16-byte LDS writes aligned.  Returns the image's first entry.
template <int NT>
__device__ __forceinline__ const uint8_t* stage_frame(const int8_t* src, uint8_t* img, int N3, int t) {
  const int pad = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15u);
  int head = (16 - pad) & 15;
  head = head < N3 ? head : N3;
  const int nbody = (N3 - head) / 16;
  uint8_t* dst = img + pad;
  for (int e = t; e < head; e += NT) dst[e] = static_cast<uint8_t>(src[e]);
  for (int c = t; c < nbody; c += NT)
    *reinterpret_cast<uint4*>(dst + head + 16 * c) = *reinterpret_cast<const uint4*>(src + head + 16 * c);
  for (int e = head + 16 * nbody + t; e < N3; e += NT) dst[e] = static_cast<uint8_t>(src[e]);
  return dst;
}

// entry x of the staged frame: the int8 value, negated (with the wrap of -128 flagged) when bit 16 of x is set
__device__ __forceinline__ int sym_entry(const uint8_t* img, int x, int& ov) {
  int v = static_cast<int8_t>(img[x & 0x7fff]);
  v = (x & kSymNeg) ? -v : v;
  ov |= v == 128;
  return v == 128 ? -128 : v;
}

// One output frame from the staged input: the split of write_frame, with the (a0,a1,a2) walk in place of e -> get(e).
// tab: three tables TS ints apart.  ABL (the A/B build's ablations, tools/symmetry_bench.py; 0 in the product): 1 = the body
// reads the staged bytes in input order, no table reads and no walk; 2 = the body's 16-byte stores are not issued.
template <typename OutT, int NT, int TS, int ABL = 0>
__device__ __forceinline__ void sym_write_frame(OutT* dst, const uint8_t* img, const int* tab, int S, int t, int& ov) {
  constexpr int PER = 16 / sizeof(OutT);
  const int S2 = S * S, N3 = S2 * S;
  int head = static_cast<int>(((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(OutT));
  head = head < N3 ? head : N3;
  const int nbody = (N3 - head) / PER;
  auto get = [&](int e) {  // the few entries outside the 16-byte body: by division
    const int i = e / S2, r = e - i * S2, j = r / S;
    return sym_entry(img, tab[i] + tab[TS + j] + tab[2 * TS + r - j * S], ov);
  };
  for (int e = t; e < head; e += NT) store1(dst + e, get(e));
  OutT* body = dst + head;
  // this thread's first entry and the step from one of its 16 bytes to the next, as (a0,a1,a2) digits
  constexpr int STEP = NT * PER;
  const int d0 = STEP / S2, dr = STEP - d0 * S2, d1 = dr / S, d2 = dr - d1 * S;
  const int e0 = head + t * PER;
  int a0 = e0 / S2, a1 = (e0 - a0 * S2) / S, a2 = e0 - a0 * S2 - a1 * S;
  for (int c = t; c < nbody; c += NT) {
    int b0 = a0, b1 = a1, b2 = a2, x01 = tab[b0] + tab[TS + b1];
    int x[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      if constexpr (ABL == 1) {
        x[q] = sym_entry(img, head + c * PER + q, ov);
        continue;
      }
      x[q] = sym_entry(img, x01 + tab[2 * TS + b2], ov);
      if (++b2 == S) {
        b2 = 0;
        if (++b1 == S) {
          b1 = 0;
          ++b0;  // (== S only behind the frame's last entry: tab[S] is inside the tables and the sum is not used)
        }
        x01 = tab[b0] + tab[TS + b1];
      }
    }
    if (ABL != 2 || x[0] == 0x7fffffff) *reinterpret_cast<uint4*>(body + c * PER) = emit_pack<OutT>(x);  // (never 2^31 - 1)
    a2 += d2;
    if (a2 >= S) a2 -= S, ++a1;
    a1 += d1;
    if (a1 >= S) a1 -= S, ++a0;
    a0 += d0;
  }
  for (int e = head + nbody * PER + t; e < N3; e += NT) store1(dst + e, get(e));
}

// NT threads per item: 256 (one item per workgroup at a time) or 16 (sixteen items per workgroup, S <= 5).
// Every loop bound and barrier is uniform over the workgroup; a team without an item (n >= N) touches no global memory.
template <typename OutT, int NT, int ABL = 0>
__global__ __launch_bounds__(kBlock) void symmetry_apply_kernel(SymArgs a) {
  constexpr int TEAMS = kBlock / NT;
  constexpr int TS = NT == kBlock ? TG_MAX_S : 8;  // ints per table
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // TEAMS images of a.img bytes
  __shared__ int tabs[TEAMS][3 * TS + 1];
  const int team = threadIdx.x / NT, t = threadIdx.x % NT;
  const int S = a.S, S2 = S * S, N3 = S2 * S, A3 = 3 * S;
  uint8_t* const img = lds + team * a.img;
  int* const tab = tabs[team];
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * TEAMS; base < a.N; base += static_cast<int64_t>(gridDim.x) * TEAMS) {
    const int64_t n = base + team;
    const bool active = n < a.N;
    // the row's bytes are checked before any of them addresses anything
    const bool mine = active && t >= 1 && t <= A3;  // thread t holds byte t: position a of mode m, t = 1 + m*S + a
    const uint8_t* row = a.sym + n * (A3 + 1);
    int code = active ? row[0] : 0;
    const int b = mine ? row[t] : 0;
    const bool bad1 = (t == 0 && code > 5) || (b & 127) >= S;
    bool bad;
    if constexpr (NT == kBlock) bad = __syncthreads_or(bad1);
    else bad = team_any<NT>(bad1);
    int ov = 0;
    if (mine) {
      const int m = (t - 1) / S, p = b & 127;
      int8_t tok = 0;
      if (!bad) {
        const int rm = rho_of(code, m);
        tab[m * TS + (t - 1 - m * S)] = p * (rm == 0 ? S2 : rm == 1 ? S : 1) | ((b & 128) ? kSymNeg : 0);
        if (a.aout) {
          int64_t v = a.ain[n * A3 + rm * S + p];
          if (b & 128) v = 2 * static_cast<int64_t>(a.shift) - v;
          ov |= v < -128 || v > 127;
          tok = static_cast<int8_t>(v);
        }
      }
      if (a.aout) a.aout[n * A3 + t - 1] = tok;
    }
    if (bad && active && t == 0 && a.status) atomicOr(a.status, 1u);
    for (int f = 0; f < a.T; ++f) {
      const int64_t fr = (n * a.T + f) * N3;
      const uint8_t* in = img;
      if (active && !bad) in = stage_frame<NT>(a.fin + fr, img, N3, t);
      lds_barrier();  // the tables and the frame are in LDS
      if (active) {
        OutT* dst = static_cast<OutT*>(a.fout) + fr;
        if (bad) write_frame(dst, N3, t, NT, [](int) { return 0; });
        else sym_write_frame<OutT, NT, TS, ABL>(dst, in, tab, S, t, ov);
      }
      lds_barrier();  // the frame's readers are done (and, after the last frame, the tables')
    }
    if constexpr (NT == kBlock) {
      if (__syncthreads_or(ov) && t == 0 && a.overflow) a.overflow[n] = 1;
    } else {
      if (ov && a.overflow) a.overflow[n] = 1;  // (lanes of one item race to store the same 1)
    }
  }
}

// ---- the sampler: one thread per (item, mode); its permutation lives in LDS bytes (entry a of thread t at
// perm[a * kBlock + t]), so the Fisher-Yates swaps index LDS and no register array.
struct SymSample {
  uint8_t* out;
  int64_t N;
  uint64_t id0;
  uint32_t seed_lo, seed_hi;
  int S, flags;
};

__global__ __launch_bounds__(kBlock) void symmetry_sample_kernel(SymSample a) {
  __shared__ uint8_t perm[TG_MAX_S * kBlock];
  const int t = threadIdx.x, S = a.S;
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + t;
  if (q >= 3 * a.N) return;
  const int64_t n = q / 3;
  const int m = static_cast<int>(q - 3 * n);
  const uint64_t id = a.id0 + static_cast<uint64_t>(n);
  U4 o{};
  uint32_t cur = ~0u;
  auto word = [&](int i) {  // w[i] of the item's stream, block by block
    const uint32_t blk = static_cast<uint32_t>(i) >> 2;
    if (blk != cur) {
      o = philox4x32_10(U4{static_cast<uint32_t>(id), static_cast<uint32_t>(id >> 32), blk, 0x53000000u}, a.seed_lo,
                        a.seed_hi);
      cur = blk;
    }
    const int k = i & 3;
    return k == 0 ? o.x : k == 1 ? o.y : k == 2 ? o.z : o.w;
  };
  uint8_t* row = a.out + n * (3 * S + 1);
  if (m == 0) {
    const uint32_t code = static_cast<uint32_t>((static_cast<uint64_t>(word(0)) * 6u) >> 32);
    row[0] = (a.flags & TG_SYM_MODES) ? static_cast<uint8_t>(code) : 0;
  }
  uint8_t* p = perm + t;
  for (int x = 0; x < S; ++x) p[x * kBlock] = static_cast<uint8_t>(x);
  const int w0 = 1 + m * S;
  if (a.flags & TG_SYM_PERMS) {
    for (int x = S - 1; x >= 1; --x) {
      const int j = static_cast<int>((static_cast<uint64_t>(word(w0 + S - 1 - x)) * static_cast<uint32_t>(x + 1)) >> 32);
      const uint8_t px = p[x * kBlock], pj = p[j * kBlock];
      p[x * kBlock] = pj;
      p[j * kBlock] = px;
    }
  }
  const uint32_t sg = (a.flags & TG_SYM_SIGNS) ? word(w0 + S - 1) : 0u;
  for (int x = 0; x < S; ++x) row[w0 + x] = p[x * kBlock] | (((sg >> x) & 1u) << 7);
}

}  // namespace tg

namespace {

template <typename OutT, int ABL>
int launch_symmetry_wg(const tg::SymArgs& a, hipStream_t st) {  // one 256-thread workgroup per item at a time
  constexpr auto k = tg::symmetry_apply_kernel<OutT, tg::kBlock, ABL>;
  const int64_t resident = static_cast<int64_t>(resident_per_cu<k>(a.img)) * device_cu_count();
  return launch("tg_symmetry_apply", k, static_cast<unsigned>(a.N < resident ? a.N : resident), tg::kBlock, a.img, st, a);
}

template <typename OutT>
int launch_symmetry(tg::SymArgs a, hipStream_t st) {
  const char* fn = "tg_symmetry_apply";
  const int N3 = a.S * a.S * a.S;
  a.img = (N3 + 16 + 15) & ~15;
  if (a.S <= 5) {  // 16 lanes per item
    constexpr int IPB = tg::kBlock / 16;
    const int64_t wgs = (a.N + IPB - 1) / IPB, resident = 8ll * device_cu_count();
    return launch(fn, tg::symmetry_apply_kernel<OutT, 16>, static_cast<unsigned>(wgs < resident ? wgs : resident),
                  tg::kBlock, IPB * a.img, st, a);
  }
#ifdef TG_AB_SWITCHES  // measurement only: the ablations of the S >= 6 kernel
  if (TG_SWITCH("TG_SYM_NO_PERM")) return launch_symmetry_wg<OutT, 1>(a, st);
  if (TG_SWITCH("TG_SYM_NO_STORE")) return launch_symmetry_wg<OutT, 2>(a, st);
#endif
  return launch_symmetry_wg<OutT, 0>(a, st);
}

}  // namespace

extern "C" int tg_symmetry_apply(const int8_t* frames_in, const int8_t* actions_in, const uint8_t* sym, int64_t N, int T,
                                 int S, int shift, int out_dtype, void* frames_out, int8_t* actions_out,
                                 uint8_t* overflow, uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_symmetry_apply";
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (T < 1 || T > TG_DEMO_MAX_T) return tg_internal_fail(TG_ERR_INVALID, "%s: T=%d outside [1,%d]", fn, T, TG_DEMO_MAX_T);
  if (out_dtype < 0 || out_dtype > 3)
    return tg_internal_fail(TG_ERR_INVALID, "%s: out_dtype=%d (0 f32, 1 f16, 2 bf16, 3 int8)", fn, out_dtype);
  const int64_t N3 = static_cast<int64_t>(S) * S * S;
  if (N < 0 || N > INT64_MAX / (T * N3 * 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)N);
  if (N == 0) return TG_OK;
  if (!frames_in || !frames_out || !sym) return tg_internal_fail(TG_ERR_INVALID, "%s: null frames_in, frames_out or sym", fn);
  if ((actions_in == nullptr) != (actions_out == nullptr))
    return tg_internal_fail(TG_ERR_INVALID, "%s: actions_in and actions_out must be given or NULL together", fn);
  if (frames_out == static_cast<const void*>(frames_in) || (actions_out && actions_out == actions_in))
    return tg_internal_fail(TG_ERR_INVALID, "%s: in-place operation is not supported", fn);
  const int esize = out_dtype == 3 ? 1 : out_dtype == 0 ? 4 : 2;
  if (!aligned(frames_out, esize))
    return tg_internal_fail(TG_ERR_INVALID, "%s: frames_out not aligned to its %d-byte elements", fn, esize);
  const tg::SymArgs a{frames_in, actions_in, sym, N, frames_out, actions_out, overflow, status, T, S, shift, 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (out_dtype) {
    case 0: return launch_symmetry<float>(a, st);
    case 1: return launch_symmetry<__half>(a, st);
    case 2: return launch_symmetry<__hip_bfloat16>(a, st);
    default: return launch_symmetry<int8_t>(a, st);
  }
}

extern "C" int tg_symmetry_sample(uint8_t* sym_out, int64_t N, int S, uint64_t seed, uint64_t item_offset, int flags,
                                  tg_stream_t stream) {
  const char* fn = "tg_symmetry_sample";
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (flags & ~(TG_SYM_MODES | TG_SYM_PERMS | TG_SYM_SIGNS))
    return tg_internal_fail(TG_ERR_INVALID, "%s: flags=%d has unknown bits", fn, flags);
  if (N < 0 || N > (INT64_MAX / 3) / (3 * S + 1)) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)N);
  if (N == 0) return TG_OK;
  if (!sym_out) return tg_internal_fail(TG_ERR_INVALID, "%s: null sym_out", fn);
  const int64_t wgs = (3 * N + tg::kBlock - 1) / tg::kBlock;
  if (wgs > 0x7fffffffll) return tg_internal_fail(TG_ERR_INVALID, "%s: N=%lld out of range", fn, (long long)N);
  const tg::SymSample a{sym_out, N, item_offset, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), S, flags};
  return launch(fn, tg::symmetry_sample_kernel, static_cast<unsigned>(wgs), tg::kBlock, 0, static_cast<hipStream_t>(stream), a);
}
