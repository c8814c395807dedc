// tg_host.h -- the host half every source of libtensorgame.so shares: the library-internal declarations, the launch and
// its error check, grid sizing, the common argument checks, and the per-device queries (CU count, occupancy, the dynamic
// LDS opt-in), cached per device with relaxed atomics: two host threads racing on a cold entry both query and store the
// same value.  Host-only; none of it is a stream operation, so every call is legal while a stream is being captured.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/tensor_game.h"
#include "tg_device.h"

// Library-internal, not part of the C ABI.
int tg_internal_fail(int code, const char* fmt, ...);  // records tg_last_error(), returns code (tg_kernels.hip)
// the key pass of tg_expand_keyed_i8 (tg_aux.hip)
extern "C" int tg_internal_hash(const int8_t* state, uint64_t* hash_out, int64_t B, int S, int64_t stride, hipStream_t st);
// the last launch of every entry that stores games in a replay ring (tg_ring.h): offset = the exclusive prefix sums of
// length (tg_replay.hip)
struct tg_replay_buffer;
int tg_internal_ring_rebuild(const tg_replay_buffer* buf, hipStream_t st);
namespace tg { struct Dist; }
// the generator in one kernel (tg_genfused.h, launched from the host side of tg_kernels.hip), called by tg_gen_demos_i8 (tg_gen.hip):
// 1 = launched, 0 = not applicable (the caller takes the token kernel + tg_gen_from_factors_i8), < 0 = error
int tg_internal_gen_fused(int8_t* target, int8_t* actions, uint8_t* overflow, const int8_t* basis, int64_t B, int S,
                          int R, const tg::Dist& D, int shift, uint64_t seed, uint64_t gid0, int64_t stride,
                          hipStream_t st);

namespace tg {

constexpr int kMaxDevices = 64;
constexpr int kMaxDynamicLds = 160 * 1024;  // per workgroup on gfx950

// The error of the launch just made (and clears it).
inline int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tg_internal_fail(TG_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return TG_OK;
}

// Clear any earlier error, launch, check.
template <typename K, typename... A>
int launch(const char* fn, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return launched(fn);
}

// `blocks` workgroups clamped to [1, cap] (the kernels' grid-stride loops take the rest)
inline unsigned grid_for(int64_t blocks, int64_t cap = 1 << 20) {
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// Workgroups for B games when `resident` workgroups fit at once: every workgroup takes several games, split evenly.
inline unsigned even_grid(int64_t B, int64_t resident) {
  const int64_t per_wg = (B + resident - 1) / resident;
  return static_cast<unsigned>((B + per_wg - 1) / per_wg);
}

// f(OutT{}) for the model-input element type out_dtype names: 0 float, 1 __half, 2 __hip_bfloat16.
template <typename F>
int with_out_type(int out_dtype, F&& f) {
  if (out_dtype == 1) return f(__half{});
  if (out_dtype == 2) return f(__hip_bfloat16{});
  return f(float{});
}

inline bool aligned(const void* p, int bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// B games of S^3 bytes, `stride` bytes apart.
inline int check_state(const char* fn, int64_t B, int S, int64_t stride) {
  if (B < 0) return tg_internal_fail(TG_ERR_INVALID, "%s: B=%lld < 0", fn, (long long)B);
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (stride < (int64_t)S * S * S)
    return tg_internal_fail(TG_ERR_INVALID, "%s: game_stride_bytes=%lld < S^3=%d", fn, (long long)stride, S * S * S);
  return TG_OK;
}

inline int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -1;
  return dev;
}

inline int device_cu_count() {  // of the current device; 256 on MI355X
  static std::atomic<int> cached[kMaxDevices];
  const int dev = current_device();
  if (dev < 0) return 256;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (!n) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cached[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// Workgroups of K one CU holds at `lds` bytes of dynamic LDS, cached per (kernel instantiation, device): the slot packs
// (lds + 1) << 32 | value, so a different LDS size simply re-queries.  A host-side calculation on the code object.
template <auto K>
int resident_per_cu(int lds) {
  static std::atomic<uint64_t> slots[kMaxDevices];
  const int dev = current_device();
  const uint64_t tag = (static_cast<uint64_t>(lds) + 1) << 32;
  if (dev >= 0) {
    const uint64_t c = slots[dev].load(std::memory_order_relaxed);
    if ((c & ~0xffffffffull) == tag) return static_cast<int>(c & 0xffffffffull);
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K, kBlock, lds) != hipSuccess || n < 1) n = 1;
  (void)hipGetLastError();
  if (dev >= 0) slots[dev].store(tag | static_cast<uint32_t>(n), std::memory_order_relaxed);
  return n;
}

// The opt-in to more than 64 KiB of dynamic LDS for K, once per (kernel, device).  It asks for all the LDS a workgroup has
// beside K's static LDS, not the current launch's size, so a later launch with more LDS needs no second opt-in.
template <auto K>
int lds_opt_in(const char* fn, size_t lds) {
  static std::atomic<unsigned> done[kMaxDevices];
  if (lds <= 64 * 1024) return TG_OK;
  int dev = current_device();
  if (dev < 0) dev = 0;
  if (done[dev].load(std::memory_order_relaxed)) return TG_OK;
  const void* k = reinterpret_cast<const void*>(K);
  hipFuncAttributes fa{};
  hipError_t e = hipFuncGetAttributes(&fa, k);
  if (e == hipSuccess) {
    const int dynamic = kMaxDynamicLds - static_cast<int>(fa.sharedSizeBytes);
    e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, dynamic);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return tg_internal_fail(TG_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  done[dev].store(1, std::memory_order_relaxed);
  return TG_OK;
}

}  // namespace tg

using tg::aligned;
using tg::grid_for;
using tg::check_state;
using tg::device_cu_count;
using tg::even_grid;
using tg::launch;
using tg::launched;
using tg::lds_opt_in;
using tg::resident_per_cu;
using tg::with_out_type;
