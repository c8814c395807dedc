// tg_sol_copy.h -- the byte copies between an action list in global memory (any alignment) and its image in LDS that
// the solution kernels share (tg_solutions.hip, tg_bases.hip): 16-byte accesses where the global side is 16-byte
// aligned, byte accesses otherwise and for the tail.  NT = the threads of the workgroup, t = this thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tg {

// n bytes from global memory (any alignment) into LDS (16-byte aligned)
template <int NT>
__device__ __forceinline__ void sol_copy_in(const int8_t* src, int8_t* dst, int n, int t) {
  int nb = 0;
  if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    nb = n / 16;
    for (int c = t; c < nb; c += NT) reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
  }
  for (int e = 16 * nb + t; e < n; e += NT) dst[e] = src[e];
}

// n bytes to global memory (any alignment) from LDS (16-byte aligned), or zeros when src is null
template <int NT>
__device__ __forceinline__ void sol_copy_out(int8_t* dst, const int8_t* src, int n, int t) {
  int nb = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    nb = n / 16;
    for (int c = t; c < nb; c += NT)
      reinterpret_cast<uint4*>(dst)[c] = src ? reinterpret_cast<const uint4*>(src)[c] : uint4{0, 0, 0, 0};
  }
  for (int e = 16 * nb + t; e < n; e += NT) dst[e] = src ? src[e] : static_cast<int8_t>(0);
}

}  // namespace tg
