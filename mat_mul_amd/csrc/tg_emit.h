// tg_emit.h -- int8 values -> 16 bytes of a model-input frame (float32, float16, bfloat16; int8 as is), shared by
// tg_aux.hip (tg_emit_frames, tg_step_emit) and tg_items.hip (tg_demo_items).
#pragma once
#include <type_traits>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include "tg_device.h"

namespace tg {

// 16 output bytes from PER = 16 / sizeof(OutT) int8 values (int8 output: their low bytes; small integers: exact in float32, float16 and bfloat16
// alike).  Built in registers, word by word: an `OutT v[PER]` array + memcpy made hipcc stage the values through LDS,
// and the f16 / bf16 kernels took 33 us where the f32 kernel took 13.5 (S=4, B=65 536, T=4).
template <typename OutT>
__device__ __forceinline__ uint4 emit_pack(const int (&x)[16 / sizeof(OutT)]) {
  if constexpr (sizeof(OutT) == 1) {  // int8: the low bytes
    return uint4{pack4(x[0], x[1], x[2], x[3]), pack4(x[4], x[5], x[6], x[7]), pack4(x[8], x[9], x[10], x[11]),
                 pack4(x[12], x[13], x[14], x[15])};
  } else if constexpr (sizeof(OutT) == 4) {
    return uint4{__float_as_uint(static_cast<float>(x[0])), __float_as_uint(static_cast<float>(x[1])),
                 __float_as_uint(static_cast<float>(x[2])), __float_as_uint(static_cast<float>(x[3]))};
  } else {
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const float lo = static_cast<float>(x[2 * d]), hi = static_cast<float>(x[2 * d + 1]);
      if constexpr (std::is_same<OutT, __half>::value) {
        typedef __fp16 h2_t __attribute__((ext_vector_type(2)));
        const h2_t h = __builtin_amdgcn_cvt_pkrtz(lo, hi);  // |x| <= 128: exact whatever the rounding
        __builtin_memcpy(&w[d], &h, 4);
      } else {  // bfloat16 = the upper half of the float32 (|x| <= 128 has at most 8 significant bits: exact)
        w[d] = __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
      }
    }
    return uint4{w[0], w[1], w[2], w[3]};
  }
}
// element t of a packed group (the last, partial group of the output)
template <typename OutT>
__device__ __forceinline__ void emit_store_one(OutT* out, const uint4& o, int t) {
  const uint32_t w[4] = {o.x, o.y, o.z, o.w};
  if constexpr (sizeof(OutT) == 1) *reinterpret_cast<uint8_t*>(out) = static_cast<uint8_t>(w[t >> 2] >> (8 * (t & 3)));
  else if constexpr (sizeof(OutT) == 4) *reinterpret_cast<uint32_t*>(out) = w[t];
  else *reinterpret_cast<uint16_t*>(out) = static_cast<uint16_t>(w[t >> 1] >> (16 * (t & 1)));
}

}  // namespace tg
