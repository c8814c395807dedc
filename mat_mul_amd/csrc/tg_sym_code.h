// tg_sym_code.h -- the mode-permutation code of include/tensor_game_symmetry.h, shared by the kernels that decode a
// row of `sym` (tg_symmetry.hip, tg_orbits.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tg {

constexpr int kSymNeg = 1 << 16;
// rho[m] of the mode permutation `code` (lexicographic rank): six codes x three modes x two bits
constexpr uint64_t kRho = (0ull | 1ull << 2 | 2ull << 4) | (0ull | 2ull << 2 | 1ull << 4) << 6 |
                          (1ull | 0ull << 2 | 2ull << 4) << 12 | (1ull | 2ull << 2 | 0ull << 4) << 18 |
                          (2ull | 0ull << 2 | 1ull << 4) << 24 | (2ull | 1ull << 2 | 0ull << 4) << 30;
__device__ __forceinline__ int rho_of(int code, int m) { return static_cast<int>(kRho >> (6 * code + 2 * m)) & 3; }

}  // namespace tg
