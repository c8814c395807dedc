// tg_lists.h -- the host half the entries over action lists share (tokens int8 (M,K,3S), lengths int64 (M), shift:
// tg_solutions.hip, tg_orbits.hip, tg_bases.hip, tg_flips.hip): the size checks, a list's LDS image size, the launch on a
// grid the device holds at once, the canon entries' pointer checks.  The first failing check is what a caller sees.
#pragma once
#include "../../include/tensor_game_solutions.h"
#include "tg_host.h"

namespace tg {

// S, K and shift of a list entry.  max_k is the entry's own bound on K; max_row, where given, its bound on K * 3S.
inline int check_lists(const char* fn, int K, int S, int shift, int max_k, int max_row = INT32_MAX) {
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (K < 1 || K > max_k) return tg_internal_fail(TG_ERR_INVALID, "%s: K=%d outside [1,%d]", fn, K, max_k);
  if (K * 3 * S > max_row) return tg_internal_fail(TG_ERR_INVALID, "%s: K*3S=%d above %d", fn, K * 3 * S, max_row);
  if (shift < 0 || shift > TG_SOL_MAX_SHIFT)
    return tg_internal_fail(TG_ERR_INVALID, "%s: shift=%d outside [0,%d]", fn, shift, TG_SOL_MAX_SHIFT);
  return TG_OK;
}

// M lists of up to TG_SOL_MAX_K terms with their targets: every byte offset stays inside int64
inline int check_list_count(const char* fn, int64_t M) {
  constexpr int64_t most = INT64_MAX / (static_cast<int64_t>(TG_SOL_MAX_K) * 3 * TG_MAX_S * TG_MAX_S);
  return M < 0 || M > most ? tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M) : TG_OK;
}

// bytes of a list's image in LDS: K * 3S rounded up to 16 (at most 24 KiB)
inline int list_image_bytes(int K, int S) { return (K * 3 * S + 15) & ~15; }

// launch `kernel` with a workgroup per item of `work` >= 1, up to per_cu on each CU (grid-stride loops take the rest)
template <typename Kern, typename... A>
int launch_resident(const char* fn, Kern kernel, int64_t work, int per_cu, int threads, size_t lds, hipStream_t st,
                    const A&... args) {
  const int64_t resident = static_cast<int64_t>(per_cu) * device_cu_count();
  return launch(fn, kernel, static_cast<unsigned>(work < resident ? work : resident), threads, lds, st, args...);
}

// the pointers tg_solution_canon takes, and behind `orbit` the three tg_orbit_canon adds
struct CanonPointers {
  const void *targets, *tokens, *lengths, *canon, *rank, *key, *residual, *status;
  bool orbit = false;
  const void *sym = nullptr, *which = nullptr, *stab = nullptr;
};

// the null, aliasing and alignment checks of the two canon entries, tg_orbit_canon's own at their places among the rest
inline int check_canon_pointers(const char* fn, const CanonPointers& p) {
  auto fail = [fn](const char* what) { return tg_internal_fail(TG_ERR_INVALID, "%s: %s", fn, what); };
  if (!p.tokens) return fail("null tokens");
  if (!p.lengths) return fail("null lengths");
  if (p.orbit && !p.sym) return fail("null sym");
  if (!p.canon) return fail("null canon");
  if (!p.rank) return fail("null rank");
  if (!p.key) return fail("null key");
  if (p.orbit && !p.which) return fail("null which");
  if (p.orbit && !p.stab) return fail("null stab");
  if (!p.targets && p.residual) return fail("residual_nnz needs targets (both NULL: no verification)");
  if (p.canon == p.tokens) return fail("canon == tokens: in-place operation is not supported");
  if (!aligned(p.lengths, 8)) return fail("lengths not 8-byte aligned");
  if (!aligned(p.key, 8)) return fail("key not 8-byte aligned");
  if (!aligned(p.rank, 4)) return fail("rank not 4-byte aligned");
  if (!aligned(p.residual, 4)) return fail("residual_nnz not 4-byte aligned");
  if (p.orbit && !aligned(p.which, 4)) return fail("which not 4-byte aligned");
  if (p.orbit && !aligned(p.stab, 4)) return fail("stab not 4-byte aligned");
  if (!aligned(p.status, 4)) return fail("status not 4-byte aligned");
  return TG_OK;
}

}  // namespace tg

using tg::check_canon_pointers;
using tg::check_list_count;
using tg::check_lists;
using tg::launch_resident;
using tg::list_image_bytes;
