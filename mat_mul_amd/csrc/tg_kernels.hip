// libtensorgame.so -- hand-written gfx950 (MI355X, CDNA4) kernels for the tensor-game hot path
// and the C ABI of include/tensor_game.h.  The single step, expand and the other byte-streaming
// entries are HBM-bound byte work on the vector ALU (state <- state - u(x)v(x)w, zero check); the
// accumulations over many rank-1 terms (generator, long step_many lists) run on the int8 matrix
// cores (tg_mfma.h).  See DESIGN.md.
//
// Kernel families, one header each, included once inside namespace tg below; this file keeps the host side
//   tg_apply.h : the modes, ApplyArgs; slow_*: one 256-thread workgroup per game, byte-granular, any S <= TG_MAX_S, any alignment.
//   tg_packed.h, tg_rows.h : packed_* / rows_* / s9_step / s25_step: aligned layouts, 16-byte chunks, int16 pairs.
//   tg_mfma.h, tg_genfused.h : *_mfma_*, gen_fused: accumulation over many terms on the matrix cores.
//   tg_s4.h : s4_*: S = 4 in registers only, 4 lanes per game.   tg_s16.h : s16_step / _emit / _tracked: a wavefront per game.
//   tg_stream.h : the resident steppers of tg_step_stream_i8.   tg_state.h : done / reset / copy.
//
// The PRODUCT build reads no environment variable and keeps no mutable host state besides per-device
// caches of device constants (atomics): TG_SWITCH() is constant false.  The A/B build (-DTG_AB_SWITCHES)
// turns the TG_* environment switches on.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/tensor_game.h"
#include "tg_device.h"
#include "tg_host.h"

namespace tg {

#include "tg_apply.h"
#include "tg_packed.h"
#include "tg_rows.h"
#include "tg_mfma.h"
#include "tg_genfused.h"
#include "tg_s4.h"
#include "tg_s16.h"
#include "tg_stream.h"
#include "tg_state.h"

}  // namespace tg

// =============================================================================================
// host side: validation, dispatch, C ABI
// =============================================================================================
static thread_local char g_err[512] = "";

// every source of the library reports through this (tg_host.h); not part of the C ABI
int tg_internal_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define fail tg_internal_fail

namespace {

// ---- the footprint thresholds of the dispatch below, each next to the measurement that placed it ----
// tg_step_i8 at S = 4: non-temporal state loads from this many bytes of states on (in place, measured: 64 MiB 23.1 / 24.0 us
// plain / nt, 128 MiB 48.6 / 44.9, 192 MiB 71.8 / 65.1, 256 MiB 92.4 / 85.4, 512 MiB 205 / 202, 1 GiB 432 / 410, 2 GiB
// 891 / 820, 4 GiB 1861 / 1666)
constexpr int64_t kS4NtLoadsFromBytes = 96ll << 20;
// tg_step_i8 at S = 4: from this many bytes of states on a lane awaits its token before it requests its slice
// (s4_step_kernel<.., TW>; placed by tools/step_sizes_bench.py sweeps; nt loads without / with the
// wait: 256 MiB 85.6 / 92.2 us, 512 MiB 202.0 / 188.3, 1 GiB 402.5 / 394.8, 1.5 GiB 611.3 / 580.2, 2 GiB 814.5 / 793.5)
constexpr int64_t kS4TokenWaitBytes = 384ll << 20;
// tg_step_i8 at S = 4: the sweep direction alternates ABOVE this many bytes of states (a batch that sits in the XCDs' L2s
// anyway -- BASELINE config 2 -- is swept in one direction)
constexpr int64_t kS4SweepAboveBytes = 16ll << 20;
// tg_step_i8 at S = 16 / 25: whole-line stores pay from ~100 MiB of states on (S = 16, measured: 6.0 / 7.0 us at 32 MiB,
// 26.3 / 25.5 at 128 MiB, 50.3 / 47.0 at 256 MiB, 150 / 128 at 512 MiB, 16-byte stores / whole lines)
constexpr int64_t kLinesFromBytes = 96ll << 20;
// tg_step_i8 at S = 16 / 25: non-temporal state loads in [from, to), where the Infinity Cache can still assist a pass but not hold it
// (S = 16, round 3 sweep, whole lines without / with them: 512 MiB 129.6 / 99.4 us, 1 GiB 257.6 / 230.0, 1.5 GiB 387.0 / 395.7,
// 2 GiB 515.5 / 537.3, 4 GiB 1023.5 / 1054.0 -- once the footprint is many times the cache the hint only costs)
// (S = 25, round 3 sweep, 16-byte stores / whole lines / whole lines + nt loads: 244 MiB 46.8 / 47.2 / 52.9 us, 488 MiB
// 135.4 / 129.9 / 99.0, 977 MiB 279.0 / 273.7 / 210.6, 1.46 GiB 428.5 / 439.6 / 464.4, 1.9 GiB 529.7 / 552.2 / 554.7,
// 3.8 GiB 1089 / 1152 / 1247: beyond 1.25 GiB the plain form is the best one again)
constexpr int64_t kNtLoadsFromBytes = 320ll << 20, kNtLoadsToBytes = 1280ll << 20;
// tg_step_i8 at S = 16 from kNtLoadsToBytes on: unused dynamic LDS, five workgroups per CU instead of eight (the kernel has no LDS
// of its own: 160 KB / 32 000 = 5; 2 GiB of states, dynamic LDS 0 / 8 / 14 / 20 / 26 / 34 KB: 516 / 516 / 515 / 514 / 504 / 506 us)
constexpr int kS16LdsPad = 32000;
// tg_step_i8 at S = 25 from kNtLoadsToBytes on: far beyond the caches FEWER resident workgroups stream better (each
// workgroup reads one 15.6 KB game: with three per CU instead of seven the HBM side sees fewer concurrent streams): unused
// dynamic LDS holds the kernel to three.  2 GiB of states, dynamic LDS 0 / 12 / 20 / 24 / 32 / 40 KB (7 / 6 / 5 / 4 / 3 / 3
// per CU): 614 / 617 / 597 / 588 / 574 / 572 us; two per CU: 751.  (BASELINE config 5's share, 61 MB: 15.0 / 15.1 / - /
// 16.1 / 16.1 -- there occupancy wins.)
constexpr int kS25LdsPad = 36000;  // (at S = 4 fewer resident wavefronts cost: 2 GiB, 24 / 32 / 48 KB of unused LDS: 841 / 942 / 1366 us against 772)
// tg_copy_i8 out of place, by the bytes both buffers hold together: non-temporal loads ABOVE the first, non-temporal loads
// and stores ABOVE the second (measured, tg_copy_i8 ping-pong between two buffers, plain / nt loads / nt loads + stores):
// 256 MiB 33 / 34 / 41 us, 384 MiB 67 / 49 / 61, 512 MiB 88 / 71 / 81, 768 MiB 131 / 127 / 120, 1 GiB 172 / 167 / 160.
// This kernel is the bench's copy ceiling: it has to be the best copy.
constexpr int64_t kCopyNtLoadsAboveBytes = 256ll << 20, kCopyNtStoresAboveBytes = 640ll << 20;
// tg_step_stream_i8 at S = 4: from this many games on the one-game-per-lane kernel (measured, four-lanes-per-game /
// one-game-per-lane, us per step with ready words and progress: 32 768 games 0.34 / 0.38, 49 152 0.38 / 0.39, 65 536
// 0.42 / 0.40, 98 304 0.58 / 0.47, 131 072 0.82 / 0.48, 262 144 1.97 / 0.90 before its token prefetch)
constexpr int64_t kLanesFrom = 57344;
// tg_step_tracked_i8 at S = 25: the sparse kernel from this many games on (placed by tools/tracked_time.py sweeps; measured,
// tg_step_i8 / full + count / sparse: 512 games 5.0 / 5.8 / 8.1 us, 1 024 6.1 / 7.1 / 8.3, 2 048 8.5 / 10.7 / 10.0, 4 096
// 14.9 / 17.0 / 13.1, 32 768 102 / - / 65, 139 264 (2 GiB) 574 / - / 303)
constexpr int64_t kTrackedSparse25 = 2048;

// ---- launches ----
// `blocks` workgroups as a grid, or the entry's "B too large"
int checked_grid(const char* fn, int64_t blocks, unsigned* grid) {
  if (blocks > 0x7fffffffLL) return fail(TG_ERR_INVALID, "%s: B too large", fn);
  *grid = static_cast<unsigned>(blocks);
  return TG_OK;
}

// One launch of the packed int16 kernels (tg_packed.h) or the row kernels (tg_rows.h): GPB games per workgroup, the
// actions in LDS tiles of up to ATILE.
template <int S, int TS, int MODE, bool... F>
int launch_packed(const char* fn, const tg::ApplyArgs& a, int flim, hipStream_t st) {
  using G = tg::PGeo<S, TS>;
  unsigned grid;
  if (int rc = checked_grid(fn, (a.B + G::GPB - 1) / G::GPB, &grid)) return rc;
  const int at = a.nact < G::ATILE ? a.nact : G::ATILE;
  return launch(fn, tg::packed_kernel<S, TS, MODE, F...>, grid, tg::kBlock, tg::packed_lds_bytes<S, TS, MODE>(at), st, a,
                flim, at);
}
template <int S, int TS, int MODE>
int launch_rows(const char* fn, const tg::ApplyArgs& a, int flim, hipStream_t st) {
  using G = tg::RGeo<S, TS>;
  unsigned grid;
  if (int rc = checked_grid(fn, (a.B + G::GPB - 1) / G::GPB, &grid)) return rc;
  const int at = a.nact < G::ATILE ? a.nact : G::ATILE;
  return launch(fn, tg::rows_kernel<S, TS, MODE>, grid, tg::kBlock, tg::rows_lds_bytes<S, TS, MODE>(at), st, a, flim, at);
}

// A workgroup's set-up (tile offsets, staging addresses) is a third of one game's work in the matrix-core kernels: every
// workgroup takes several games, as many workgroups as the chip holds at once, games split evenly.
template <auto K>
int launch_resident(const char* fn, const tg::ApplyArgs& a, int Rp, int ldsb, hipStream_t st) {
  const int64_t resident = static_cast<int64_t>(resident_per_cu<K>(ldsb)) * device_cu_count();
  return launch(fn, K, even_grid(a.B, resident), tg::kBlock, ldsb, st, a, Rp);
}
// The matrix-core kernels take the action count padded to a multiple of 32 and a K-step count as a template parameter:
// f(Rp, KS) with KS = 1 / 2 for exactly one / two steps of 32 actions, 0 for the general loop.
template <typename F>
int with_k_steps(int nact, F&& f) {
  const int Rp = (nact + 31) & ~31;
  if (Rp == 32) return f(Rp, std::integral_constant<int, 1>{});
  if (Rp == 64) return f(Rp, std::integral_constant<int, 2>{});
  return f(Rp, std::integral_constant<int, 0>{});
}
template <int S>
int launch_genf_mfma(const char* fn, const tg::ApplyArgs& a, hipStream_t st) {
  return with_k_steps(a.nact, [&](int Rp, auto ks) {
    return launch_resident<tg::genf_mfma_kernel<S, decltype(ks)::value>>(fn, a, Rp, tg::mfma_lds_bytes<S>(Rp), st);
  });
}
template <int S>
int launch_many_mfma(const char* fn, const tg::ApplyArgs& a, hipStream_t st) {
  return with_k_steps(a.nact, [&](int Rp, auto ks) {
    return launch_resident<tg::many_mfma_kernel<S, decltype(ks)::value>>(fn, a, Rp, tg::many_mfma_lds_bytes<S>(Rp), st);
  });
}

// The single step's variants by footprint band, each size's bands stated once (DIG = false: the packed form alone, A/B
// library only).  S = 4: plain / non-temporal loads / non-temporal loads with the token awaited first.
template <bool DIG>
int launch_s4_step(const char* fn, bool nt, bool tw, unsigned grid, hipStream_t st, const tg::S4StepArgs& sa) {
  if (tw) return launch(fn, tg::s4_step_kernel<true, true, DIG>, grid, tg::kBlock, 0, st, sa);
  if (nt) return launch(fn, tg::s4_step_kernel<true, false, DIG>, grid, tg::kBlock, 0, st, sa);
  return launch(fn, tg::s4_step_kernel<false, false, DIG>, grid, tg::kBlock, 0, st, sa);
}
// S = 16: 16-byte stores / whole lines / whole lines with non-temporal loads.
template <bool DIG>
int launch_s16_step(const char* fn, bool lines, bool nt, unsigned grid, int lds, hipStream_t st, const tg::ApplyArgs& a) {
  if (nt) return launch(fn, tg::s16_step_kernel<tg::STEP, true, true, DIG>, grid, tg::kBlock, lds, st, a);
  if (lines) return launch(fn, tg::s16_step_kernel<tg::STEP, true, false, DIG>, grid, tg::kBlock, lds, st, a);
  return launch(fn, tg::s16_step_kernel<tg::STEP, false, false, DIG>, grid, tg::kBlock, lds, st, a);
}

// ---- what the dispatch of tg_step_i8, tg_step_many_i8, tg_expand[_keyed]_i8 and tg_gen_from_factors_i8 shares ----
// The layout of the 16-byte-chunk kernels: states and strides aligned to 16 bytes (the generator reads no state).
bool aligned_layout(const tg::ApplyArgs& a, bool reads_state) {
  return (!reads_state || (aligned(a.in, 16) && a.in_stride % 16 == 0)) && aligned(a.out, 16) && a.out_stride % 16 == 0;
}
// S = 4 in registers (tg_s4.h): aligned layout, tokens as dwords, 32-bit game offsets inside a workgroup.
bool s4_layout(const tg::ApplyArgs& a, bool al) {
  return al && a.S == 4 && aligned(a.actions, 4) && a.in_stride < (1 << 20) && a.out_stride < (1 << 20);
}
int s4_grid(const char* fn, const tg::ApplyArgs& a, unsigned* grid) { return checked_grid(fn, (a.B * 4 + tg::kBlock - 1) / tg::kBlock, grid); }
// packed int16 path: exact while n * f^3 <= 32000 for every |factor| <= f (checked on device); n actions per result
int factor_limit(int64_t n) {
  int flim = 0;
  while (flim < 31 && static_cast<int64_t>(flim + 1) * (flim + 1) * (flim + 1) * n <= 32000) ++flim;
  return flim;
}
constexpr int kLatticeFactorLimit = 127;  // step_many's lattice form (tg_packed.h): u*v and 256*w must be representable in int16

// The tail every entry falls through to: the packed int16 teams (tg_packed.h) on the aligned layout, else the byte kernel.
template <int MODE>
int packed_or_slow(const char* fn, const tg::ApplyArgs& a, bool al, int flim, hipStream_t st) {
  if (al && flim >= 1) {
    // S=9: a game is only 46 chunks, so a wavefront takes FOUR games (teams of 16 lanes, 9 active, 6
    // chunks per lane): measured 0.48 of the HBM peak at 2^19 games against 0.43 (TS=32) and 0.29 (TS=64)
    if (a.S == 9) return launch_packed<9, 16, MODE>(fn, a, flim, st);
    if (a.S == 16) return launch_packed<16, 64, MODE>(fn, a, flim, st);
    if (a.S == 25) return launch_packed<25, 256, MODE>(fn, a, flim, st);
  }
  return launch(fn, tg::slow_kernel<MODE>, grid_for(a.B), tg::kBlock, 0, st, a);
}
// The same for the entries that accumulate over several actions (MANY, GENF).  Odd S, three actions and more: each lane
// owns whole rows (tg_rows.h); the LDS transposition is amortised over the actions.
template <int MODE>
int rows_packed_or_slow(const char* fn, const tg::ApplyArgs& a, bool al, int flim, hipStream_t st) {
  if (al && flim >= 1 && !TG_SWITCH("TG_NO_ROWS") && a.nact >= 3) {  // (A/B switch for measurements)
    if (a.S == 9) return launch_rows<9, 64, MODE>(fn, a, flim, st);
    if (a.S == 25) return launch_rows<25, 256, MODE>(fn, a, flim, st);
  }
  return packed_or_slow<MODE>(fn, a, al, flim, st);
}

// The fused generator's launch (tg_genfused.h) for one shape: twice as many workgroups as fit at once (two games each at
// B = 4096): the second wave of workgroups fills the chip as the first ones finish, which evens out the tail (measured:
// 40 -> 38 us).  TG_GF_WGS (A/B library) sets the workgroups per CU instead.
struct GenFused {
  const char* fn;
  tg::GenArgs ga;
  int Rp, wgs_override;
  bool lut_values;
  hipStream_t st;
};
template <auto K>
int launch_gen_fused(const GenFused& g, int ldsb) {
  const int64_t resident = g.wgs_override > 0 ? static_cast<int64_t>(g.wgs_override) * device_cu_count()
                                              : static_cast<int64_t>(resident_per_cu<K>(ldsb)) * device_cu_count() * 2;
  if (int rc = launch(g.fn, K, even_grid(g.ga.B, resident), tg::kBlock, ldsb, g.st, g.ga, g.Rp)) return rc;
  return 1;
}
template <int S, int KS, bool BAS, bool CHK>
int gen_fused_k(const GenFused& g) {
  const int ldsb = tg::genfused_lds_bytes<S>(g.Rp);
  if (g.ga.D.nthr == 2 && KS != 0) {  // the reference's three values: the specialised draw evaluation
    constexpr bool kLutShape = !BAS && !CHK;  // values exactly (-1,0,1): byte products by table lookup
    if (kLutShape && g.lut_values) return launch_gen_fused<tg::gen_fused_kernel<S, KS, BAS, 4, CHK, true, kLutShape>>(g, ldsb);
    return launch_gen_fused<tg::gen_fused_kernel<S, KS, BAS, 4, CHK, true>>(g, ldsb);
  }
  return launch_gen_fused<tg::gen_fused_kernel<S, KS, BAS, 4, CHK>>(g, ldsb);
}
template <int S, bool BAS, bool CHK>
int gen_fused_r(const GenFused& g) {
  if (g.Rp == 32) return gen_fused_k<S, 1, BAS, CHK>(g);
  if (g.Rp == 64) return gen_fused_k<S, 2, BAS, CHK>(g);
  return gen_fused_k<S, 0, BAS, CHK>(g);
}
template <int S>
int gen_fused_s(const GenFused& g, bool basis, bool in_range) {
  if (basis) return gen_fused_r<S, true, true>(g);
  if (!in_range) return gen_fused_r<S, false, true>(g);
  return gen_fused_r<S, false, false>(g);
}

}  // namespace

int tg_internal_gen_fused(int8_t* target, int8_t* actions, uint8_t* overflow, const int8_t* basis, int64_t B, int S,
                          int R, const tg::Dist& D, int shift, uint64_t seed, uint64_t gid0, int64_t stride,
                          hipStream_t st) {
  if (TG_SWITCH("TG_NO_FUSED_GEN") || TG_SWITCH("TG_NO_MFMA")) return 0;
  if (!(S == 9 || S == 16 || S == 25) || R > 256 || B == 0) return 0;
  if (!aligned(target, 16) || stride % 16 != 0) return 0;
  if (!basis) {  // the drawn values are the factors: u * v must fit a byte product, tokens must fit int8
    for (int t = 0; t < D.nv; ++t) {
      const int v = D.val[t];
      if (v > 11 || v < -11 || v + shift > 127 || v + shift < -128) return 0;
    }
  }
  GenFused g{"tg_gen_demos_i8", {target, actions, overflow, basis, B, stride, seed, gid0, R, shift, D}, (R + 31) & ~31, 0,
             false, st};
#ifdef TG_AB_SWITCHES
  g.ga.ablate = getenv("TG_GF_ABLATE") ? atoi(getenv("TG_GF_ABLATE")) : 0;
  g.wgs_override = getenv("TG_GF_WGS") ? atoi(getenv("TG_GF_WGS")) : 0;
#endif
  // without a basis the factors are the drawn values: when R * max|value|^3 <= 127 no entry of a target can leave
  // int8 (the reference's {-1,0,1} up to R = 127) and the tiles need no range tracking
  int fmax = 0;
  for (int t = 0; t < D.nv; ++t) fmax = D.val[t] > fmax ? D.val[t] : (-D.val[t] > fmax ? -D.val[t] : fmax);
  const bool in_range = !basis && static_cast<int64_t>(R) * fmax * fmax * fmax <= 127;
  g.lut_values = D.nv == 3 && D.val[0] == -1 && D.val[1] == 0 && D.val[2] == 1 && !TG_SWITCH("TG_GF_NO_LUT");
  if (S == 9) return gen_fused_s<9>(g, basis, in_range);
  if (S == 16) return gen_fused_s<16>(g, basis, in_range);
  return gen_fused_s<25>(g, basis, in_range);
}

// The dispatch of the apply entries: one function each, directly above its entry point, reading top to bottom as S, alignment,
// footprint -> kernel, grid, LDS (DESIGN.md section 3 has the table).  Their order here, and the order in which each names
// its kernels, is the order of the kernels in the code object.
static int apply_step(const char* fn, const tg::ApplyArgs& a, hipStream_t st);
static int apply_many(const char* fn, tg::ApplyArgs a, hipStream_t st);
static int apply_expand(const char* fn, tg::ApplyArgs a, hipStream_t st, bool* keys_fused);
static int apply_genf(const char* fn, const tg::ApplyArgs& a, hipStream_t st);
template <int MODE>
static int launch_apply(const char* fn, const tg::ApplyArgs& a, hipStream_t st, bool* keys_fused = nullptr) {
  if (a.B == 0) return TG_OK;
  switch (MODE) {
    case tg::STEP: return apply_step(fn, a, st);
    case tg::MANY: return apply_many(fn, a, st);
    case tg::EXPAND: return apply_expand(fn, a, st, keys_fused);
    default: return apply_genf(fn, a, st);
  }
}

extern "C" {

int tg_abi_version(void) { return TG_ABI_VERSION; }

int tg_debug_fallbacks(uint64_t* count) {
  if (!count) return fail(TG_ERR_INVALID, "tg_debug_fallbacks: null pointer");
  unsigned long long v = 0;
  hipError_t e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(tg::g_fallback_workgroups), sizeof(v));
  if (e != hipSuccess) return fail(TG_ERR_HIP, "tg_debug_fallbacks: %s", hipGetErrorString(e));
  *count = v;
  return TG_OK;
}
int tg_debug_handovers(uint64_t* count) {
  if (!count) return fail(TG_ERR_INVALID, "tg_debug_handovers: null pointer");
  unsigned long long v = 0;
  hipError_t e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(tg::g_many_handovers), sizeof(v));
  if (e != hipSuccess) return fail(TG_ERR_HIP, "tg_debug_handovers: %s", hipGetErrorString(e));
  *count = v;
  return TG_OK;
}
const char* tg_last_error(void) { return g_err; }

static std::atomic<unsigned> g_sweep{0};  // direction of the next tg_step_i8 sweep (sweep_index)

// tg_step_i8: one action per game.
static int apply_step(const char* fn, const tg::ApplyArgs& a, hipStream_t st) {
  using namespace tg;
  const bool al = aligned_layout(a, true);
  const int64_t B = a.B;
  unsigned grid;
  if (s4_layout(a, al)) {
    if (int rc = s4_grid(fn, a, &grid)) return rc;
    const int64_t bytes = B * a.in_stride;
    const bool nt = (bytes >= kS4NtLoadsFromBytes || TG_SWITCH("TG_S4_NT_LOADS"));
    const bool tw = nt && (bytes >= kS4TokenWaitBytes || TG_SWITCH("TG_S4_TOKEN_WAIT"));
    const S4StepArgs sa{a.in, a.out, a.actions, a.done, a.overflow, a.B, static_cast<uint32_t>(a.in_stride), a.shift,
                        s4_digits_limit(a.shift), bytes > kS4SweepAboveBytes ? a.sweep : 0};
#ifdef TG_AB_SWITCHES
    if (TG_SWITCH("TG_S4_NO_DIGITS")) return launch_s4_step<false>(fn, nt, tw, grid, st, sa);
#endif
    return launch_s4_step<true>(fn, nt, tw, grid, st, sa);
  }
  if (al && a.S == 16 && aligned(a.actions, 16) && !TG_SWITCH("TG_NO_S16_DIRECT")) {  // one wavefront per game (tg_s16.h)
    if (int rc = checked_grid(fn, (B + 3) / 4, &grid)) return rc;
    const int64_t bytes = B * a.in_stride;
    const bool nt = (bytes >= kNtLoadsFromBytes && bytes < kNtLoadsToBytes) || TG_SWITCH("TG_S16_NT_LOADS");  // (A/B switches: tests)
    const bool lines = bytes >= kLinesFromBytes || TG_SWITCH("TG_S16_LINES");  // (A/B switch: tests at small batches)
#ifdef TG_AB_SWITCHES
    if (TG_SWITCH("TG_S16_NO_DIGITS")) return launch_s16_step<false>(fn, lines, nt, grid, 0, st, a);
#endif
    // (the padding applies from kNtLoadsToBytes on, where the 16-byte-store form is never chosen)
    return launch_s16_step<true>(fn, lines, nt, grid, bytes >= kNtLoadsToBytes ? kS16LdsPad : 0, st, a);
  }
  if (al && a.S == 9 && a.shift >= -127 && a.shift <= 127 && !TG_SWITCH("TG_NO_S9_DIRECT")) {
    if (int rc = checked_grid(fn, (B + 15) / 16, &grid)) return rc;  // four wavefronts of four games
    return launch(fn, s9_step_kernel<STEP>, grid, kBlock, 0, st, a);
  }
  // (|shift| <= 127: factors within +-255, which the 32-bit redo of s25_step_kernel takes from its int16 tables)
  if (al && a.S == 25 && a.shift >= -127 && a.shift <= 127 && B <= 0x7fffffffLL && !TG_SWITCH("TG_NO_S25_DIRECT")) {
    // as at S=16: whole-line stores once the batch leaves the caches, non-temporal state loads beyond the Infinity
    // Cache (A/B switches: the variants at test sizes); beyond kNtLoadsToBytes the plain form again, with fewer waves
    const int64_t bytes = B * a.in_stride;
    const bool nt = (bytes >= kNtLoadsFromBytes && bytes < kNtLoadsToBytes) || TG_SWITCH("TG_S25_NT_LOADS");
    const bool lines = (bytes >= kLinesFromBytes && bytes < kNtLoadsToBytes) || TG_SWITCH("TG_S25_LINES");
    const int lds = bytes >= kNtLoadsToBytes ? kS25LdsPad : 0;
    grid = static_cast<unsigned>(B);
    if (nt) return launch(fn, s25_step_kernel<true, true>, grid, kBlock, lds, st, a);
    if (lines) return launch(fn, s25_step_kernel<true, false>, grid, kBlock, lds, st, a);
    return launch(fn, s25_step_kernel<false, false>, grid, kBlock, lds, st, a);
  }
  return packed_or_slow<STEP>(fn, a, al, factor_limit(1), st);
}

int tg_step_i8(const int8_t* state_in, int8_t* state_out, const int8_t* actions, uint8_t* done,
               uint8_t* overflow, int64_t B, int S, int64_t game_stride_bytes, int shift,
               tg_stream_t stream) {
  if (int rc = check_state("tg_step_i8", B, S, game_stride_bytes)) return rc;
  if (B && (!state_in || !state_out || !actions || !done))
    return fail(TG_ERR_INVALID, "tg_step_i8: null pointer");
  tg::ApplyArgs a{state_in, state_out, actions, done, nullptr, nullptr, overflow, B,
                  game_stride_bytes, game_stride_bytes, S, 1, shift};
  a.sweep = static_cast<int>(g_sweep.fetch_add(1u, std::memory_order_relaxed) & 1u);
  return launch_apply<tg::STEP>("tg_step_i8", a, static_cast<hipStream_t>(stream));
}

constexpr uint32_t kStreamWaitTicks = 100000000u;  // 1.0 s of s_memrealtime (100 MHz)

// The resident steppers (tg_stream.h), enumerated once.  A unit is one wavefront.  S = 4: 64 games per wavefront in the
// one-game-per-lane kernel (four workgroups per CU at 122 VGPRs), or NG games x 16 (NG = 1, 2: 8 workgroups per CU;
// NG = 4 / 8 -- 103 / 196 VGPRs, no more resident games than the lane kernel -- went in round 4).  S = 16 / 25: a
// wavefront per game.
struct StreamKernel {
  int games_per_unit;
  void (*kernel)(tg::StreamArgs);
  int (*per_cu)(int lds);  // workgroups of ITS kernel one CU of THIS device holds (resident_per_cu)
};
#define TG_STREAM_KERNEL(games_per_unit, k) {games_per_unit, k, resident_per_cu<k>}
static const StreamKernel kS4StreamLanes = TG_STREAM_KERNEL(64, tg::s4_stream_kernel_lanes);
static const StreamKernel kS4StreamTeams[] = {TG_STREAM_KERNEL(16, tg::s4_stream_kernel<1>), TG_STREAM_KERNEL(32, tg::s4_stream_kernel<2>)};
static const StreamKernel kS16Stream = TG_STREAM_KERNEL(1, tg::s16_stream_kernel), kS25Stream = TG_STREAM_KERNEL(1, tg::s25_stream_kernel);
#undef TG_STREAM_KERNEL

// Units of a streamed stepper this device keeps resident at once (from the occupancy of ITS kernel on THIS device).
static int64_t stream_units_resident(const StreamKernel& k) { return static_cast<int64_t>(device_cu_count()) * 4 * k.per_cu(0); }
static int64_t stream_games_resident(const StreamKernel& k) { return stream_units_resident(k) * k.games_per_unit; }

// S = 4: the largest batch any variant keeps resident.
static int64_t s4_stream_most() {
  int64_t most = stream_games_resident(kS4StreamLanes);
  for (const StreamKernel& k : kS4StreamTeams) most = stream_games_resident(k) > most ? stream_games_resident(k) : most;
  return most;
}

// S = 4: which kernel takes a resident batch of B games.  From kLanesFrom games on the one-game-per-lane kernel; below
// that, and beyond what it holds, the smallest NG whose units all fit.  Returns the kernel and its *units, or null when no
// variant keeps B games resident.
static const StreamKernel* s4_stream_variant(int64_t B, int64_t* units) {
  const int64_t lane_units = (B + 63) / 64;
  const bool lanes_ok = !TG_SWITCH("TG_STREAM_NO_LANES") && lane_units <= stream_units_resident(kS4StreamLanes);
  if (lanes_ok && (B >= kLanesFrom || TG_SWITCH("TG_STREAM_LANES"))) {
    *units = lane_units;
    return &kS4StreamLanes;
  }
  for (const StreamKernel& k : kS4StreamTeams) {
    const int64_t u = (B + k.games_per_unit - 1) / k.games_per_unit;
    if (u <= stream_units_resident(k)) {
      *units = u;
      return &k;
    }
  }
  return nullptr;
}

/* the largest batch tg_step_stream_i8 takes WITH ready words: every unit resident at once on the current device */
int tg_step_stream_capacity(int S, int64_t* games) {
  if (S != 4 && S != 16 && S != 25)
    return fail(TG_ERR_UNSUPPORTED, "tg_step_stream_capacity: S=%d (the streamed stepper is built for S=4, S=16 and S=25)", S);
  if (!games) return fail(TG_ERR_INVALID, "tg_step_stream_capacity: null pointer");
  *games = S == 4 ? s4_stream_most() : stream_games_resident(S == 16 ? kS16Stream : kS25Stream);  // (S = 16 / 25: a wavefront per game)
  return TG_OK;
}

/* units (wavefronts) and games per unit of tg_step_stream_i8 for a batch of B games, or a negative TG_ERR_* */
int tg_step_stream_layout(int64_t B, int S, int64_t* n_units, int* games_per_unit) {
  if (B < 0) return fail(TG_ERR_INVALID, "tg_step_stream_layout: B < 0");
  if (S != 4 && S != 16 && S != 25)
    return fail(TG_ERR_UNSUPPORTED, "tg_step_stream_layout: S=%d (the streamed stepper is built for S=4, S=16 and S=25)", S);
  if (S == 16 || S == 25) {  // one wavefront per game at any B (beyond tg_step_stream_capacity the units run in rounds: no ready words)
    if (n_units) *n_units = B;
    if (games_per_unit) *games_per_unit = 1;
    return TG_OK;
  }
  // S = 4: every wavefront must be resident at once when the producer waits for the whole batch
  int64_t units = 0;
  const StreamKernel* k = s4_stream_variant(B, &units);
  if (!k)
    return fail(TG_ERR_UNSUPPORTED, "tg_step_stream_layout: B=%lld exceeds the %lld games this device keeps resident at once",
                (long long)B, (long long)s4_stream_most());
  if (n_units) *n_units = units;
  if (games_per_unit) *games_per_unit = k->games_per_unit;
  return TG_OK;
}

int tg_step_stream_i8(int8_t* state, const int8_t* actions, uint8_t* done, uint8_t* overflow, const uint32_t* ready,
                      uint32_t* progress, uint32_t* status, int64_t B, int S, int K, int64_t game_stride_bytes, int shift,
                      tg_stream_t stream) {
  const char* fn = "tg_step_stream_i8";
  if (int rc = check_state(fn, B, S, game_stride_bytes)) return rc;
  if (K < 1 || K > (1 << 24)) return fail(TG_ERR_INVALID, "%s: K=%d outside [1,2^24]", fn, K);
  if (B == 0) return TG_OK;
  if (!state || !actions || !done) return fail(TG_ERR_INVALID, "%s: null pointer", fn);
  if (S != 4 && S != 16 && S != 25)
    return fail(TG_ERR_UNSUPPORTED, "%s: S=%d (the streamed stepper is built for S=4, S=16 and S=25)", fn, S);
  int64_t units = B;  // S = 16 / 25: one wavefront per game
  const StreamKernel* k = S == 16 ? &kS16Stream : &kS25Stream;
  if (S == 4) {
    k = s4_stream_variant(B, &units);
    if (!k) {
      // beyond what the device keeps resident: without ready words no producer can be waiting for the whole batch, so the
      // units (64 games each, the one-game-per-lane kernel) simply run in rounds, every wavefront taking its games
      // through all K steps.  Always the lane kernel, whatever the A/B switches say: they choose among RESIDENT layouts only,
      // and a caller sizes progress for the rounds by this fixed layout (ops.step_stream: one word per 64 games)
      if (ready) return tg_step_stream_layout(B, S, nullptr, nullptr);  // (fails with the message that names the capacity)
      k = &kS4StreamLanes;
      units = (B + k->games_per_unit - 1) / k->games_per_unit;
    }
  }
  // S = 16 / 25 beyond the resident batch run in rounds as well -- and with ready words a producer that releases step k+1
  // only once EVERY unit has published k would never see the later rounds start (each would wait out its whole bound and
  // leave the games at different steps): refused, as tg_step_stream_layout refuses it at S = 4
  if (ready && S != 4 && units > stream_units_resident(*k))
    return fail(TG_ERR_UNSUPPORTED, "%s: B=%lld exceeds the %lld games of S=%d this device keeps resident at once; with ready "
                "words every unit must be resident (tg_step_stream_capacity) -- pass ready = NULL to run the batch in rounds",
                fn, (long long)B, (long long)stream_units_resident(*k), S);
  // (a single game has no stride to speak of; S = 25 reads the 16-byte chunk that holds the game's last byte: it lies inside
  // the last game's final aligned 16 bytes, and only the game's own 9 bytes of it are ever written)
  if (!aligned(state, 16) || (game_stride_bytes % 16 != 0 && B > 1) || !(S == 16 ? aligned(actions, 16) : aligned(actions, 4)) ||
      B * game_stride_bytes > 0x7fffffffLL || static_cast<int64_t>(K) * B > 0x7fffffffLL ||
      static_cast<unsigned>(shift + 127) > 254u)
    return fail(TG_ERR_UNSUPPORTED, "%s: needs 16-byte aligned states, aligned actions (4 bytes at S=4, 16 at S=16), B*stride and K*B < 2^31, |shift| <= 127", fn);
  if (!aligned(ready, 4) || !aligned(progress, 4))
    return fail(TG_ERR_INVALID, "%s: ready / progress must be 4-byte aligned", fn);
  tg::StreamArgs a{state, actions, done, overflow, ready, progress, status, B, game_stride_bytes, K, shift, kStreamWaitTicks};
  const unsigned grid = static_cast<unsigned>((units + 3) / 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return launch(fn, k->kernel, grid, tg::kBlock, 0, st, a);
}

int tg_step_tracked_i8(int8_t* state, const int8_t* actions, int32_t* nnz, uint8_t* done, uint8_t* overflow, int64_t B,
                       int S, int64_t game_stride_bytes, int shift, tg_stream_t stream) {
  const char* fn = "tg_step_tracked_i8";
  if (int rc = check_state(fn, B, S, game_stride_bytes)) return rc;
  if (B == 0) return TG_OK;
  if (!state || !actions || !nnz || !done) return fail(TG_ERR_INVALID, "%s: null pointer", fn);
  if (!aligned(nnz, 4)) return fail(TG_ERR_INVALID, "%s: nnz must be 4-byte aligned", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (S == 25 && aligned(state, 16) && game_stride_bytes % 16 == 0 && static_cast<unsigned>(shift + 127) <= 254u &&
      B <= 0x7fffffffLL) {
    // sparse kernel from kTrackedSparse25 games on, fewer: the full step's kernel with the count updated (one round trip
    // instead of two)
    tg::ApplyArgs a{state, state, actions, done, nnz, nullptr, overflow, B, game_stride_bytes, game_stride_bytes, S, 1, shift};
    if ((B >= kTrackedSparse25 || TG_SWITCH("TG_TRACKED_SPARSE")) && !TG_SWITCH("TG_TRACKED_FULL"))
      return launch(fn, tg::s25_tracked_kernel, static_cast<unsigned>((B + 3) / 4), tg::kBlock, 0, st, a, nnz);
    return launch(fn, tg::s25_step_kernel<false, false, true>, static_cast<unsigned>(B), tg::kBlock, 0, st, a);
  }
  if (S == 16 && aligned(state, 16) && aligned(actions, 16) && game_stride_bytes % 16 == 0 && B <= 0x7fffffffLL) {
    // The sparse kernel pays two dependent round trips for ~28 % of the lines (measured, tg_step_i8 / this: 2 048 games 3.3 /
    // 3.5 us, 8 192 5.8 / 6.5, 12 288 11.1 / 8.4, 32 768 26.7 / 16.6, 131 072 99.7 / 73.7, 2 GiB 504 / 296).  The full step's
    // kernel with the count added was no better at the small end (3.8 / 6.6 us): one kernel for every batch.
    tg::ApplyArgs a{state, state, actions, done, nullptr, nullptr, overflow, B, game_stride_bytes, game_stride_bytes, S, 1, shift};
    return launch(fn, tg::s16_tracked_kernel, static_cast<unsigned>((B + 3) / 4), tg::kBlock, 0, st, a, nnz);
  }
  // other sizes and layouts: the full step, then the count (two launches inside this call; same results)
  if (int rc = tg_step_i8(state, state, actions, done, overflow, B, S, game_stride_bytes, shift, stream)) return rc;
  return tg_done_i8(state, done, nnz, B, S, game_stride_bytes, stream);
}

// tg_step_many_i8: K actions per game, the first step that reaches zero.
static int apply_many(const char* fn, tg::ApplyArgs a, hipStream_t st) {
  using namespace tg;
  const bool al = aligned_layout(a, true);
  unsigned grid;
  if (s4_layout(a, al)) {
    if (int rc = s4_grid(fn, a, &grid)) return rc;
    return launch(fn, s4_kernel<MANY>, grid, kBlock, 0, st, a);
  }
  // K fused steps: the final state is one accumulation on the matrix cores; games it cannot certify (a step
  // may have left int8, or the zero state was reached before the last step) are flagged through done_step and
  // redone by the lattice kernels below, launched with only_flagged (tg_mfma.h)
  // Where it pays (measured, tools/sweep_many.py): the per-game set-up (transposed factors, input image,
  // per-action scalars, verdict) outweighs the lattice kernels' K S^3 MACs only for long action lists; beyond
  // K = 127 the overflow bound cannot certify the reference's {-1,0,1} factors any more.
  const bool many_always = TG_SWITCH("TG_MFMA_MANY_ALWAYS");  // tests: every eligible shape
  const bool pays = (a.S == 25 && a.nact >= 3) || (a.S == 16 && a.nact >= 20) || (a.S == 9 && a.nact >= 30);  // up to 256
  // (tools/many_k_sweep.py, profiles/r02_many_k_sweep.txt: the matrix-core pass costs ~44.5 us at S=25 B=4096 and ~41 us at
  //  S=16 B=8192 whatever K is -- staging, the tiles' fixed part, verdict; the lattice kernels 30 / 50 / 52 us at K = 2 / 3 / 4
  //  (S=25), 24 / 35 / 41 / 45 / 55 at K = 8 / 16 / 20 / 24 / 32 (S=16), 58 / 82 / 106 against 88 / 96 / 99 at K = 12 / 24 / 32 (S=9))
  if (al && a.nact <= 256 && !TG_SWITCH("TG_NO_MFMA") && (a.S == 9 || a.S == 16 || a.S == 25) && (pays || many_always)) {
    const int rc = a.S == 9 ? launch_many_mfma<9>(fn, a, st) : a.S == 16 ? launch_many_mfma<16>(fn, a, st)
                                                                         : launch_many_mfma<25>(fn, a, st);
    if (rc) return rc;
    a.only_flagged = 1;
  }
  return rows_packed_or_slow<MANY>(fn, a, al, kLatticeFactorLimit, st);
}

int tg_step_many_i8(const int8_t* state_in, int8_t* state_out, const int8_t* actions,
                    int32_t* done_step, uint8_t* overflow, int64_t B, int S, int K,
                    int64_t game_stride_bytes, int shift, tg_stream_t stream) {
  if (int rc = check_state("tg_step_many_i8", B, S, game_stride_bytes)) return rc;
  if (K < 1 || K > TG_MAX_ACTIONS)
    return fail(TG_ERR_INVALID, "tg_step_many_i8: K=%d outside [1,%d]", K, TG_MAX_ACTIONS);
  if (B && (!state_in || !state_out || !actions || !done_step))
    return fail(TG_ERR_INVALID, "tg_step_many_i8: null pointer");
  tg::ApplyArgs a{state_in, state_out, actions, nullptr, done_step, nullptr, overflow, B,
                  game_stride_bytes, game_stride_bytes, S, K, shift};
  return launch_apply<tg::MANY>("tg_step_many_i8", a, static_cast<hipStream_t>(stream));
}

// tg_expand_i8 / tg_expand_keyed_i8: k children per game.  *keys_fused = the launch formed the keys as well.
static int apply_expand(const char* fn, tg::ApplyArgs a, hipStream_t st, bool* keys_fused) {
  using namespace tg;
  const bool al = aligned_layout(a, true);
  const int64_t B = a.B;
  unsigned grid;
  a.stream_out = (B * a.nact * a.out_stride >= kStreamOutBytes || TG_SWITCH("TG_EXPAND_NT")) && !TG_SWITCH("TG_EXPAND_NO_NT");
  if (s4_layout(a, al)) {
    if (int rc = s4_grid(fn, a, &grid)) return rc;
    if (a.nact <= 64 && a.out_stride * 64 < (1 << 24)) {  // 64 / k parents per workgroup, a lane per (child, slice)
      const int PB = 64 / a.nact, recip = (65536 + a.nact - 1) / a.nact;
      if (int rc = checked_grid(fn, (B + PB - 1) / PB, &grid)) return rc;
      if (a.keys) {
        if (keys_fused) *keys_fused = true;
        if (a.stream_out) return launch(fn, s4_expand_kernel<true, true>, grid, kBlock, 0, st, a, PB, recip);
        return launch(fn, s4_expand_kernel<false, true>, grid, kBlock, 0, st, a, PB, recip);
      }
      if (a.stream_out) return launch(fn, s4_expand_kernel<true>, grid, kBlock, 0, st, a, PB, recip);
      return launch(fn, s4_expand_kernel<false>, grid, kBlock, 0, st, a, PB, recip);
    }
    return launch(fn, s4_kernel<EXPAND>, grid, kBlock, 0, st, a);
  }
  const int flim = factor_limit(1);
  // S = 9: one 16-lane team per child (s9_step_kernel<EXPAND>): 80 -> 61 us at B = 32 768, k = 8
  if (al && a.S == 9 && a.shift >= -127 && a.shift <= 127 && !TG_SWITCH("TG_NO_S9_DIRECT") && B * a.nact < 0x7fffffffLL)
    return launch(fn, s9_step_kernel<EXPAND>, (unsigned)((B * a.nact + 15) / 16), kBlock, 0, st, a);
  if (al && flim >= 1) {
    if (a.S == 9) return launch_packed<9, 16, EXPAND>(fn, a, flim, st);  // (as in the tail; named ahead of the variants below)
    // S = 16: children of 128 MiB and more leave by non-temporal stores; with keys asked for (tg_expand_keyed_i8) they
    // are formed in the same launch while a child is in registers
    if (a.S == 16 && a.keys) {
      if (keys_fused) *keys_fused = true;
      if (a.stream_out) return launch_packed<16, 64, EXPAND, true, true>(fn, a, flim, st);
      return launch_packed<16, 64, EXPAND, false, true>(fn, a, flim, st);
    }
    if (a.S == 16 && a.stream_out) return launch_packed<16, 64, EXPAND, true>(fn, a, flim, st);
    if (a.S == 25 && a.keys) {  // tg_expand_keyed_i8 at S = 25: the keys from the same launch (a workgroup per parent)
      if (int rc = checked_grid(fn, B, &grid)) return rc;
      const int at = a.nact < PGeo<25, 256>::ATILE ? a.nact : PGeo<25, 256>::ATILE;
      if (keys_fused) *keys_fused = true;
      return launch(fn, packed_kernel<25, 256, EXPAND, false, true>, grid, kBlock, packed_lds_bytes<25, 256, EXPAND, true>(at),
                    st, a, flim, at);
    }
  }
  return packed_or_slow<EXPAND>(fn, a, al, flim, st);
}

static int expand_common(const char* fn, const int8_t* state_in, int8_t* state_out, const int8_t* actions, uint8_t* done,
                         uint8_t* changed, uint8_t* overflow, uint64_t* keys_out, int64_t B, int S, int k,
                         int64_t in_stride_bytes, int64_t out_stride_bytes, int shift, tg_stream_t stream) {
  if (int rc = check_state(fn, B, S, in_stride_bytes)) return rc;
  if (int rc = check_state(fn, B, S, out_stride_bytes)) return rc;
  if (k < 1 || k > TG_MAX_ACTIONS) return fail(TG_ERR_INVALID, "%s: k=%d outside [1,%d]", fn, k, TG_MAX_ACTIONS);
  if (B && (!state_in || !state_out || !actions || !done)) return fail(TG_ERR_INVALID, "%s: null pointer", fn);
  if (B && state_in == state_out) return fail(TG_ERR_INVALID, "%s: in-place expansion is not defined", fn);
  if (!aligned(keys_out, 8)) return fail(TG_ERR_INVALID, "%s: keys_out must be 8-byte aligned", fn);
  tg::ApplyArgs a{state_in, state_out, actions, done, nullptr, changed, overflow, B,
                  in_stride_bytes, out_stride_bytes, S, k, shift};
  a.keys = keys_out;
  bool fused = false;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = launch_apply<tg::EXPAND>(fn, a, st, &fused)) return rc;
  // kernel families that do not hash the children while they hold them: one pass of the key kernel over the children
  // just written (S = 4, the shape MCTS expansion runs at in the reference, is fused)
  if (keys_out && B && !fused) return tg_internal_hash(state_out, keys_out, B * k, S, out_stride_bytes, st);
  return TG_OK;
}

int tg_expand_i8(const int8_t* state_in, int8_t* state_out, const int8_t* actions, uint8_t* done,
                 uint8_t* changed, uint8_t* overflow, int64_t B, int S, int k,
                 int64_t in_stride_bytes, int64_t out_stride_bytes, int shift, tg_stream_t stream) {
  return expand_common("tg_expand_i8", state_in, state_out, actions, done, changed, overflow, nullptr, B, S, k,
                       in_stride_bytes, out_stride_bytes, shift, stream);
}

int tg_expand_keyed_i8(const int8_t* state_in, int8_t* state_out, const int8_t* actions, uint8_t* done,
                       uint8_t* changed, uint8_t* overflow, uint64_t* keys_out, int64_t B, int S, int k,
                       int64_t in_stride_bytes, int64_t out_stride_bytes, int shift, tg_stream_t stream) {
  return expand_common("tg_expand_keyed_i8", state_in, state_out, actions, done, changed, overflow, keys_out, B, S, k,
                       in_stride_bytes, out_stride_bytes, shift, stream);
}

int tg_step_emit(int8_t* ring, const int8_t* actions, void* out, float* scalars, uint8_t* done, uint8_t* overflow,
                 int out_dtype, int64_t B, int S, int T, int head_slot, float t_step, int64_t frame_stride_bytes,
                 int64_t game_stride_bytes, int shift, tg_stream_t stream) {
  const char* fn = "tg_step_emit";
  if (int rc = check_state(fn, B, S, frame_stride_bytes)) return rc;
  if (T < 1 || T > 64 || head_slot < 0 || head_slot >= T)
    return fail(TG_ERR_INVALID, "%s: need 1 <= T <= 64 and 0 <= head_slot < T", fn);
  if (game_stride_bytes < static_cast<int64_t>(T - 1) * frame_stride_bytes + static_cast<int64_t>(S) * S * S)
    return fail(TG_ERR_INVALID, "%s: game_stride_bytes too small for T frames", fn);
  if (out_dtype < 0 || out_dtype > 2) return fail(TG_ERR_INVALID, "%s: out_dtype must be 0 (f32), 1 (f16) or 2 (bf16)", fn);
  if (B == 0) return TG_OK;
  if (!ring || !actions || !out || !done) return fail(TG_ERR_INVALID, "%s: null pointer", fn);
  if (!aligned(out, 16)) return fail(TG_ERR_INVALID, "%s: out must be 16-byte aligned", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nxt = head_slot + 1 < T ? head_slot + 1 : 0;
  // One launch while the model input stays in the caches (65 536 games, T = 4: 9.9 us against 14.3 for step + frames in
  // float16, 14.4 against 18.4 in float32).  Once the output streams to HBM the frames kernel's fully coalesced
  // 16-byte-per-thread write stream wins over the fused kernel's 64-byte team runs (2^20 games: 243 against 185 us,
  // 350 against 320), so from kStreamOutBytes of output on this entry is the two launches.
  const int64_t out_bytes = B * T * 64 * (out_dtype ? 2 : 4);
  const bool fused = S == 4 && aligned(ring, 4) && frame_stride_bytes % 4 == 0 &&
                     game_stride_bytes % 4 == 0 && aligned(actions, 4) && static_cast<unsigned>(shift + 127) <= 254u &&
                     (out_bytes < tg::kStreamOutBytes || TG_SWITCH("TG_STEP_EMIT_FUSED"));
  if (fused) {
    tg::StepEmitArgs a{ring, actions, out, scalars, done, overflow, B, frame_stride_bytes, game_stride_bytes, T, head_slot, shift, t_step};
    const int64_t blocks = (B * 4 + tg::kBlock - 1) / tg::kBlock;
    if (blocks > 0x7fffffffLL) return fail(TG_ERR_INVALID, "%s: B too large", fn);
    const bool nt = out_bytes >= tg::kStreamOutBytes || TG_SWITCH("TG_EMIT_NT");  // (A/B library only, see above)
    const unsigned grid = static_cast<unsigned>(blocks);
    return with_out_type(out_dtype, [&](auto t) {
      using OutT = decltype(t);
      if (nt) return launch(fn, tg::s4_step_emit_kernel<OutT, true>, grid, tg::kBlock, 0, st, a);
      return launch(fn, tg::s4_step_emit_kernel<OutT, false>, grid, tg::kBlock, 0, st, a);
    });
  }
  // S = 16 while the output stays in the caches: one launch (s16_step_emit_kernel)
  const int64_t out_bytes16 = B * T * 4096 * (out_dtype ? 2 : 4);
  const bool fused16 = S == 16 && aligned(ring, 16) && frame_stride_bytes % 16 == 0 && game_stride_bytes % 16 == 0 && aligned(actions, 16) &&
                       (out_bytes16 < tg::kStreamOutBytes || TG_SWITCH("TG_STEP_EMIT_FUSED"));
  if (fused16) {
    tg::StepEmitArgs a{ring, actions, out, scalars, done, overflow, B, frame_stride_bytes, game_stride_bytes, T, head_slot, shift, t_step};
    const int64_t blocks = (B + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail(TG_ERR_INVALID, "%s: B too large", fn);
    const bool nt = out_bytes16 >= tg::kStreamOutBytes;
    const unsigned grid = static_cast<unsigned>(blocks);
    return with_out_type(out_dtype, [&](auto t) {
      using OutT = decltype(t);
      if (nt) return launch(fn, tg::s16_step_emit_kernel<OutT, true>, grid, tg::kBlock, 0, st, a);
      return launch(fn, tg::s16_step_emit_kernel<OutT, false>, grid, tg::kBlock, 0, st, a);
    });
  }
  // other sizes and layouts: the step into the next ring slot, then the frames (two launches inside this call)
  if (int rc = tg_step_i8(ring + head_slot * frame_stride_bytes, ring + nxt * frame_stride_bytes, actions, done, overflow, B, S,
                          game_stride_bytes, shift, stream))
    return rc;
  return tg_emit_frames(ring, out, scalars, out_dtype, B, S, T, nxt, t_step, frame_stride_bytes, game_stride_bytes, stream);
}

// tg_gen_from_factors_i8: the sum of R rank-1 terms per game.
static int apply_genf(const char* fn, const tg::ApplyArgs& a, hipStream_t st) {
  using namespace tg;
  const bool al = aligned_layout(a, false);
  unsigned grid;
  if (s4_layout(a, al)) {
    if (int rc = s4_grid(fn, a, &grid)) return rc;
    return launch(fn, s4_kernel<GENF>, grid, kBlock, 0, st, a);
  }
  // the accumulation over R is a dense contraction: matrix cores (tg_mfma.h); u*v must fit int8 (checked
  // on device, per game), the transposed factors of one game must fit LDS
  if (al && a.nact <= 256 && !TG_SWITCH("TG_NO_MFMA")) {  // (A/B switch for measurements)
    if (a.S == 9) return launch_genf_mfma<9>(fn, a, st);
    if (a.S == 16) return launch_genf_mfma<16>(fn, a, st);
    if (a.S == 25) return launch_genf_mfma<25>(fn, a, st);
  }
  return rows_packed_or_slow<GENF>(fn, a, al, factor_limit(a.nact), st);
}

int tg_gen_from_factors_i8(const int8_t* actions, int8_t* target_out, uint8_t* overflow, int64_t B,
                           int S, int R, int64_t game_stride_bytes, int shift, tg_stream_t stream) {
  if (int rc = check_state("tg_gen_from_factors_i8", B, S, game_stride_bytes)) return rc;
  if (R < 1 || R > TG_MAX_ACTIONS)
    return fail(TG_ERR_INVALID, "tg_gen_from_factors_i8: R=%d outside [1,%d]", R, TG_MAX_ACTIONS);
  if (B && (!actions || !target_out)) return fail(TG_ERR_INVALID, "tg_gen_from_factors_i8: null pointer");
  tg::ApplyArgs a{nullptr, target_out, actions, nullptr, nullptr, nullptr, overflow, B,
                  game_stride_bytes, game_stride_bytes, S, R, shift};
  return launch_apply<tg::GENF>("tg_gen_from_factors_i8", a, static_cast<hipStream_t>(stream));
}

int tg_copy_i8(const int8_t* state_in, int8_t* state_out, int64_t B, int S, int64_t in_stride_bytes,
               int64_t out_stride_bytes, tg_stream_t stream) {
  if (int rc = check_state("tg_copy_i8", B, S, in_stride_bytes)) return rc;
  if (int rc = check_state("tg_copy_i8", B, S, out_stride_bytes)) return rc;
  if (B == 0) return TG_OK;
  if (!state_in || !state_out) return fail(TG_ERR_INVALID, "tg_copy_i8: null pointer");
  if (state_in == state_out) return in_stride_bytes == out_stride_bytes ? TG_OK : fail(TG_ERR_INVALID, "tg_copy_i8: in place with different strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = S * S * S;
  auto copy = [&](auto kernel, unsigned grid, auto... x) {
    return launch("tg_copy_i8", kernel, grid, tg::kBlock, 0, st, state_in, state_out, B, x..., in_stride_bytes,
                  out_stride_bytes);
  };
  if (aligned(state_in, 16) && aligned(state_out, 16) && in_stride_bytes % 16 == 0 && out_stride_bytes % 16 == 0) {
    const int nchunk = (N + 15) / 16;
    int sh = -1;
    for (int t = 0; t < 12; ++t)
      if ((1 << t) == nchunk) sh = t;
    const int64_t blocks = (B * nchunk + tg::kBlock - 1) / tg::kBlock;
    if (blocks > 0x7fffffffLL) return fail(TG_ERR_INVALID, "tg_copy_i8: B too large");
    // Out of place, by the bytes both buffers hold together (kCopyNtLoadsAboveBytes, kCopyNtStoresAboveBytes)
    const int64_t both = state_in == state_out ? 0 : B * (in_stride_bytes + out_stride_bytes);
    const unsigned grid = static_cast<unsigned>(blocks);
    if (TG_SWITCH("TG_COPY_PLAIN")) return copy(tg::copy_kernel<0>, grid, nchunk, sh, N % 16);
    else if (both > kCopyNtStoresAboveBytes || TG_SWITCH("TG_COPY_NT2")) return copy(tg::copy_kernel<2>, grid, nchunk, sh, N % 16);
    else if (both > kCopyNtLoadsAboveBytes || TG_SWITCH("TG_COPY_NT1")) return copy(tg::copy_kernel<1>, grid, nchunk, sh, N % 16);
    else return copy(tg::copy_kernel<0>, grid, nchunk, sh, N % 16);
  }
  return copy(tg::copy_bytes_kernel, grid_for(B, 65536), N);
}

int tg_done_i8(const int8_t* state, uint8_t* done, int32_t* nnz, int64_t B, int S,
               int64_t game_stride_bytes, tg_stream_t stream) {
  if (int rc = check_state("tg_done_i8", B, S, game_stride_bytes)) return rc;
  if (B == 0) return TG_OK;
  if (!state || !done) return fail(TG_ERR_INVALID, "tg_done_i8: null pointer");
  const int vec16 = aligned(state, 16) && game_stride_bytes % 16 == 0;
  const int N = S * S * S;
  int lpg = 1;
  // lanes per game: up to four 16-byte chunks per lane for games of 16 chunks and more (S=9: 16 lanes x 3 chunks, four
  // games per wavefront -- with a wavefront per game 46 lanes did one load each and the launch was latency-bound:
  // 12-16 us for 24 MB), one chunk per lane for the small ones (S=4: 4 lanes)
  while (lpg < 64 && lpg * 16 * (N >= 256 ? 4 : 1) < N) lpg <<= 1;
  const int64_t blocks = (B * lpg + tg::kBlock - 1) / tg::kBlock;
  return launch("tg_done_i8", tg::done_kernel, grid_for(blocks, 8192), tg::kBlock, 0, static_cast<hipStream_t>(stream),
                state, done, nnz, B, N, game_stride_bytes, vec16, lpg);
}

int tg_reset_matmul_i8(int8_t* state_out, int64_t B, int n, int64_t game_stride_bytes,
                       tg_stream_t stream) {
  if (n < 1 || n * n > TG_MAX_S) return fail(TG_ERR_INVALID, "tg_reset_matmul_i8: n=%d, need 1 <= n*n <= %d", n, TG_MAX_S);
  if (int rc = check_state("tg_reset_matmul_i8", B, n * n, game_stride_bytes)) return rc;
  if (B == 0) return TG_OK;
  if (!state_out) return fail(TG_ERR_INVALID, "tg_reset_matmul_i8: null pointer");
  const int S = n * n, N = S * S * S;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char* fn = "tg_reset_matmul_i8";
  if (int rc = launch(fn, tg::matmul_template_kernel, (N + tg::kBlock - 1) / tg::kBlock, tg::kBlock, 0, st, state_out, n))
    return rc;
  if (B == 1) return TG_OK;
  const int vec16 = aligned(state_out, 16) && game_stride_bytes % 16 == 0;
  const int64_t work = (B - 1) * (vec16 ? (N + 15) / 16 : N);
  return launch(fn, tg::broadcast_kernel, grid_for((work + tg::kBlock - 1) / tg::kBlock, 8192), tg::kBlock, 0, st,
                state_out, state_out, (int64_t)1, B, N, game_stride_bytes, vec16);
}

int tg_reset_broadcast_i8(const int8_t* start, int8_t* state_out, int64_t B, int S,
                          int64_t game_stride_bytes, tg_stream_t stream) {
  if (int rc = check_state("tg_reset_broadcast_i8", B, S, game_stride_bytes)) return rc;
  if (B == 0) return TG_OK;
  if (!start || !state_out) return fail(TG_ERR_INVALID, "tg_reset_broadcast_i8: null pointer");
  const int vec16 = aligned(start, 16) && aligned(state_out, 16) && game_stride_bytes % 16 == 0;
  const int N = S * S * S;
  const int64_t work = B * (vec16 ? (N + 15) / 16 : N);
  const int64_t blocks = (work + tg::kBlock - 1) / tg::kBlock;
  return launch("tg_reset_broadcast_i8", tg::broadcast_kernel, grid_for(blocks, 8192), tg::kBlock, 0,
                static_cast<hipStream_t>(stream), start, state_out, (int64_t)0, B, N, game_stride_bytes, vec16);
}

}  // extern "C"
