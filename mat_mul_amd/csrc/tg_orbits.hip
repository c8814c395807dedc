// The canonical form of a factorisation modulo a set of symmetries of its target, and the check that the set fixes a
// target (include/tensor_game_orbits.h).  gfx950 only; part of libtensorgame.so.
//
// orbit_canon_kernel, one (list, slice of the set) per workgroup at a time: NT = 64 threads (a wavefront) while K <= 64,
// NT = 256 above, so thread t owns term t in the per-term phases, as in tg_solutions.hip.  The list's L * 3S token bytes
// are staged into LDS once (the pristine image) and verified once, by the verifier tg_solutions.hip uses
// (tg_sol_phases.h).  Then, per element g of the slice:
//   row        the 3S+1 bytes of g are checked and decoded into an LDS table, entry m*S + a = the source position
//              rho[m]*S + pi_m[a] inside a term | the sign bit (two tables, used in turn: one barrier per g);
//   gather     one thread per factor of g.X (3L of them) walks the table, finds the first non-zero value, and writes the
//              NORMALISED factor straight into the sort keys: P = 3S rounded up to 8 bytes per term, every byte with
//              its sign bit flipped and every 8 bytes reversed, so unsigned 8-byte compares order the values as signed.
//              g.X itself and its normalised image are never stored;
//   order      the rank sort and merge tg_solutions.hip calls too (tg_sol_phases.h), as are the term signs and the key;
//   emit       the kept terms go from the keys into the candidate image (negating w where the run's sum is negative);
//   compare    every thread compares 16-byte chunks of the candidate and the running best and reports its first
//              differing byte; the workgroup's minimum decides.  The smaller image stays by swapping two pointers.
// Both images are zero behind what was written into them (the extent is tracked, so nothing is cleared per g while the
// rank does not change, which it cannot for signed permutations).
// LDS budget, dynamic: the pristine image, the keys (K * max(P, 32) bytes; the verifier's w rows live there first) and
// the two candidate images, each K * 3S rounded up to 16: 4 * 24 KiB = 96 KiB at K = 256, S = 32, above the 64 KiB a
// kernel gets by default, hence the opt-in (lds_opt_in); 39 KiB at K = 128, S = 25.  Static: 3.5 KiB.
//
// Decomposition.  With M lists that do not fill the device the set is cut into NS slices of `per` elements and the
// grid is M * NS workgroups; each writes its slice's winner (image, rank, which, count, flags, residual) into the
// caller's workspace, and orbit_reduce_kernel, a wavefront per list, takes the smallest winner in slice order (so `which`
// is the smallest index) and adds the counts of the slices that attain it.  With NS = 1 the first kernel writes the
// outputs itself.  Either way an output is a function of the list and the set: the minimum, the smallest index of it
// and the number of elements attaining it do not depend on where the set is cut.
// A bad row of the set is found by whichever workgroup walks it (every list walks every row, sliced or not, and a list
// that is bad for another reason still scans its rows), so TG_ORBIT_BAD_GROUP reaches every list without a pass of its
// own.  The one atomic is the OR of the sticky bits into *status.  No floating point.
//
// orbit_fixes_kernel, one target per 256-thread workgroup: the S^3 bytes are staged into LDS, and per element the
// tables of tg_symmetry.hip (pi_m[a] * stride of mode rho[m] | sign << 16) give the source of every entry.
#include <hip/hip_runtime.h>

#include "../../include/tensor_game_orbits.h"
#include "tg_lists.h"
#include "tg_sol_copy.h"
#include "tg_sol_phases.h"
#include "tg_sym_code.h"

namespace tg {

struct OrbArgs {
  const int8_t* targets;   // (M, S, S, S) or null
  const int8_t* tokens;    // (M, K, 3S)
  const int64_t* lengths;  // (M)
  int64_t M;
  const uint8_t* sym;      // (G, 3S+1)
  int8_t* canon;           // (M, K, 3S)
  int32_t* rank;
  uint64_t* key;
  int32_t* residual;       // or null
  int32_t* which;
  int32_t* stab;
  uint32_t* status;        // or null
  uint8_t* ws;             // (M, NS) slice records of `rec` bytes, or null when NS == 1
  int K, S, shift, G;
  int NS, per;             // slices of the set and elements per slice
  int img;                 // bytes of one LDS image: K * 3S rounded up to 16
  int region;              // bytes of the keys: K * max(P, kSolWRow)
  int rec;                 // bytes of a slice record: img + kOrbHdr
};

constexpr int kOrbHdr = 32;      // a slice record's header behind its image: int32 rank, which, stab, flags, nnz
constexpr int kOrbMinSlice = 8;  // elements per slice at least: staging and verifying a list costs about as much
constexpr uint32_t kOrbEqual = 0xffffffffu;

// the workgroup's minimum of x (uniform result)
template <int NT>
__device__ __forceinline__ uint32_t orb_block_min(uint32_t x, uint32_t* wmin, int t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = __shfl_xor(x, o, 64);
    x = y < x ? y : x;
  }
  if constexpr (NT == 64) return x;
  if ((t & 63) == 0) wmin[t >> 6] = x;
  __syncthreads();
  uint32_t r = wmin[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) r = wmin[i] < r ? wmin[i] : r;
  __syncthreads();
  return r;
}

// one 32-bit word of a chunk pair: the first differing byte, if any, as (byte index << 1) | (x's byte < y's, signed)
__device__ __forceinline__ void orb_word(uint32_t x, uint32_t y, int at, uint32_t& enc) {
  if (x == y) return;
  const int b = (__ffs(static_cast<int>(x ^ y)) - 1) >> 3;  // little endian: the lowest address is the lowest byte
  const int xs = static_cast<int8_t>(x >> (8 * b)), ys = static_cast<int8_t>(y >> (8 * b));
  enc = (static_cast<uint32_t>(at + b) << 1) | (xs < ys ? 1u : 0u);
}

// Rows a and b over `chunks` 16-byte chunks (both 16-byte aligned), compared byte by byte as signed tokens: kOrbEqual,
// or (index of the first differing byte << 1) | (a is the smaller one).  Uniform result.
template <int NT>
__device__ __forceinline__ uint32_t orb_compare(const int8_t* a, const int8_t* b, int chunks, uint32_t* wmin, int t) {
  uint32_t enc = kOrbEqual;
  for (int c = t; c < chunks && enc == kOrbEqual; c += NT) {
    const uint4 x = reinterpret_cast<const uint4*>(a)[c], y = reinterpret_cast<const uint4*>(b)[c];
    orb_word(x.w, y.w, 16 * c + 12, enc);  // downwards: the lowest differing word is written last
    orb_word(x.z, y.z, 16 * c + 8, enc);
    orb_word(x.y, y.y, 16 * c + 4, enc);
    orb_word(x.x, y.x, 16 * c, enc);
  }
  return orb_block_min<NT>(enc, wmin, t);
}

// a bad list: zero canon row, rank 0, key 0, residual -1, which -1, stab 0
template <int NT>
__device__ __forceinline__ void orb_bad_row(const OrbArgs& a, int64_t m, int n_row, int t) {
  sol_copy_out<NT>(a.canon + m * n_row, nullptr, n_row, t);
  if (t == 0) {
    a.rank[m] = 0;
    a.key[m] = 0;
    a.which[m] = -1;
    a.stab[m] = 0;
    if (a.residual) a.residual[m] = -1;
  }
}

// the outputs of a good list from its winning image (zero behind rank * 3S, 16-byte aligned, LDS or workspace)
template <int NT>
__device__ __forceinline__ void orb_emit(const OrbArgs& a, int64_t m, const int8_t* best, int rank, int which, int stab,
                                         int nnz, uint64_t* red, int t) {
  const int A3 = 3 * a.S, n_row = a.K * A3;
  const uint64_t key = sol_image_key<NT>(best, rank * A3, red, t);
  sol_copy_out<NT>(a.canon + m * n_row, best, n_row, t);
  if (t == 0) {
    a.rank[m] = rank;
    a.key[m] = key;
    a.which[m] = which;
    a.stab[m] = stab;
    if (a.residual) a.residual[m] = nnz;
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void orbit_canon_kernel(OrbArgs a) {
  // the pristine image, the keys (first the verifier's w rows), two candidate images
  extern __shared__ __attribute__((aligned(16))) uint8_t orb_lds[];
  __shared__ uint64_t red[NT];
  __shared__ uint32_t wmin[4];
  __shared__ uint8_t fcode[3 * TG_SOL_MAX_K];  // per factor: 0 all zero, 1 as gathered, 2 negated; | 4: a token left int8
  __shared__ int8_t tsign[TG_SOL_MAX_K];       // per term: 0 null, else sigma
  __shared__ uint8_t keep[TG_SOL_MAX_K];       // per place among the live terms: the term there is kept
  __shared__ uint8_t tab[2][3 * TG_MAX_S];     // the decoded row of g, even and odd g in turn
  int8_t* const orig = reinterpret_cast<int8_t*>(orb_lds);
  uint8_t* const keys = orb_lds + a.img;
  int8_t* const buf0 = reinterpret_cast<int8_t*>(keys + a.region);
  int8_t* const buf1 = buf0 + a.img;
  const int t = threadIdx.x, S = a.S, A3 = 3 * S, K = a.K, shift = a.shift;
  const int n_row = K * A3, N3 = S * S * S, P = (A3 + 7) & ~7, chunks = a.img / 16;
  const int64_t jobs = a.M * a.NS;

  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t m = job / a.NS;
    const int s = static_cast<int>(job - m * a.NS);
    const int g0 = s * a.per, g1 = g0 + a.per < a.G ? g0 + a.per : a.G;
    const int64_t L64 = a.lengths[m];  // uniform: every barrier below is reached by the whole workgroup or by none
    const bool lenbad = L64 < 0 || L64 > K;  // checked before it addresses anything
    const int L = lenbad ? 0 : static_cast<int>(L64);
    uint32_t flags = lenbad ? TG_ORBIT_BAD_LENGTH : 0;
    sol_copy_in<NT>(a.tokens + m * n_row, orig, L * A3, t);
    for (int q = t; q < 2 * chunks; q += NT) reinterpret_cast<uint4*>(buf0)[q] = uint4{0, 0, 0, 0};
    __syncthreads();

    // ---- verify, from the original terms, once per list
    int nnz = 0;
    if (a.residual && s == 0 && !lenbad) {  // (the host refuses residual_nnz without targets)
      sol_stage_w<NT>(orig, reinterpret_cast<int8_t*>(keys), L, S, t);
      __syncthreads();
      nnz = sol_verify<NT>(orig, reinterpret_cast<const int8_t*>(keys), a.targets + m * N3, L, S, shift, t);
      __syncthreads();  // the w rows are read
    }
    for (int x = t; x < L * P; x += NT) {  // the keys' padding behind 3S bytes: the same for every g
      const int r = x / P, e = x - r * P;
      if (e >= A3) keys[r * P + sol_key_at(e)] = 0;
    }

    int cur = 0, ext0 = 0, ext1 = 0;  // the best image is buf<cur>; buf<i> is zero from ext<i> on
    int which = -1, stab = 0, brank = 0;
    for (int g = g0; g < g1; ++g) {
      // ---- the row of g, checked before it addresses anything
      uint8_t* const tb = tab[g & 1];
      const uint8_t* row = a.sym + static_cast<int64_t>(g) * (A3 + 1);
      const int code = row[0];
      bool bad1 = false;
      for (int x = t; x <= A3; x += NT) {
        const int b = row[x];
        if (x == 0) {
          bad1 |= b > 5;
        } else {
          const int p = b & 127, mm = (x - 1) / S;
          bad1 |= p >= S;
          tb[x - 1] = static_cast<uint8_t>(((rho_of(code > 5 ? 0 : code, mm) * S + p) & 127) | (b & 128));
        }
      }
      if (__syncthreads_or(bad1)) {  // (also: the table is written, and whatever the last g left is read)
        flags |= TG_ORBIT_BAD_GROUP;
        continue;
      }
      // a bad list only scans the rows (a bad row elsewhere in the set does not stop the search for a bad negation:
      // each bit is decided on its own, wherever the set is cut)
      if (flags & (TG_ORBIT_BAD_LENGTH | TG_ORBIT_BAD_NEGATION)) continue;

      // ---- gather and normalise: factor q = 3 * term + mm of g.X, straight into the keys
      for (int q = t; q < 3 * L; q += NT) {
        const int term = q / 3, mm = q - 3 * term;
        const int8_t* src = orig + term * A3;
        const uint8_t* tm = tb + mm * S;
        int first = 0;
        for (int e = 0; e < S && first == 0; ++e) {
          const int c = tm[e], v = src[c & 127] - shift;
          first = (c & 128) ? -v : v;
        }
        uint8_t fc = first == 0 ? 0 : first > 0 ? 1 : 2;
        uint8_t* kd = keys + term * P;
        for (int e = 0; e < S; ++e) {
          const int c = tm[e];
          int v = src[c & 127] - shift;
          v = ((c & 128) != 0) != (first < 0) ? -v : v;
          const int tk = v + shift;
          if (tk < -128 || tk > 127) fc |= 4;
          kd[sol_key_at(mm * S + e)] = sol_key_flip(tk);
        }
        fcode[q] = fc;
      }
      __syncthreads();
      int bad = sol_term_sign(fcode, tsign, L, t);
      __syncthreads();

      // ---- order and merge: thread t = term t (K <= NT)
      const SolRank o = sol_rank(keys, tsign, keep, L, P, t);
      __syncthreads();

      // ---- emit into the image that is not the best
      int8_t* const cand = cur ? buf0 : buf1;
      const int extc = cur ? ext0 : ext1;
      if (o.kept) {
        const uint8_t* me = keys + t * P;
        int8_t* dst = cand + sol_kept_below(keep, o.place) * A3;
        for (int e = 0; e < A3; ++e) {
          int v = static_cast<int8_t>(sol_key_flip(me[sol_key_at(e)]));
          if (e >= 2 * S && o.c < 0) {
            v = 2 * shift - v;
            bad |= v < -128 || v > 127;
          }
          dst[e] = static_cast<int8_t>(v);
        }
      }
      const int rank = __syncthreads_count(o.kept);  // (also: the kept terms are in the image, the flags are read)
      if (__syncthreads_or(bad)) {
        flags |= TG_ORBIT_BAD_NEGATION;
        continue;
      }
      const int n = rank * A3;
      if (extc > n) {  // an earlier candidate of a higher rank: only a row with repeated indices can change the rank
        for (int x = n + t; x < extc; x += NT) cand[x] = 0;
        __syncthreads();
      }
      if (cur) ext0 = n;
      else ext1 = n;

      // ---- compare with the best so far
      bool take = which < 0;
      if (take) {
        stab = 1;
      } else {
        const int extb = cur ? ext1 : ext0, span = n > extb ? n : extb;
        const uint32_t enc = orb_compare<NT>(cand, cur ? buf1 : buf0, (span + 15) / 16, wmin, t);
        if (enc == kOrbEqual) ++stab;
        else if (enc & 1u) take = true, stab = 1;
      }
      if (take) {
        cur ^= 1;
        which = g;
        brank = rank;
      }
    }
    __syncthreads();  // the last compare is done: red and the images are free

    const int8_t* best = cur ? buf1 : buf0;
    if (flags && t == 0 && a.status) atomicOr(a.status, flags);
    if (a.NS == 1) {
      if (flags) {
        orb_bad_row<NT>(a, m, n_row, t);
      } else {
        const int total = static_cast<int>(sol_block_sum<NT>(static_cast<uint64_t>(nnz), red, t));
        orb_emit<NT>(a, m, best, brank, which, stab, total, red, t);
      }
    } else {
      uint8_t* rec = a.ws + job * a.rec;
      for (int q = t; q < chunks; q += NT) reinterpret_cast<uint4*>(rec)[q] = reinterpret_cast<const uint4*>(best)[q];
      const int total = static_cast<int>(sol_block_sum<NT>(static_cast<uint64_t>(nnz), red, t));
      if (t == 0) {
        int32_t* hdr = reinterpret_cast<int32_t*>(rec + a.img);
        hdr[0] = brank;
        hdr[1] = which;
        hdr[2] = stab;
        hdr[3] = static_cast<int32_t>(flags);
        hdr[4] = total;
      }
    }
    __syncthreads();  // the images, the keys and the flags are free for the next list
  }
}

// The second pass of a sliced call: the smallest of a list's NS slice winners, in slice order.
template <int NT>
__global__ __launch_bounds__(NT) void orbit_reduce_kernel(OrbArgs a) {
  __shared__ uint64_t red[NT];
  __shared__ uint32_t wmin[4];
  const int t = threadIdx.x, n_row = a.K * 3 * a.S, chunks = a.img / 16;
  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    const uint8_t* recs = a.ws + m * a.NS * a.rec;
    auto hdr = [&](int s) { return reinterpret_cast<const int32_t*>(recs + static_cast<int64_t>(s) * a.rec + a.img); };
    auto image = [&](int s) { return reinterpret_cast<const int8_t*>(recs + static_cast<int64_t>(s) * a.rec); };
    int fl = 0;
    for (int s = t; s < a.NS; s += NT) fl |= hdr(s)[3];
    if (__syncthreads_or(fl)) {  // (the first pass has set the status bits)
      orb_bad_row<NT>(a, m, n_row, t);
      continue;
    }
    int best = 0, stab = hdr(0)[2];
    for (int s = 1; s < a.NS; ++s) {
      const uint32_t enc = orb_compare<NT>(image(s), image(best), chunks, wmin, t);
      if (enc == kOrbEqual) stab += hdr(s)[2];
      else if (enc & 1u) best = s, stab = hdr(s)[2];
    }
    orb_emit<NT>(a, m, image(best), hdr(best)[0], hdr(best)[1], stab, hdr(0)[4], red, t);
    __syncthreads();
  }
}

struct FixArgs {
  const int8_t* targets;  // (M, S, S, S)
  int64_t M;
  const uint8_t* sym;     // (G, 3S+1)
  uint8_t* fixes;         // (M)
  uint32_t* status;       // or null
  int S, G;
};

__global__ __launch_bounds__(kBlock) void orbit_fixes_kernel(FixArgs a) {
  __shared__ __attribute__((aligned(16))) int8_t T[TG_MAX_S * TG_MAX_S * TG_MAX_S];
  __shared__ int tabs[2][3 * TG_MAX_S];  // pi_m[a] * stride of mode rho[m] | sign << 16, even and odd g in turn
  const int t = threadIdx.x, S = a.S, S2 = S * S, N3 = S2 * S, A3 = 3 * S;
  for (int64_t m = blockIdx.x; m < a.M; m += gridDim.x) {
    const int8_t* src = a.targets + m * N3;
    for (int e = t; e < N3; e += kBlock) T[e] = src[e];
    bool ok = true, gbad = false;
    for (int g = 0; g < a.G; ++g) {
      int* const tb = tabs[g & 1];
      const uint8_t* row = a.sym + static_cast<int64_t>(g) * (A3 + 1);
      const int code = row[0];
      bool bad1 = false;
      for (int x = t; x <= A3; x += kBlock) {  // the row is checked before it addresses anything
        const int b = row[x];
        if (x == 0) {
          bad1 |= b > 5;
        } else {
          const int p = b & 127, mm = (x - 1) / S, rm = rho_of(code > 5 ? 0 : code, mm);
          bad1 |= p >= S;
          tb[x - 1] = p * (rm == 0 ? S2 : rm == 1 ? S : 1) | ((b & 128) ? kSymNeg : 0);
        }
      }
      if (__syncthreads_or(bad1)) {  // (also: the target and the table are in LDS)
        gbad = true;
        continue;
      }
      for (int e = t; e < N3; e += kBlock) {
        const int a0 = e / S2, r = e - a0 * S2, a1 = r / S, a2 = r - a1 * S;
        const int x = tb[a0] + tb[S + a1] + tb[2 * S + a2];
        const int v = T[x & 0x7fff];  // int32: the negative of -128 is 128
        ok &= ((x & kSymNeg) ? -v : v) == T[e];
      }
    }
    const int all = __syncthreads_and(ok);  // (also: the target is read)
    if (t == 0) {
      a.fixes[m] = all && !gbad;
      if (gbad && a.status) atomicOr(a.status, 1u);
    }
  }
}

}  // namespace tg

namespace {

int orbit_sizes(const char* fn, int64_t M, int K, int S, int shift, int G) {
  if (const int rc = check_lists(fn, K, S, shift, TG_SOL_MAX_K, TG_ORBIT_MAX_ROW)) return rc;
  if (G < 1 || G > TG_ORBIT_MAX_G) return tg_internal_fail(TG_ERR_INVALID, "%s: G=%d outside [1,%d]", fn, G, TG_ORBIT_MAX_G);
  return check_list_count(fn, M);
}

struct OrbitPlan {
  int nt, per_cu, img, region, rec, NS, per;
  int64_t bytes;
};

// The decomposition for M lists: slices only while M workgroups leave the device idle, and of kOrbMinSlice elements at least.
OrbitPlan orbit_plan(int64_t M, int K, int S, int G) {
  OrbitPlan p{};
  p.nt = K <= 64 ? 64 : 256;
  p.per_cu = p.nt == 64 ? 32 : 8;
  const int64_t resident = static_cast<int64_t>(p.per_cu) * device_cu_count();
  p.img = list_image_bytes(K, S);
  const int P = (3 * S + 7) & ~7;
  p.region = (K * (P > tg::kSolWRow ? P : tg::kSolWRow) + 15) & ~15;
  p.rec = p.img + tg::kOrbHdr;
  int NS = 1;
  if (M > 0 && M < resident) {
    const int64_t want = resident / M, cap = G / tg::kOrbMinSlice;
    NS = static_cast<int>(want < cap ? want : cap);
    if (NS < 1) NS = 1;
  }
  p.per = (G + NS - 1) / NS;
  p.NS = (G + p.per - 1) / p.per;  // no empty slice
  p.bytes = p.NS > 1 ? M * p.NS * p.rec : 0;
  return p;
}

template <int NT>
int launch_orbit(const tg::OrbArgs& a, const OrbitPlan& p, hipStream_t st) {
  const char* fn = "tg_orbit_canon";
  const size_t lds = 3 * static_cast<size_t>(a.img) + static_cast<size_t>(a.region);
  if (const int rc = lds_opt_in<tg::orbit_canon_kernel<NT>>(fn, lds)) return rc;
  if (const int rc = launch_resident(fn, tg::orbit_canon_kernel<NT>, a.M * a.NS, p.per_cu, NT, lds, st, a)) return rc;
  if (a.NS == 1) return TG_OK;
  return launch_resident(fn, tg::orbit_reduce_kernel<64>, a.M, 32, 64, 0, st, a);
}

}  // namespace

extern "C" int tg_orbit_check(int64_t M, int K, int S, int shift, int G) {
  return orbit_sizes("tg_orbit_check", M, K, S, shift, G);
}

extern "C" int tg_orbit_workspace_size(int64_t M, int K, int S, int G, int64_t* bytes) {
  const char* fn = "tg_orbit_workspace_size";
  if (const int rc = orbit_sizes(fn, M, K, S, 0, G)) return rc;
  if (!bytes) return tg_internal_fail(TG_ERR_INVALID, "%s: null bytes", fn);
  *bytes = orbit_plan(M, K, S, G).bytes;
  return TG_OK;
}

extern "C" int tg_orbit_fixes(const int8_t* targets, int64_t M, int S, const uint8_t* sym, int G, uint8_t* fixes,
                              uint32_t* status, tg_stream_t stream) {
  const char* fn = "tg_orbit_fixes";
  if (S < 1 || S > TG_MAX_S) return tg_internal_fail(TG_ERR_INVALID, "%s: S=%d outside [1,%d]", fn, S, TG_MAX_S);
  if (G < 1 || G > TG_ORBIT_MAX_G) return tg_internal_fail(TG_ERR_INVALID, "%s: G=%d outside [1,%d]", fn, G, TG_ORBIT_MAX_G);
  if (M < 0 || M > INT64_MAX / (static_cast<int64_t>(TG_MAX_S) * TG_MAX_S * TG_MAX_S))
    return tg_internal_fail(TG_ERR_INVALID, "%s: M=%lld out of range", fn, (long long)M);
  if (M == 0) return TG_OK;
  if (!targets) return tg_internal_fail(TG_ERR_INVALID, "%s: null targets", fn);
  if (!sym) return tg_internal_fail(TG_ERR_INVALID, "%s: null sym", fn);
  if (!fixes) return tg_internal_fail(TG_ERR_INVALID, "%s: null fixes", fn);
  if (!aligned(status, 4)) return tg_internal_fail(TG_ERR_INVALID, "%s: status not 4-byte aligned", fn);
  const tg::FixArgs a{targets, M, sym, fixes, status, S, G};
  return launch_resident(fn, tg::orbit_fixes_kernel, M, 8, tg::kBlock, 0, static_cast<hipStream_t>(stream), a);
}

extern "C" int tg_orbit_canon(const int8_t* targets, const int8_t* tokens, const int64_t* lengths, int64_t M, int K, int S,
                              int shift, const uint8_t* sym, int G, int8_t* canon, int32_t* rank, uint64_t* key,
                              int32_t* residual_nnz, int32_t* which, int32_t* stab, uint32_t* status, void* workspace,
                              int64_t workspace_bytes, tg_stream_t stream) {
  const char* fn = "tg_orbit_canon";
  if (const int rc = orbit_sizes(fn, M, K, S, shift, G)) return rc;
  if (M == 0) return TG_OK;
  const tg::CanonPointers ptrs{targets, tokens, lengths, canon, rank, key, residual_nnz, status, true, sym, which, stab};
  if (const int rc = check_canon_pointers(fn, ptrs)) return rc;
  OrbitPlan p = orbit_plan(M, K, S, G);
  if (!workspace || p.NS == 1) {
    p.NS = 1;
    p.per = G;
    workspace = nullptr;
  } else {
    if (!aligned(workspace, 16)) return tg_internal_fail(TG_ERR_INVALID, "%s: workspace not 16-byte aligned", fn);
    if (workspace_bytes < p.bytes)
      return tg_internal_fail(TG_ERR_INVALID, "%s: workspace_bytes=%lld below the %lld tg_orbit_workspace_size asks for", fn,
                              (long long)workspace_bytes, (long long)p.bytes);
  }
  const tg::OrbArgs a{targets, tokens, lengths, M, sym, canon, rank, key, residual_nnz, which, stab, status,
                      static_cast<uint8_t*>(workspace), K, S, shift, G, p.NS, p.per, p.img, p.region, p.rec};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (p.nt == 64) return launch_orbit<64>(a, p, st);  // a wavefront per (list, slice)
  return launch_orbit<256>(a, p, st);                 // a 256-thread workgroup per (list, slice)
}
