// tg_s16.h -- S = 16 with one wavefront per game, registers only (included inside namespace tg by tg_kernels.hip after
// tg_s4.h): the single step (s16_step_kernel), the fused step + model input (s16_step_emit_kernel) and the tracked step
// (s16_tracked_kernel).

// =============================================================================================
// S = 16 single step, register only.  One wavefront per game; lane = (r, j) owns the four rows
// (i = r + 4n, j), n = 0..3, i.e. chunks lane + 64 n.  The game's 48 tokens come straight into
// registers (u and w as uniform dwordx4 loads, v_j as a byte), so there is no LDS staging and no
// workgroup barrier: the wavefront's dependency chain is ONE memory round trip, arithmetic, stores.
// (The staged packed_kernel needs three barriers.)  Factors beyond the 16-bit path's range are handled
// by the same wavefront in 32-bit.  Requires 16-byte aligned state and actions.
//
// History: in rounds 2 and 3 the rows the action touches (u_i v_j != 0: 9 % under the reference's factor distribution) were
// COMPACTED into a 64-entry queue of the wavefront in LDS and worked on in one dense pass, because the unpack / multiply-add
// / pack / range test of all four chunks in the packed int16 form was 45 % of the kernel (4.0 us without it at BASELINE
// config 3, 6.6 with).  With the digit form a row costs ~20 instructions and the kernel does every row in its own lane
// again (comment inside); the queue is gone.
// =============================================================================================
// one chunk: x - (-uv) ... i.e. x + uvn * w, uvn = -u_i v_j; saturating int16 form, 32-bit redo when the range test fails
// (wfetch: the game's 16 w tokens again, for the redo only -- keeping them would cost four registers on the common path)
// The digit form of one row (round 3; s4_step_digits has the argument): a row is 16 bytes = four base-256 integers of
// biased digits, the game's w the four integers Wd[d] = w token dword - shift * 0x01010101, and the update of dword d is
// ONE multiply-add, X' = X + uvn * Wd[d] -- exact when no digit leaves [0, 255], which the caller guarantees up front:
// all 48 tokens <= 3 and 0 <= shift <= 3 (wave-uniform, on the scalar unit) bound every |u v w| by F^3, and the row's
// L1 norm (four v_sad_u8) bounds every |x|.  ~20 VALU instructions per row instead of ~32, and the sixteen that build
// the int16 weight pairs leave the kernel's common path altogether.  Returns false when this lane's row is not covered.
__device__ __forceinline__ bool s16_chunk_digits(const uint4& x, int uvn, const uint32_t (&Wd)[4], int limit, uint4& res,
                                                 uint32_t& cnz) {
  const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
  uint32_t o[4], l1 = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t xb = xs[d] ^ 0x80808080u;
    l1 = __builtin_amdgcn_sad_u8(xb, 0x80808080u, l1);
    o[d] = (xb + static_cast<uint32_t>(uvn) * Wd[d]) ^ 0x80808080u;
  }
  res = uint4{o[0], o[1], o[2], o[3]};
  cnz = o[0] | o[1] | o[2] | o[3];
  return static_cast<int>(l1) <= limit;
}

template <class WFetch>
__device__ __forceinline__ uint4 s16_chunk(const uint4& x, int uvn, const uint32_t (&wp)[8], WFetch wfetch, int shift,
                                           bool wide_shift, uint32_t& cnz, uint32_t& ovf) {
  // Saturating int16 form, as in s4_step_slice: with |factor| <= 255 (int8 tokens, |shift| <= 127) the clamped u*v and
  // (u v) w + x are formed exactly or saturate, so everything the 16-bit form cannot represent ends outside int8 --
  // exactly the results that overflow.  No check of the factors; a chunk whose range test fails is redone in 32-bit by
  // its lane (wrapped bytes + flag).
  const int cl = max(-32767, min(32767, uvn));
  const uint32_t pr = __builtin_amdgcn_perm(static_cast<uint32_t>(cl), static_cast<uint32_t>(cl), 0x05040100u);
  uint32_t A[8];
  unpack_pairs(x, A);
#pragma unroll
  for (int p = 0; p < 8; ++p) A[p] = pk_mad_i16_sat(pr, wp[p], A[p]);
  uint32_t c16 = 0;
  cnz = 0;
  uint4 res = pack_pairs(A, cnz, c16);
  if (__builtin_expect(wide_shift || (c16 & 0xFF00FF00u), 0)) {  // rare: exact 32-bit form of this chunk,
    const uint4 wq = wfetch();
    const uint32_t wd[4] = {wq.x, wq.y, wq.z, wq.w};              // one dword at a time (the common path keeps <= 64 VGPRs:
    const uint32_t pd[4] = {x.x, x.y, x.z, x.w};                  // 8 wavefronts per SIMD, cfg3 resident in one round)
    uint32_t rd[4];
    int o32 = 0;
    cnz = 0;
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
      int e[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        e[t] = sbyte(pd[d], t) + uvn * (sbyte(wd[d], t) - shift);
        o32 |= e[t] + 128;
      }
      rd[d] = pack4(e[0], e[1], e[2], e[3]);
      cnz |= rd[d];
    }
    res = uint4{rd[0], rd[1], rd[2], rd[3]};
    ovf |= static_cast<uint32_t>(o32) & ~255u;
  }
  return res;
}

// LINES: stores at 128-byte-line granularity -- a chunk is stored when any of the eight chunks of its line changed.
// For batches that stream from HBM: a partially written line costs the memory side a read-modify-write (measured at
// 131 072 games: 148 us with 16-byte or 64-byte stores, 130 us with whole lines, although those write 1.7x the bytes).
// Cache-resident batches store only the rows that changed.
// NTL: the state is read by non-temporal loads.  With whole-line stores and a batch beyond the 256 MiB Infinity Cache
// that is worth a quarter of the launch (131 072 games = 512 MiB: 131.5 -> 99.0 us; 262 144 games: 260 -> 232); up to
// ~300 MiB it is neutral to harmful (77 000 games = 301 MiB: 58.7 / 60.3 us, 65 536 games: 50.3 / 52.0, BASELINE config
// 3: 6.0 / 8.5), from 86 000 games = 336 MiB on it wins (80.0 / 66.4): taken from 320 MiB on.  Without whole-line stores
// (the S = 25 step as it was: 16-byte pieces) it gains nothing at any size (143.1 / 143.0 us at 32 768 games).
// DIG: rows go through the digit form first (false only in the A/B library: TG_S16_NO_DIGITS).
template <int MODE, bool LINES, bool NTL = false, bool DIG = true>
__global__ __launch_bounds__(kBlock, LINES ? 6 : 8) void s16_step_kernel(ApplyArgs a) {  // (LINES keeps the inputs to the end)
  static_assert(MODE == STEP, "s16_step_kernel: single step only");
  // (the wavefront index is uniform; saying so lets the game's tokens come by scalar loads)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  int64_t g = static_cast<int64_t>(sweep_index(blockIdx.x, gridDim.x, a.sweep)) * (kBlock / 64) + wave;
  const bool live = g < a.B;
  if (!live) g = a.B - 1;
  const int8_t* tok = a.actions + g * 48;
  const int8_t* src = a.in + g * a.in_stride + 16 * lane;
  // every load of the wavefront is issued before anything is used.  (Four named chunks, not an array: hipcc keeps an
  // array that lives to the end of the LINES variant in scratch.)
  auto ld = [&](const int8_t* q) {
    if constexpr (NTL) {
      const v4u_t v = __builtin_nontemporal_load(reinterpret_cast<const v4u_t*>(q));
      return uint4{v.x, v.y, v.z, v.w};
    } else {
      return *reinterpret_cast<const uint4*>(q);
    }
  };
  const uint4 p0 = ld(src), p1 = ld(src + 1024), p2 = ld(src + 2048), p3 = ld(src + 3072);
  const uint4 uq = *reinterpret_cast<const uint4*>(tok);
  const uint4 wq = *reinterpret_cast<const uint4*>(tok + 32);
  auto wfetch = [&]() { return *reinterpret_cast<const uint4*>(tok + 32); };
  const int vj = tok[16 + (lane & 15)] - a.shift;
  const int r = lane >> 4;
  uint32_t nz = 0, ovf = 0;
  const bool inplace = a.in == a.out;
  int8_t* const out = a.out + g * a.out_stride;
  const uint32_t shp = (static_cast<uint32_t>(a.shift) & 0xFFFFu) | (static_cast<uint32_t>(a.shift) << 16);
  const bool wide_shift = static_cast<unsigned>(a.shift + 127) > 254u;  // uniform; factors may exceed 255
  // digit form (s16_chunk_digits): its precondition on tokens and shift is wave-uniform -- all 48 tokens come by scalar
  // loads -- so a game either offers it to every row or to none; limit < 0 = not offered
  const uint4 vq = *reinterpret_cast<const uint4*>(tok + 16);
  const uint32_t tok_or = uq.x | uq.y | uq.z | uq.w | vq.x | vq.y | vq.z | vq.w | wq.x | wq.y | wq.z | wq.w;
  const int dig_limit = (DIG && (tok_or & 0xFCFCFCFCu) == 0) ? s4_digits_limit(a.shift) : -1;
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  const uint32_t Wd[4] = {wq.x - shrep, wq.y - shrep, wq.z - shrep, wq.w - shrep};
  // one row, digit form first; the packed int16 form (its weight pairs built here, off the common path) for the rest
  auto chunk = [&](const uint4& x, int uvn, uint32_t& cnz) {
    uint4 res;
    if (__builtin_expect(s16_chunk_digits(x, uvn, Wd, dig_limit, res, cnz), 1)) return res;
    uint32_t wp[8];
    unpack_pairs(wq, wp);
#pragma unroll
    for (int p = 0; p < 8; ++p) wp[p] = pk_sub_i16(wp[p], shp);
    return s16_chunk(x, uvn, wp, wfetch, a.shift, wide_shift, cnz, ovf);
  };
  auto differs = [](const uint4& x, const uint4& y) { return x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w; };
  // does this lane store chunk (lane, n), given whether it changed and the ballot of the lanes whose chunk n changed?
  auto stores = [&](bool changed, unsigned long long cm) {
    if (!inplace) return true;  // out of place everything is written
    return LINES ? ((cm >> (lane & ~7)) & 0xFFull) != 0 : changed;
  };

  {
    // EVERY row by its own lane (round 3, late).  Rounds 2-3 compacted the rows the action touches (9 %) into a queue of
    // the wavefront in LDS and did the arithmetic in one dense pass: that paid while a row cost ~32 instructions (packed
    // int16 form).  In the digit form a row costs ~20, and the compaction -- ballots, slots, two LDS trips, a divergent
    // dense pass, for the whole-line variants a third trip back to the owners -- costs more than it saves: 5.61 -> 5.51 us
    // at BASELINE config 3, 3.08 -> 2.87 at 2 048 games, equal within 1.5 % from 128 MiB to 2 GiB of states.
    auto one = [&](int n, const uint4& pn, uint32_t udw) {
      const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(udw), 8 * r, 8);  // -(u_i), i = r + 4 n
      const int uvn = ui * vj;
      uint32_t cnz;
      const uint4 res = chunk(pn, uvn, cnz);
      nz |= cnz;
      // in place, a row the action left as it was needs no store (LINES: unless one of the eight rows of its line changed)
      const bool chg = differs(res, pn);
      const bool st = LINES ? stores(chg, __ballot(chg)) : (!inplace || chg);
      if (live && st) *reinterpret_cast<uint4*>(out + 16 * (lane + 64 * n)) = res;
    };
    one(0, p0, uq.x);
    one(1, p1, uq.y);
    one(2, p2, uq.z);
    one(3, p3, uq.w);
    const bool any_nz0 = __ballot(nz != 0) != 0;
    const bool any_ovf0 = __ballot(ovf != 0) != 0;
    if (lane == 0 && live) {
      a.done[g] = any_nz0 ? 0 : 1;
      if (a.overflow && any_ovf0) a.overflow[g] = 1;
    }
  }
}

// =============================================================================================
// tg_step_emit at S = 16 (round 4): one env step on the history ring AND the (B,T,16,16,16) float model input of the new
// state in one launch, while that output stays in the caches (two launches -- tg_step_i8, then emit_frames_kernel --
// measured 15.9 us at 1 024 games, T = 4, float16, of which the frames alone are 9.0: the step's round trip and a launch
// boundary are what a fused kernel saves; from kStreamOutBytes of output on the frames kernel's write stream is the
// whole cost and the entry stays two launches).
// s16_step_kernel's mapping -- a wavefront per game, lane (r, j) owns rows (i = r + 4 n, j) = chunks lane + 64 n -- so a
// lane's sixteen elements of a chunk leave as 32 (16-bit types) or 64 (float32) contiguous output bytes; frame 0 comes
// from the registers that hold the new head, frame 1 from the registers the step read the old head into, older frames
// from the ring.
// =============================================================================================
template <typename OutT, bool NT>
__device__ __forceinline__ void s16_emit_chunk(OutT* dst, const uint4& q) {  // sixteen int8 -> sixteen OutT at dst
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  if constexpr (sizeof(OutT) == 4) {
#pragma unroll
    for (int d = 0; d < 4; ++d) s4_emit_f32<NT>(reinterpret_cast<float*>(dst) + 4 * d, w[d]);
  } else {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint2 a = s4_cvt16<OutT>(w[2 * hh]), b = s4_cvt16<OutT>(w[2 * hh + 1]);
      const uint4 o{a.x, a.y, b.x, b.y};
      if constexpr (NT) store16_nt(dst + 8 * hh, o);
      else *reinterpret_cast<uint4*>(dst + 8 * hh) = o;
    }
  }
}

template <typename OutT, bool NT>
__global__ __launch_bounds__(kBlock) void s16_step_emit_kernel(StepEmitArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  int64_t g = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave;
  const bool live = g < a.B;
  if (!live) g = a.B - 1;
  const int8_t* tok = a.actions + g * 48;
  int8_t* const game = a.ring + g * a.game_stride;
  const int nxt = a.head + 1 < a.T ? a.head + 1 : 0;
  const int8_t* src = game + a.head * a.frame_stride + 16 * lane;
  const uint4 p0 = *reinterpret_cast<const uint4*>(src), p1 = *reinterpret_cast<const uint4*>(src + 1024),
              p2 = *reinterpret_cast<const uint4*>(src + 2048), p3 = *reinterpret_cast<const uint4*>(src + 3072);
  const uint4 uq = *reinterpret_cast<const uint4*>(tok);
  const uint4 vq = *reinterpret_cast<const uint4*>(tok + 16);
  const uint4 wq = *reinterpret_cast<const uint4*>(tok + 32);
  auto wfetch = [&]() { return *reinterpret_cast<const uint4*>(tok + 32); };
  const int vj = tok[16 + (lane & 15)] - a.shift;
  const int r = lane >> 4;
  uint32_t nz = 0, ovf = 0;
  const uint32_t shp = (static_cast<uint32_t>(a.shift) & 0xFFFFu) | (static_cast<uint32_t>(a.shift) << 16);
  const bool wide_shift = static_cast<unsigned>(a.shift + 127) > 254u;
  const uint32_t tok_or = uq.x | uq.y | uq.z | uq.w | vq.x | vq.y | vq.z | vq.w | wq.x | wq.y | wq.z | wq.w;
  const int dig_limit = (tok_or & 0xFCFCFCFCu) == 0 ? s4_digits_limit(a.shift) : -1;
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  const uint32_t Wd[4] = {wq.x - shrep, wq.y - shrep, wq.z - shrep, wq.w - shrep};
  auto chunk = [&](const uint4& x, int uvn, uint32_t& cnz) {  // (s16_step_kernel: the digit form first, then the packed int16 form)
    uint4 res;
    if (__builtin_expect(s16_chunk_digits(x, uvn, Wd, dig_limit, res, cnz), 1)) return res;
    uint32_t wp[8];
    unpack_pairs(wq, wp);
#pragma unroll
    for (int p = 0; p < 8; ++p) wp[p] = pk_sub_i16(wp[p], shp);
    return s16_chunk(x, uvn, wp, wfetch, a.shift, wide_shift, cnz, ovf);
  };
  OutT* const out = static_cast<OutT*>(a.out) + g * (static_cast<int64_t>(a.T) * 4096) + 16 * lane;
  int8_t* const dst = game + nxt * a.frame_stride + 16 * lane;
  auto one = [&](int n, const uint4& pn, uint32_t udw) {
    const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(udw), 8 * r, 8);  // -(u_i), i = r + 4 n
    uint32_t cnz;
    const uint4 res = chunk(pn, ui * vj, cnz);
    nz |= cnz;
    if (live) {
      *reinterpret_cast<uint4*>(dst + 1024 * n) = res;                      // the new head -> ring slot nxt
      s16_emit_chunk<OutT, NT>(out + 1024 * n, res);                        // frame 0
      if (a.T > 1) s16_emit_chunk<OutT, NT>(out + 4096 + 1024 * n, pn);     // frame 1: the old head
    }
  };
  one(0, p0, uq.x);
  one(1, p1, uq.y);
  one(2, p2, uq.z);
  one(3, p3, uq.w);
  if (live) {
    int slot = a.head;
    for (int f = 2; f < a.T; ++f) {  // older frames from the ring
      slot = slot > 0 ? slot - 1 : a.T - 1;
      const int8_t* const old = game + slot * a.frame_stride + 16 * lane;
      const uint4 z0 = *reinterpret_cast<const uint4*>(old), z1 = *reinterpret_cast<const uint4*>(old + 1024),
                  z2 = *reinterpret_cast<const uint4*>(old + 2048), z3 = *reinterpret_cast<const uint4*>(old + 3072);
      OutT* const of = out + static_cast<int64_t>(f) * 4096;
      s16_emit_chunk<OutT, NT>(of, z0);
      s16_emit_chunk<OutT, NT>(of + 1024, z1);
      s16_emit_chunk<OutT, NT>(of + 2048, z2);
      s16_emit_chunk<OutT, NT>(of + 3072, z3);
    }
  }
  const bool any_nz0 = __ballot(nz != 0) != 0;
  const bool any_ovf0 = __ballot(ovf != 0) != 0;
  if (lane == 0 && live) {
    a.done[g] = any_nz0 ? 0 : 1;
    if (a.scalars) a.scalars[g] = a.t_step;
    if (a.overflow && any_ovf0) a.overflow[g] = 1;
  }
}

// =============================================================================================
// tg_step_tracked_i8 at S = 16 (round 3; s25_tracked_kernel in tg_packed.h has the argument): the in-place step that
// loads only the rows the action touches -- row (i, j) changes iff u_i v_j != 0, which the tokens alone decide: ~9 % of the
// rows, in ~28 % of the game's 128-byte lines -- with the number of non-zero entries carried per game.
// One wavefront per game as in s16_step_kernel; the candidate rows' INDICES are compacted into a queue of up to 256
// entries (every row: never flushed), lane k takes entries k, k + 64, ... with all their loads in flight together,
// then per row: count the non-zero bytes, apply (digit form first, packed int16 form behind it), count again, store.
// =============================================================================================
__global__ __launch_bounds__(kBlock, 8) void s16_tracked_kernel(ApplyArgs a, int32_t* nnz) {
  constexpr int NW = kBlock / 64;
  __shared__ __attribute__((aligned(8))) int2 qm[NW][256];  // (row index i * 16 + j, -u_i v_j)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  int64_t g = static_cast<int64_t>(blockIdx.x) * NW + wave;
  const bool live = g < a.B;
  if (!live) g = a.B - 1;
  const int8_t* tok = a.actions + g * 48;
  int8_t* const st = a.out + g * a.out_stride;
  const int nnz_in = nnz[g];
  const uint4 uq = *reinterpret_cast<const uint4*>(tok);
  const uint4 vq = *reinterpret_cast<const uint4*>(tok + 16);
  const uint4 wq = *reinterpret_cast<const uint4*>(tok + 32);
  auto wfetch = [&]() { return *reinterpret_cast<const uint4*>(tok + 32); };
  const int vj = tok[16 + (lane & 15)] - a.shift;
  const int r = lane >> 4;
  const uint32_t shp = (static_cast<uint32_t>(a.shift) & 0xFFFFu) | (static_cast<uint32_t>(a.shift) << 16);
  const bool wide_shift = static_cast<unsigned>(a.shift + 127) > 254u;
  const uint32_t tok_or = uq.x | uq.y | uq.z | uq.w | vq.x | vq.y | vq.z | vq.w | wq.x | wq.y | wq.z | wq.w;
  const int dig_limit = (tok_or & 0xFCFCFCFCu) == 0 ? s4_digits_limit(a.shift) : -1;
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  const uint32_t Wd[4] = {wq.x - shrep, wq.y - shrep, wq.z - shrep, wq.w - shrep};
  uint32_t ovf = 0;
  auto chunk = [&](const uint4& x, int uvn, uint32_t& cnz) {
    uint4 res;
    if (__builtin_expect(s16_chunk_digits(x, uvn, Wd, dig_limit, res, cnz), 1)) return res;
    uint32_t wp[8];
    unpack_pairs(wq, wp);
#pragma unroll
    for (int p = 0; p < 8; ++p) wp[p] = pk_sub_i16(wp[p], shp);
    return s16_chunk(x, uvn, wp, wfetch, a.shift, wide_shift, cnz, ovf);
  };
  // ---- candidate rows -> the queue (indices only) ----
  const uint32_t ud[4] = {uq.x, uq.y, uq.z, uq.w};
  int total = 0;  // wave-uniform
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(ud[n]), 8 * r, 8);  // -(u_i), i = r + 4 n
    const int uvn = ui * vj;
    const bool cand = uvn != 0;
    const unsigned long long m = __ballot(cand);
    const int slot = total + static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
    if (cand) qm[wave][slot] = int2{lane + 64 * n, uvn};
    total += __builtin_popcountll(m);
  }
  __builtin_amdgcn_wave_barrier();  // (LDS serves one wavefront's accesses in order)
  // ---- dense passes: entries lane, lane + 64, ...; a pass's loads first ----
  int delta = 0;
  const int npass = (total + 63) >> 6;  // uniform; 1 for the reference's factor distribution
  for (int k0 = 0; k0 < npass; k0 += 2) {
    int2 me[2];
    uint4 x[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = lane + 64 * (k0 + k);
      me[k] = qm[wave][e < total ? e : 0];
      if (e >= total) me[k].x = -1;
      x[k] = *reinterpret_cast<const uint4*>(st + 16 * (me[k].x < 0 ? 0 : me[k].x));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (me[k].x >= 0) {
        uint32_t cnz;
        const uint4 res = chunk(x[k], me[k].y, cnz);
        delta += nz_bytes16(res) - nz_bytes16(x[k]);
        if (live && (res.x != x[k].x || res.y != x[k].y || res.z != x[k].z || res.w != x[k].w))
          *reinterpret_cast<uint4*>(st + 16 * me[k].x) = res;
      }
    }
  }
  delta = wave_sum(delta);
  const bool wovf = __ballot(ovf != 0) != 0;
  if (lane == 0 && live) {
    const int n = nnz_in + delta;
    nnz[g] = n;
    a.done[g] = n == 0 ? 1 : 0;
    if (a.overflow && wovf) a.overflow[g] = 1;
  }
}
