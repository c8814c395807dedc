// tg_stream.h -- the resident steppers of tg_step_stream_i8 (included inside namespace tg by tg_kernels.hip after
// tg_s16.h: the S = 16 stepper uses s16_chunk): s4_stream_kernel<NG>, s4_stream_kernel_lanes, s16_stream_kernel and
// s25_stream_kernel.

// =============================================================================================
// tg_step_stream_i8, S = 4: K steps in ONE launch for action blocks that arrive step by step.
// The dependent-launch boundary (1.55 us between two kernels of one stream) is what bounds the
// single-step entry at BASELINE config 2; a stepper that stays resident pays instead its own chain per step:
//   poll ready[k] (sc1 load) -> the 12 token bytes (sc1 loads: the producer is another kernel or the host) ->
//   8 packed MADs per slice -> state + done stored write-through (sc1) -> drain -> progress word (sc1 store).
// Games are independent, so there is NO barrier of any kind: the unit of work and of progress is the WAVEFRONT
// (16 games x NG, four lanes per game, the slices stay in VGPRs for all K steps).  Unit u = global wavefront index
// owns games [u * 16 NG, (u + 1) * 16 NG) and stores k + 1 into progress[u] once step k of its games is visible.
// Every spin is bounded: a wavefront whose ready word never arrives sets *status = 1 and leaves.
// =============================================================================================
struct StreamArgs {
  int8_t* state;
  const int8_t* actions;    // (K, B, 12) step-major
  uint8_t* done;            // (K, B)
  uint8_t* overflow;        // (B), nullable, sticky
  const uint32_t* ready;    // (K), nullable: all blocks valid at launch
  uint32_t* progress;       // (units), nullable
  uint32_t* status;         // (1), nullable
  int64_t B;
  int64_t stride;
  int K;
  int shift;
  uint32_t wait_ticks;  // how long a wavefront waits for a ready word: ticks of s_memrealtime (100 MHz)
};

// The ready-word protocol shared by the four resident steppers (D = steps a wavefront takes at once, <= 8).
// stream_released: how many of ready[kp], ready[kp + 1], ... are set without a gap, given lane's word in v (lanes < D,
// kp + lane < K); wave-uniform, <= D.
template <int D>
__device__ __forceinline__ int stream_released(const StreamArgs& a, uint32_t v, int kp, int lane) {
  const unsigned long long m = __ballot(lane < D && kp + lane < a.K && v != 0);
  return static_cast<int>(__builtin_ctzll(~m));
}
// stream_wait_released: poll until step kp is released (relaxed agent-scope loads: they bypass this CU's L1).  Bounded in
// TIME: the first miss starts a clock on s_memrealtime (100 MHz, one counter for the whole chip), after a.wait_ticks the
// wavefront sets *status and the caller leaves (returns 0).
template <int D>
__device__ __forceinline__ int stream_wait_released(const StreamArgs& a, int kp, int lane) {
  uint64_t t0 = 0;
  for (;;) {
    const uint32_t v = (lane < D && kp + lane < a.K) ? __hip_atomic_load(a.ready + kp + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const int n = stream_released<D>(a, v, kp, lane);
    if (n) return n;
    const uint64_t now = __builtin_amdgcn_s_memrealtime();
    if (t0 == 0) t0 = now;
    if (now - t0 >= a.wait_ticks) {
      if (lane == 0 && a.status) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return 0;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

template <int NG>
__global__ __launch_bounds__(kBlock) void s4_stream_kernel(StreamArgs a) {
  const int lane = threadIdx.x & 63, q = lane & 3, lg = lane >> 2;
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const int64_t g0 = unit * (16 * NG);
  if (g0 >= a.B) return;
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.state, 0, static_cast<int>(a.B * a.stride), 0x00027000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(a.done, 0, 0x7fffffff, 0x00027000);
  uint4 pk[NG];
  int64_t g[NG];
  bool live[NG];
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    g[n] = g0 + 16 * n + lg;
    live[n] = g[n] < a.B;
    if (!live[n]) g[n] = a.B - 1;  // dead lanes shadow the last game, stores predicated off
    pk[n] = *reinterpret_cast<const uint4*>(a.state + g[n] * a.stride + 16 * q);
  }
  // the slices stay biased for all K steps, each with its L1 norm (s4_step_biased); un-biased when they are stored
  uint32_t l1s[NG];
  int ovfs[NG];  // bits beyond the low byte: an entry left int8 (general form only); written out once per block
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    uint32_t xb[4];
    ovfs[n] = 0;
    l1s[n] = s4_digits_pre(pk[n], xb);
    pk[n] = uint4{xb[0], xb[1], xb[2], xb[3]};
  }
  const int dig_limit = s4_digits_limit(a.shift);
  // The step's chain, in BLOCKS (round 3).  It used to be, per step: poll ready[k] -> the tokens -> arithmetic ->
  // write-through drain -> progress: three memory round trips in a row.  Now a wavefront takes as many steps at once as
  // it has already SEEN released, up to D: the tokens of a block's D steps are requested together, right behind the
  // stores of the previous block (so that block's drain and this block's token round trip overlap), and a poll of the
  // NEXT block's D ready words travels with them.  One round trip per block instead of three per step; progress is
  // published per block.  A producer that releases block k + 1 only after progress[k] (the interactive case) is seen
  // as "one step released": blocks of one, progress per step, the serial order drain -> publish -> spin -> tokens.
  // Invariant: the tokens of step j are requested only after ready[j] was observed set (by an earlier poll).
  // The requests are asm loads with counted waits: vmcnt counts loads and stores together in issue order, so "all but
  // the loads behind them" is exactly the previous block's stores; hipcc's own bookkeeping would drain everything,
  // progress store included, at the loop header.  No asm load is in flight across the loop's back edge.
  // One dword per lane and step (lane q holds dword min(q, 2) of its game's twelve bytes; s4_team_token_bcast).
  static_assert(NG == 1 || NG == 2, "NG = 4 / 8 were retired with the one-game-per-lane kernel");
  constexpr int D = NG == 1 ? 8 : 4;
  uint32_t tk[D][NG], pollv = 0u;
  const uint32_t toff0 = static_cast<uint32_t>(g0 + lg) * 12u + 4u * static_cast<uint32_t>(q < 3 ? q : 2);
  const uint32_t toff_last = static_cast<uint32_t>(a.B - 1) * 12u + 4u * static_cast<uint32_t>(q < 3 ? q : 2);
  // poll of ready[kp + lane], lane < D (with_poll), then the tokens of steps kb .. kb + D - 1 (steps beyond K - 1 repeat
  // the last one; what lies beyond the released steps is loaded and never looked at): sc1 loads, the producer is another agent
  auto request = [&](int kb, int kp, bool with_poll) {
    if (with_poll) {
      const uint32_t* rp = a.ready + kp;
      const uint32_t poff = (lane < D && kp + lane < a.K) ? 4u * lane : 0u;
      asm volatile("global_load_dword %0, %1, %2 sc1" : "=&v"(pollv) : "v"(poff), "s"(rp) : "memory");
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int kd = kb + d < a.K ? kb + d : a.K - 1;
      const int8_t* blk = a.actions + static_cast<int64_t>(kd) * a.B * 12;
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        uint32_t off = toff0 + 192u * n;
        off = off < toff_last ? off : toff_last;  // dead lanes shadow the last game
        asm volatile("global_load_dword %0, %1, %2 sc1" : "=&v"(tk[d][n]) : "v"(off), "s"(blk) : "memory");
      }
    }
  };
  auto arrived = [&]() {  // after the wait that covers them: from here on the registers hold the loaded values
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int n = 0; n < NG; ++n) asm volatile("" : "+v"(tk[d][n]));
    asm volatile("" : "+v"(pollv));
  };
  // how many of ready[kp], ready[kp + 1], ... are set without a gap, given lane's word in v (lanes < D, kp + lane < K)
  auto released = [&](uint32_t v, int kp) { return stream_released<D>(a, v, kp, lane); };
  auto wait_released = [&](int kp) { return stream_wait_released<D>(a, kp, lane); };
  // (the state is in its registers before the first asm load: hipcc waits for its own loads with vmcnt(0) wherever it
  // thinks one may still be pending -- inside the loop that would be every block)
#pragma unroll
  for (int n = 0; n < NG; ++n) asm volatile("" : "+v"(pk[n].x), "+v"(pk[n].y), "+v"(pk[n].z), "+v"(pk[n].w));
  int kb = 0;                                         // first step of the block (uniform)
  int nb = a.ready ? wait_released(0) : (a.K < D ? a.K : D);  // its steps: released, not yet requested
  if (nb == 0) return;
  // STAGGER (round 4).  All resident wavefronts start together and do identical work, so they stay in lockstep: every
  // wavefront of a SIMD waits for its block's tokens at the same time and then all compute at once.  The FIRST block is cut
  // to 1 .. D steps by the workgroup's residency slot on its CU (consecutive workgroups go round the 8 XCDs, then round an
  // XCD's 32 CUs: blockIdx / 256 counts the slots), which spreads the wavefronts of a SIMD over the period: 0.776 -> 0.754 us
  // per step at 131 072 games with ready words, nothing without (same run, A/B).  What bounds this kernel at full occupancy
  // is the number of its small memory operations (the lane kernel below has the ablation), not the phase of its wavefronts.
  if constexpr (D > 1) {
    const int first = 1 + static_cast<int>((blockIdx.x >> 8) & (D - 1));
    nb = nb < first ? nb : first;
  }
  bool fresh = true;  // nothing stored since the last publish (the first block; after the serial order below)
  for (;;) {
    const bool with_poll = a.ready && kb + nb < a.K;  // uniform
    request(kb, kb + nb, with_poll);
    if (a.progress && !fresh) {  // the previous block's stores have left: publish its last step
      if (with_poll) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D * NG + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D * NG) : "memory");
      if (lane == 0) __hip_atomic_store(a.progress + unit, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // the tokens are in; only that progress store may be under way
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    arrived();
    // (round 4) per BLOCK: does any token byte of the team's steps exceed 3?  (lane q holds dword min(q, 2) of every step's
    // twelve bytes; steps beyond nb repeat valid ones, at worst they send a block through the general form needlessly)
    bool wide[NG];
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      uint32_t w = 0;
#pragma unroll
      for (int d = 0; d < D; ++d) w |= tk[d][n];
      wide[n] = quad_or(w & 0xFCFCFCFCu) != 0;
    }
    // one step of every game of the wavefront: done[k] from the team's summed L1 norms (two DPP adds); the overflow flags
    // are only ever raised inside the general form and leave once per block
    auto one_step = [&](int d) {
      const int k = kb + d;
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        uint32_t du, dv, dw;
        s4_team_token_bcast(tk[d][n], du, dv, dw);
        s4_step_biased_blk(pk[n], l1s[n], du, dv, dw, q, a.shift, dig_limit, wide[n], ovfs[n]);
        const uint32_t team_l1 = quad_sum(l1s[n]);
        if (live[n] && q == 0)  // write-through (sc1) stores: visible to other agents once this wavefront's vmcnt drains
          __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(team_l1 == 0 ? 1 : 0), drs,
                                               static_cast<int>(static_cast<int64_t>(k) * a.B + g[n]), 0, 16);
      }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (d >= nb) break;  // uniform
      one_step(d);
    }
    if (a.overflow) {
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        if (__builtin_expect(quad_or(static_cast<uint32_t>(ovfs[n]) & ~255u) != 0, 0)) {
          if (live[n] && q == 0) a.overflow[g[n]] = 1;
          ovfs[n] = 0;  // (sticky in memory: raised once is enough)
        }
      }
    }
    // the state leaves once per block, as whole 64-byte games (16 games of a wavefront: 1 KiB in a row): nobody may
    // look at it before the block's progress word, and a block of one -- the interactive case -- is the old per-step store
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      typedef unsigned int tg_u32x4 __attribute__((ext_vector_type(4)));
      if (live[n])
        __builtin_amdgcn_raw_buffer_store_b128(tg_u32x4{pk[n].x ^ 0x80808080u, pk[n].y ^ 0x80808080u, pk[n].z ^ 0x80808080u,
                                                        pk[n].w ^ 0x80808080u}, srs,
                                               static_cast<int>(g[n] * a.stride) + 16 * q, 0, 16);
    }
    kb += nb;
    fresh = false;
    if (kb >= a.K) break;
    nb = a.ready ? released(pollv, kb) : (a.K - kb < D ? a.K - kb : D);
    if (nb == 0) {  // nothing released beyond this block yet: the serial order
      if (a.progress) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.progress + unit, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      fresh = true;
      nb = wait_released(kb);
      if (nb == 0) return;
    }
  }
  if (a.progress) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's last stores have left
    if (lane == 0) __hip_atomic_store(a.progress + unit, static_cast<uint32_t>(a.K), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// =============================================================================================
// tg_step_stream_i8, S = 4, ONE GAME PER LANE (round 4).  Ablation of s4_stream_kernel<1> at BASELINE config 4's share
// (131 072 games resident, tools/stream_ablate.sh): without its arithmetic 0.77 of 0.84 us per step, without the done
// stores 0.57, without any store 0.49 -- the stepper is bound by the NUMBER of small memory operations (a 16-lane byte
// store and a 192-byte token load per 16 games and step, write-through), not by its instructions.  Here a lane owns a
// whole game (sixteen biased dwords X[i][j], the digits are the l index) and a wavefront 64 games:
//   tokens  one global_load_dwordx3 per lane and step: 768 contiguous bytes per wavefront (were 4 x 192);
//   done    one 64-byte row per wavefront and step (were 4 x 16 bytes);
//   state   once per block, transposed through 4 KiB of LDS per wavefront so that every store instruction writes 1 KiB
//           in a row (lane-strided 16-byte pieces would be partial lines);
//   VALU    per step 4 + 4 byte extractions, 4 products G_i = -u_i W, 16 multiply-adds X[i][j] += v_j G_i, 16 v_sad_u8:
//           ~48 instructions for 64 games (the four-lanes-per-game form: ~27 for 16).
// A step some lane's digit form does not cover (tokens > 3, entries near the int8 range, other shifts) is taken by the
// WHOLE wavefront through the general form on an LDS image of its games (s4_step_slice per slice, rolled): exact, rare.
// Protocol (ready / progress / status, blocks of up to D released steps, counted waits) as s4_stream_kernel.
// =============================================================================================
__global__ __launch_bounds__(kBlock) void s4_stream_kernel_lanes(StreamArgs a) {
  typedef unsigned int tg_u32x3 __attribute__((ext_vector_type(3)));
  typedef unsigned int tg_u32x4 __attribute__((ext_vector_type(4)));
  constexpr int D = 8, NW = kBlock / 64;
  constexpr uint32_t BIAS = 0x80808080u;
  constexpr int kDropped = static_cast<int>(0x80000000u);  // a buffer offset beyond every range: the store is dropped
  __shared__ __attribute__((aligned(16))) uint32_t img[NW][64 * 16];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * NW + wave;
  const int64_t g0 = unit * 64;
  if (g0 >= a.B) return;
  // (range-checked buffers: a dead lane's store goes to kDropped instead of being branched around, so the number of
  // memory operations a block issues is exact -- the counted waits below depend on it)
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.state, 0, static_cast<int>(a.B * a.stride), 0x00027000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(a.done, 0, static_cast<int>(static_cast<int64_t>(a.K) * a.B), 0x00027000);
  const bool live = g0 + lane < a.B;
  const int64_t g = live ? g0 + lane : a.B - 1;  // dead lanes shadow the last game
  uint32_t* const row = &img[wave][lane * 16];
  uint32_t x[16];
  {
    const int8_t* src = a.state + g * a.stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + 16 * i);
      x[4 * i] = v.x ^ BIAS, x[4 * i + 1] = v.y ^ BIAS, x[4 * i + 2] = v.z ^ BIAS, x[4 * i + 3] = v.w ^ BIAS;
    }
  }
  auto norm = [&]() {
    uint32_t s0 = 0, s1 = 0;
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
      s0 = __builtin_amdgcn_sad_u8(x[e], BIAS, s0);
      s1 = __builtin_amdgcn_sad_u8(x[e + 1], BIAS, s1);
    }
    return s0 + s1;
  };
  uint32_t l1 = norm();
  int ovf = 0;
  const int dig_limit = s4_digits_limit(a.shift);
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  // TWO sets of token registers: while the block in tkA is worked on, the next block's tokens travel into tkB (a wavefront
  // alone on its SIMD -- 65 536 games -- otherwise waits a memory round trip per block with nothing to issue)
  tg_u32x3 tkA[D], tkB[D];
  uint32_t pollv = 0u;
  const uint32_t toff = static_cast<uint32_t>(g) * 12u;
  // poll of ready[kp + lane], lane < D (with_poll), then the tokens of steps kb .. kb + D - 1 (steps beyond K - 1 repeat the
  // last one; what lies beyond the released steps is loaded and at most OR-ed into the block's `wide` test)
  auto request = [&](tg_u32x3 (&tk)[D], int kb, int kp, bool with_poll) {
    if (with_poll) {
      const uint32_t* rp = a.ready + kp;
      const uint32_t poff = (lane < D && kp + lane < a.K) ? 4u * lane : 0u;
      asm volatile("global_load_dword %0, %1, %2 sc1" : "=&v"(pollv) : "v"(poff), "s"(rp) : "memory");
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int kd = kb + d < a.K ? kb + d : a.K - 1;
      const int8_t* blk = a.actions + static_cast<int64_t>(kd) * a.B * 12;
      asm volatile("global_load_dwordx3 %0, %1, %2 sc1" : "=&v"(tk[d]) : "v"(toff), "s"(blk) : "memory");
    }
  };
  auto arrived = [&](tg_u32x3 (&tk)[D]) {  // behind the wait that covers them: from here on the registers hold the loaded values
#pragma unroll
    for (int d = 0; d < D; ++d) asm volatile("" : "+v"(tk[d]));
    asm volatile("" : "+v"(pollv));
  };
  auto released = [&](uint32_t v, int kp) { return stream_released<D>(a, v, kp, lane); };
  auto wait_released = [&](int kp) { return stream_wait_released<D>(a, kp, lane); };
  auto publish = [&](int k) {
    if (lane == 0) __hip_atomic_store(a.progress + unit, static_cast<uint32_t>(k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  // how many steps the block behind step kn - 1 has, from the poll that travelled with the block before it
  auto next_size = [&](int kn) {
    if (kn >= a.K) return 0;
    return a.ready ? released(pollv, kn) : (a.K - kn < D ? a.K - kn : D);
  };
  // the digit form of one step for the lane's game
  auto fast_step = [&](const tg_u32x3& t) {
    const uint32_t W = t.z - shrep;
    uint32_t G[4], vj[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) G[i] = mul_lo_mad(static_cast<uint32_t>(a.shift) - ((t.x >> (8 * i)) & 255u), W);
    asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(vj[0]) : "v"(t.y), "s"(a.shift));
    asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(vj[1]) : "v"(t.y), "s"(a.shift));
    asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(vj[2]) : "v"(t.y), "s"(a.shift));
    asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(vj[3]) : "v"(t.y), "s"(a.shift));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) x[4 * i + j] += vj[j] * G[i];
    l1 = norm();
  };
  // the general form of one step for every game of the wavefront, on an LDS image (each lane touches its own row only)
  auto general_step = [&](const tg_u32x3& t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4*>(row + 4 * i) = uint4{x[4 * i] ^ BIAS, x[4 * i + 1] ^ BIAS, x[4 * i + 2] ^ BIAS, x[4 * i + 3] ^ BIAS};
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      uint32_t nz = 0;
      const uint4 r = s4_step_slice(*reinterpret_cast<const uint4*>(row + 4 * i), t.x, t.y, t.z, i, a.shift, nz, ovf);
      *reinterpret_cast<uint4*>(row + 4 * i) = r;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + 4 * i);
      x[4 * i] = v.x ^ BIAS, x[4 * i + 1] = v.y ^ BIAS, x[4 * i + 2] = v.z ^ BIAS, x[4 * i + 3] = v.w ^ BIAS;
    }
    l1 = norm();
  };
#pragma unroll
  for (int e = 0; e < 16; ++e) asm volatile("" : "+v"(x[e]));  // the state is in its registers before the first asm load
  int kb = 0;                                                    // first step of the block in tkA (uniform)
  int nb = a.ready ? wait_released(0) : (a.K < D ? a.K : D);     // its steps
  if (nb == 0) return;
  int nb_next = 0;       // steps of the block behind it, as far as they were SEEN released
  int pub = 0;           // > 0: steps [.., pub) are stored but not yet published
  bool have = false;     // tkA holds this block's tokens
  for (;;) {
    if (!have) {  // the serial order (first block; after a spin): request, drain everything, publish what was pending
      request(tkA, kb, kb + nb, a.ready && kb + nb < a.K);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      arrived(tkA);
      if (a.progress && pub) publish(pub);
      pub = 0;
      nb_next = next_size(kb + nb);
    }
    // ---- the next block's tokens set off before this block is worked on (only steps SEEN released are ever requested)
    const int kn = kb + nb;
    const bool pf = nb_next > 0;                              // uniform
    const bool poll2 = a.ready && kn + nb_next < a.K;         // uniform
    if (pf) request(tkB, kn, kn + nb_next, poll2);
    // ---- this block: does any token byte of the lane's steps exceed 3?
    uint32_t wq = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) wq |= tkA[d].x | tkA[d].y | tkA[d].z;
    const bool wide = (wq & 0xFCFCFCFCu) != 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (d >= nb) break;  // uniform
      if (__builtin_expect(__ballot(wide || static_cast<int>(l1) > dig_limit) != 0, 0)) general_step(tkA[d]);
      else fast_step(tkA[d]);
      // write-through (sc1) stores: visible to other agents once this wavefront's vmcnt drains
      __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(l1 == 0 ? 1 : 0), drs,
                                           live ? static_cast<int>(static_cast<int64_t>(kb + d) * a.B + g) : kDropped, 0, 16);
    }
    if (a.overflow && __builtin_expect(__ballot((ovf & ~255) != 0) != 0, 0)) {  // (one more store than counted: the waits then
      if (live && (ovf & ~255)) a.overflow[g] = 1;                               // cover one operation more than they need to)
      ovf = 0;  // sticky in memory: raised once is enough
    }
    // the state leaves once per block, transposed through LDS: chunk c = lane + 64 r is 16-byte piece c & 3 of game c >> 2
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<uint4*>(row + 4 * i) = uint4{x[4 * i] ^ BIAS, x[4 * i + 1] ^ BIAS, x[4 * i + 2] ^ BIAS, x[4 * i + 3] ^ BIAS};
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = lane + 64 * r;
      const uint4 v = *reinterpret_cast<const uint4*>(&img[wave][4 * c]);
      const int64_t gg = g0 + (c >> 2);
      __builtin_amdgcn_raw_buffer_store_b128(tg_u32x4{v.x, v.y, v.z, v.w}, srs,
                                             gg < a.B ? static_cast<int>(gg * a.stride) + 16 * (c & 3) : kDropped, 0, 16);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- in flight now, oldest first: [stores of the block before] [tkB's L = D (+1) loads] [this block's nb + 4 stores]
    const bool whole = nb == D;  // (a partial block -- the last one, or a producer releasing step by step -- drains instead)
    if (a.progress && pub) {  // the block before is visible once everything older than tkB's loads has left
      if (!whole || !pf) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (poll2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + 1 + D + 4) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + D + 4) : "memory");
      publish(pub);
      pub = 0;
      if (pf) {  // tkB: older than this block's D + 4 stores and that progress store
        if (whole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + 4 + 1) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    } else if (pf) {
      if (whole) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + 4) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    pub = kn;
    kb = kn;
    if (kb >= a.K) break;
    if (pf) {
      arrived(tkB);
#pragma unroll
      for (int d = 0; d < D; ++d) tkA[d] = tkB[d];
      nb = nb_next;
      nb_next = next_size(kb + nb);
      have = true;
    } else {  // nothing seen released beyond this block: drain, publish, spin
      if (a.progress) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        publish(pub);
      }
      pub = 0;
      nb = wait_released(kb);
      if (nb == 0) return;
      have = false;
    }
  }
  if (a.progress) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's last stores have left
    publish(a.K);
  }
}

// =============================================================================================
// tg_step_stream_i8, S = 16: one wavefront per game, resident for all K steps, the game in REGISTERS -- sixteen VGPRs of biased
// state per lane (lane (r, j) holds rows (i = r + 4 n, j)); 8192 games = 32 wavefronts per CU on 256 CUs: all resident at
// <= 64 VGPRs.  Every step updates all four rows of a lane in the digit form -- no queue, no LDS image, no divergent dense
// pass; the L1 norm of a new row is this step's zero test and the next step's precondition (one bit per row); the game
// is written through once per block.  Rows the digit form does not cover take the packed int16 form inline.
// (Round 2 kept the state in registers too but compacted candidate rows through an LDS queue and OR-ed all sixteen
// registers per step: 3.35 us per step at BASELINE config 3; round 3's first form -- the tracked step on an LDS image of the
// game -- 2.27; this one 1.76: with the biased state a row costs four multiply-adds, four adds and four v_sad_u8, which is
// less than finding out which rows to skip.)
// =============================================================================================
__global__ __launch_bounds__(kBlock, 8) void s16_stream_kernel(StreamArgs a) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr int NW = kBlock / 64;
  constexpr uint32_t BIAS = 0x80808080u;
  constexpr int D = 8;                                         // steps per block (below)
  __shared__ __attribute__((aligned(16))) uint32_t tokbuf[NW][D][12];  // the block's tokens: 48 bytes per step
  const int lane = threadIdx.x & 63;
  // the game index is wave-uniform; say so (readfirstlane): its token and flag addresses stay on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t g = static_cast<int64_t>(blockIdx.x) * NW + wave;
  if (g >= a.B) return;
  const int r = lane >> 4;
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.state, 0, static_cast<int>(a.B * a.stride), 0x00027000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(a.done, 0, 0x7fffffff, 0x00027000);
  const int soff = static_cast<int>(g * a.stride);
  // ---- the game -> registers, biased (x ^ 0x80808080): lane (r, j) holds rows (i = r + 4 n, j) = chunks lane + 64 n ----
  auto l1_of = [&](const uint4& q) {
    return static_cast<int>(__builtin_amdgcn_sad_u8(q.w, BIAS, __builtin_amdgcn_sad_u8(q.z, BIAS,
                            __builtin_amdgcn_sad_u8(q.y, BIAS, __builtin_amdgcn_sad_u8(q.x, BIAS, 0u)))));
  };
  const int limit = s4_digits_limit(a.shift);
  uint4 x[4];
  uint32_t okbits = 0;  // bit n: row n's L1 norm <= limit (the digit form's precondition for the next step)
  {
    const int8_t* const src = a.state + g * a.stride + 16 * lane;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + 1024 * n);
      x[n] = uint4{q.x ^ BIAS, q.y ^ BIAS, q.z ^ BIAS, q.w ^ BIAS};
      okbits |= (l1_of(x[n]) <= limit ? 1u : 0u) << n;
    }
  }
  const uint32_t shp = (static_cast<uint32_t>(a.shift) & 0xFFFFu) | (static_cast<uint32_t>(a.shift) << 16);
  const bool wide_shift = static_cast<unsigned>(a.shift + 127) > 254u;  // uniform; factors may exceed 255
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  // The step's chain runs in BLOCKS as in s4_stream_kernel: up to D steps the wavefront has seen released are taken at
  // once -- their tokens requested together right behind the previous block's stores, with the poll of the next block's
  // ready words; asm loads (sc1: the producer is another agent), counted waits, nothing in flight across the back edge.
  // ONE dword per lane and step -- lane l < 12 asks for dword l of the step's 48 token bytes -- staged through LDS once
  // they are in, so that the steps run as a rolled loop (one copy of the code, no token registers live across it): a
  // step reads u and w back as two uniform 16-byte reads (on to the scalar unit: they are the same for the whole
  // wavefront) and its v_j as a byte.
  uint32_t tk[D], pollv = 0u;
  const uint32_t tk_off = 4u * (lane < 12 ? lane : 11);
  auto tokens_of = [&](int k) { return a.actions + (static_cast<int64_t>(k) * a.B + g) * 48; };
  auto request = [&](int kb, int kp, bool with_poll) {
    if (with_poll) {
      const uint32_t* rp = a.ready + kp;
      const uint32_t poff = (lane < D && kp + lane < a.K) ? 4u * lane : 0u;
      asm volatile("global_load_dword %0, %1, %2 sc1" : "=&v"(pollv) : "v"(poff), "s"(rp) : "memory");
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {  // (steps beyond K - 1 repeat the last one; what lies beyond the released steps is never looked at)
      const int8_t* tp = tokens_of(kb + d < a.K ? kb + d : a.K - 1);
      asm volatile("global_load_dword %0, %1, %2 sc1" : "=&v"(tk[d]) : "v"(tk_off), "s"(tp) : "memory");
    }
  };
  auto arrived = [&]() {
#pragma unroll
    for (int d = 0; d < D; ++d) asm volatile("" : "+v"(tk[d]));
    asm volatile("" : "+v"(pollv));
    if (lane < 12) {
#pragma unroll
      for (int d = 0; d < D; ++d) tokbuf[wave][d][lane] = tk[d];
    }
    __builtin_amdgcn_wave_barrier();  // (LDS serves one wavefront's accesses in order)
  };
  auto released = [&](uint32_t v, int kp) { return stream_released<D>(a, v, kp, lane); };
  auto wait_released = [&](int kp) { return stream_wait_released<D>(a, kp, lane); };
  // (the state is in its registers before the first asm load, or hipcc waits for it -- with vmcnt(0) -- inside the loop)
#pragma unroll
  for (int n = 0; n < 4; ++n) asm volatile("" : "+v"(x[n].x), "+v"(x[n].y), "+v"(x[n].z), "+v"(x[n].w));
  // one step, its tokens in slot d of the block: EVERY row of the lane in the digit form (no compaction: four rows of
  // sixteen bytes, one product -u_i v_j each, the weight integers on the scalar unit)
  auto step = [&](int k, int d) {
    const uint4 u4 = *reinterpret_cast<const uint4*>(&tokbuf[wave][d][0]), w4 = *reinterpret_cast<const uint4*>(&tokbuf[wave][d][8]);
    const uint32_t vdw = tokbuf[wave][d][4 + ((lane & 15) >> 2)];
    const uint32_t us[4] = {static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(u4.x))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(u4.y))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(u4.z))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(u4.w)))};
    const uint32_t ws[4] = {static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(w4.x))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(w4.y))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(w4.z))),
                            static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(w4.w)))};
    const int vj = __builtin_amdgcn_sbfe(static_cast<int>(vdw), 8 * (lane & 3), 8) - a.shift;
    auto wfetch = [&]() { return uint4{ws[0], ws[1], ws[2], ws[3]}; };  // (the 32-bit redo only)
    uint32_t ovf = 0;
    const uint32_t uw_or = us[0] | us[1] | us[2] | us[3] | ws[0] | ws[1] | ws[2] | ws[3];
    const bool small = (uw_or & 0xFCFCFCFCu) == 0 && __ballot((vdw & 0xFCFCFCFCu) != 0) == 0;  // all 48 tokens <= 3 (uniform)
    const uint32_t Wd[4] = {ws[0] - shrep, ws[1] - shrep, ws[2] - shrep, ws[3] - shrep};
    // X + uvn * Wd per dword: v_mad_u64_u32 from the inline constant 0 (full rate; no register pair to set up) and an add
    auto fast_row = [&](const uint4& xb, int uvn) {
      auto dig = [&](uint32_t xd, uint32_t w) {
        uint64_t rr;
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(rr) : "v"(uvn), "s"(w) : "vcc");
        return xd + static_cast<uint32_t>(rr);
      };
      return uint4{dig(xb.x, Wd[0]), dig(xb.y, Wd[1]), dig(xb.z, Wd[2]), dig(xb.w, Wd[3])};
    };
    // a row the digit form does not cover: un-bias, the packed int16 form (32-bit redo behind it), bias again
    auto slow_row = [&](const uint4& xb, int uvn) {
      uint32_t w0 = ws[0], w1 = ws[1], w2 = ws[2], w3 = ws[3];
      asm volatile("" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3));  // (or hipcc builds the weight pairs on the common path)
      uint32_t wp[8], cnz;
      unpack_pairs(uint4{w0, w1, w2, w3}, wp);
#pragma unroll
      for (int p = 0; p < 8; ++p) wp[p] = pk_sub_i16(wp[p], shp);
      const uint4 r4 = s16_chunk(uint4{xb.x ^ BIAS, xb.y ^ BIAS, xb.z ^ BIAS, xb.w ^ BIAS}, uvn, wp, wfetch, a.shift, wide_shift, cnz, ovf);
      return uint4{r4.x ^ BIAS, r4.y ^ BIAS, r4.z ^ BIAS, r4.w ^ BIAS};
    };
    const bool all_fast = small && __ballot((okbits & 15u) != 15u) == 0;  // uniform
    uint32_t l1tot = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(us[n]), 8 * r, 8);  // -(u_i), i = r + 4 n
      const int uvn = __mul24(ui, vj);  // (|factor| <= 255 here: full rate, v_mul_lo_u32 is a quarter-rate instruction)
      if (__builtin_expect(all_fast, 1)) x[n] = fast_row(x[n], uvn);
      else if (small && ((okbits >> n) & 1u)) x[n] = fast_row(x[n], uvn);
      else if (uvn != 0) x[n] = slow_row(x[n], uvn);
      const int l1 = l1_of(x[n]);
      l1tot += static_cast<uint32_t>(l1);
      okbits = l1 <= limit ? okbits | (1u << n) : okbits & ~(1u << n);
    }
    const bool any_nz = __ballot(l1tot != 0) != 0;
    if (lane == 0)
      __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(any_nz ? 0 : 1), drs,
                                           static_cast<int>(static_cast<int64_t>(k) * a.B + g), 0, 16);
    if (__builtin_expect(ovf != 0, 0) && a.overflow) a.overflow[g] = 1;
  };
  // the game leaves once per block (write-through, sc1), as in s4_stream_kernel
  auto put_state = [&]() {
#pragma unroll
    for (int n = 0; n < 4; ++n)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{x[n].x ^ BIAS, x[n].y ^ BIAS, x[n].z ^ BIAS, x[n].w ^ BIAS}, srs,
                                             soff + 16 * (lane + 64 * n), 0, 16);
  };
  int kb = 0;                                                  // first step of the block (uniform)
  int nb = a.ready ? wait_released(0) : (a.K < D ? a.K : D);   // its steps: released, not yet requested
  if (nb == 0) return;
  bool fresh = true;  // nothing stored since the last publish
  for (;;) {
    const bool with_poll = a.ready && kb + nb < a.K;  // uniform
    request(kb, kb + nb, with_poll);
    if (a.progress && !fresh) {  // the previous block's stores have left: publish its last step
      if (with_poll) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D) : "memory");
      if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // the tokens are in; only that progress store may be under way
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    arrived();
#pragma unroll 1
    for (int d = 0; d < nb; ++d) step(kb + d, d);
    put_state();
    kb += nb;
    fresh = false;
    if (kb >= a.K) break;
    nb = a.ready ? released(pollv, kb) : (a.K - kb < D ? a.K - kb : D);
    if (nb == 0) {  // nothing released beyond this block yet: the serial order
      if (a.progress) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      fresh = true;
      nb = wait_released(kb);
      if (nb == 0) return;
    }
  }
  if (a.progress) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's last stores have left
    if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(a.K), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// =============================================================================================
// tg_step_stream_i8, S = 25 (round 3): one wavefront per game with the game's 15 625 bytes in REGISTERS for all K steps --
// 80 VGPRs of state per lane, four wavefronts per SIMD: 4 096 games (BASELINE config 5's share of one GPU) are resident at
// once on 256 CUs (LDS could hold 2 560).  Registers cannot be indexed by a lane, so nothing is compacted: every step
// touches all twenty 16-byte chunks of every lane -- in the digit form, with the state kept BIASED (x ^ 0x80808080) between
// steps so that a chunk costs eight multiply-adds, four v_sad_u8 (the new L1 norm: the zero test of this step and the
// precondition of the next, remembered as one bit per chunk) and a compare.
// Layout (the period trick of packed_kernel): lane t < 50 owns chunks t + 50 n, n < 20 (16 * 50 = 800 = 32 rows): its
// 16-byte window starts at byte s = 16 t mod 25 of row r0 = floor(16 t / 25) + 32 n and runs into row r0 + 1 when s > 9 --
// s and the split are lane constants, so the two masked weight integers per dword (W0: the window's bytes in row r0, W1:
// those in row r0 + 1) are built once per step and a chunk needs only its two products -u_i v_j, read from a per-step
// table in LDS at a compile-time offset.  X' = X + uv0 * W0 + uv1 * W1 per dword; exact while no digit leaves [0, 255],
// guaranteed by: all 75 tokens <= 3 and 0 <= shift <= 3 (uniform) and the chunk's L1 norm <= 127 - F^3 (per chunk: the
// bit).  A chunk without its bit is done byte by byte in 32-bit (wrap + overflow flag) by its lane, inline.
// Steps come in blocks, tokens staged through LDS, state written through once per block -- as in s16_stream_kernel.
// =============================================================================================
__global__ __launch_bounds__(kBlock, 4) void s25_stream_kernel(StreamArgs a) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  constexpr int NW = kBlock / 64, D = 8, NSLOT = 20, NCH = 977, TL = 50;
  constexpr uint32_t BIAS = 0x80808080u;
  __shared__ int uvt[NW][656];                                          // -u_i v_j per row 25 i + j; 0 from row 625 on
  __shared__ __attribute__((aligned(4))) uint8_t wext[NW][56];          // the w tokens, periodically extended
  __shared__ __attribute__((aligned(16))) uint32_t tokbuf[NW][D][64];   // the block's tokens: 75 bytes per step (a row per LDS-DMA)
  __shared__ __attribute__((aligned(16))) uint32_t pollbuf[NW][64];     // the next block's ready words
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t g = static_cast<int64_t>(blockIdx.x) * NW + wave;
  if (g >= a.B) return;
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(a.state, 0, static_cast<int>(a.B * a.stride), 0x00027000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(a.done, 0, 0x7fffffff, 0x00027000);
  const int soff = static_cast<int>(g * a.stride);
  const bool act = lane < TL;
  const uint32_t shrep = static_cast<uint32_t>(a.shift) * 0x01010101u;
  const int limit = s4_digits_limit(a.shift);
  auto l1_of = [&](const uint4& q) {
    return static_cast<int>(__builtin_amdgcn_sad_u8(q.w, BIAS, __builtin_amdgcn_sad_u8(q.z, BIAS,
                            __builtin_amdgcn_sad_u8(q.y, BIAS, __builtin_amdgcn_sad_u8(q.x, BIAS, 0u)))));
  };
  // ---- the game -> registers, biased; the padding behind byte 15 624 (chunk 976 = lane 26, slot 19) is held as zero ----
  uint4 x[NSLOT];
  uint32_t okbits = 0;
  {
    const int8_t* const src = a.state + g * a.stride;
#pragma unroll
    for (int n = 0; n < NSLOT; ++n) {
      const int c = lane + TL * n;
      uint4 q{0, 0, 0, 0};
      if (act && c < NCH) q = *reinterpret_cast<const uint4*>(src + 16 * c);
      if (n == NSLOT - 1 && lane == NCH - 1 - TL * (NSLOT - 1)) {
        q.z &= 0xFFu;
        q.w = 0;
      }
      x[n] = uint4{q.x ^ BIAS, q.y ^ BIAS, q.z ^ BIAS, q.w ^ BIAS};
      okbits |= (l1_of(x[n]) <= limit ? 1u : 0u) << n;
    }
  }
  // Token requests by LDS-DMA (global_load_lds_dword: lane l's dword lands at the row's base + 4 l, no VGPR destination): this
  // kernel runs at its register limit, and a register that an asm load has yet to fill may be copied or spilled by hipcc
  // before the data is there -- LDS cannot.  Counted waits as in the other steppers; M0 (the DMA's LDS base) is saved
  // and restored inside the statement.
  // The DMA moves ALIGNED dwords: a step's 75 token bytes start at any byte address A, so lane l < nd asks for dword l of
  // [A - (A & 3), ...), nd = ceil(((A & 3) + 75) / 4) = 19 or 20, and the step reads its token i at byte (A & 3) + i of the row
  // (actions is 4-byte aligned: nothing in front of the buffer is touched, and behind it at most the rest of the dword that
  // holds the last token -- a fixed 20 dwords would ask for [end, end + 4) of the last game's last step when A & 3 <= 1).
  auto tokens_of = [&](int k) { return a.actions + (static_cast<int64_t>(k) * a.B + g) * 75; };
  auto dma = [&](const void* base, uint32_t voff, const void* lds_row) {
    const uint32_t dst = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_row));
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, %3 sc1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(dst), "v"(voff), "s"(base) : "memory");
  };
  auto request = [&](int kb, int kp, bool with_poll) {
    if (with_poll) dma(a.ready + kp, (lane < D && kp + lane < a.K) ? 4u * lane : 0u, &pollbuf[wave][0]);
#pragma unroll 1
    for (int d = 0; d < D; ++d) {
      const uintptr_t A = reinterpret_cast<uintptr_t>(tokens_of(kb + d < a.K ? kb + d : a.K - 1));
      const uint32_t nd = (static_cast<uint32_t>(A & 3) + 75u + 3u) >> 2;  // dwords that hold this step's 75 tokens
      dma(reinterpret_cast<const void*>(A & ~static_cast<uintptr_t>(3)), static_cast<uint32_t>(lane) < nd ? 4u * lane : 0u,
          &tokbuf[wave][d][0]);
    }
  };
  auto arrived = [&]() { __builtin_amdgcn_wave_barrier(); };  // behind the counted wait: the rows are in LDS
  auto released = [&](uint32_t v, int kp) { return stream_released<D>(a, v, kp, lane); };
  auto wait_released = [&](int kp) { return stream_wait_released<D>(a, kp, lane); };
  // (the state is in its registers before the first asm load, or hipcc waits for it -- with vmcnt(0) -- inside the loop)
#pragma unroll
  for (int n = 0; n < NSLOT; ++n) asm volatile("" : "+v"(x[n].x), "+v"(x[n].y), "+v"(x[n].z), "+v"(x[n].w));

  // one step, its tokens in slot d of the block
  auto step = [&](int k, int d) {
    // (the lane constants are worked out again in every step, from a lane index hipcc cannot see through: hoisted out of
    // the step loop -- sixteen masks and offsets -- they went to scratch, and every step waited for twenty reloads in a row)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const bool act = ln < TL;
    const int ws = (16 * ln) % 25, r0l = (16 * ln) / 25, k0 = 25 - ws;
    const uint32_t actm = act ? ~0u : 0u;
    const int lane = ln;
    const uint8_t* const tb = reinterpret_cast<const uint8_t*>(&tokbuf[wave][d][0]) + (reinterpret_cast<uintptr_t>(tokens_of(k)) & 3);
    // ---- per-step tables: -u_i v_j for the 625 rows, the extended w, the lane's weight integers ----
    struct __attribute__((packed)) U32 { uint32_t v; };
    uint32_t uw[7], uw_or = 0;  // u's bytes 0..27 on the scalar unit (bytes 25..27 are v tokens)
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      uw[i] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(reinterpret_cast<const U32*>(tb + 4 * i)->v)));
      uw_or |= uw[i];
    }
    const int vtok = static_cast<int8_t>(tb[25 + (lane < 25 ? lane : (lane < TL ? lane - 25 : 0))]);
    const int wtok = static_cast<int8_t>(tb[50 + lane % 25]);
    const int vj = vtok - a.shift;
    // are all 75 tokens <= 3?  (uniform)
    const bool small = (uw_or & 0xFCFCFCFCu) == 0 && __ballot(((vtok | wtok) & ~3) != 0) == 0;
#pragma unroll
    for (int m = 0; m < 13; ++m) {  // rows 2 m (lanes 0..24) and 2 m + 1 (lanes 25..49); "row 25" gives the zeros behind the table
      const int ua = sbyte(uw[(2 * m) >> 2], (2 * m) & 3);
      const int ub = 2 * m + 1 < 25 ? sbyte(uw[(2 * m + 1) >> 2], (2 * m + 1) & 3) : a.shift;
      const int ui = a.shift - (lane < 25 ? ua : ub);
      if (act) uvt[wave][TL * m + lane] = __mul24(ui, vj);
    }
    if (lane < 56) wext[wave][lane] = static_cast<uint8_t>(wtok);
    __builtin_amdgcn_wave_barrier();
    uint32_t W0[4], W1[4];
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
      const uint8_t* wp = &wext[wave][ws + 4 * dd];
      const uint32_t wq = static_cast<uint32_t>(wp[0]) | (static_cast<uint32_t>(wp[1]) << 8) | (static_cast<uint32_t>(wp[2]) << 16) |
                          (static_cast<uint32_t>(wp[3]) << 24);
      // byte masks: the window's bytes in row r0 / in row r0 + 1 (both 0 in the idle lanes: their weights are 0)
      const int nbr = k0 - 4 * dd;
      const uint32_t mk0 = (nbr <= 0 ? 0u : (nbr >= 4 ? ~0u : ((1u << (8 * nbr)) - 1u))) & actm, mk1 = ~mk0 & actm;
      W0[dd] = (wq & mk0) - (shrep & mk0);
      W1[dd] = (wq & mk1) - (shrep & mk1);
    }
    bool ovf_any = false;  // uniform (kept off the vector registers: the kernel has none to spare)
    // a chunk byte by byte (its precondition failed, or the step's tokens are not small): exact, wrapped, flagged
    auto slow_chunk = [&](const uint4& xb, int uv0, int uv1) {
      uint32_t q0 = xb.x ^ BIAS, q1 = xb.y ^ BIAS, q2 = xb.z ^ BIAS, q3 = xb.w ^ BIAS, ovf = 0;
      if (!act) uv0 = 0, uv1 = 0;
#pragma unroll 1
      for (int it = 0; it < 4; ++it) {
        uint32_t o = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int b = 4 * it + t;
          const int wv = static_cast<int>(static_cast<int8_t>(wext[wave][ws + b])) - a.shift;
          const int e = sbyte(q0, t) + __mul24(b < k0 ? uv0 : uv1, wv);  // (|u_i v_j| < 2^17, |w_l| <= 255)
          ovf |= static_cast<uint32_t>(e + 128) & ~255u;
          o |= (static_cast<uint32_t>(e) & 255u) << (8 * t);
        }
        q0 = q1, q1 = q2, q2 = q3, q3 = o;  // (rotation: no register is indexed by the loop counter)
      }
      ovf_any |= ovf != 0;
      return uint4{q0 ^ BIAS, q1 ^ BIAS, q2 ^ BIAS, q3 ^ BIAS};
    };
    auto fast_chunk = [&](const uint4& xb, int uv0, int uv1) {
      auto dig = [&](uint32_t xd, uint32_t w0, uint32_t w1) {
        uint64_t r;
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, 0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0" : "=&v"(r) : "v"(uv0), "v"(w0), "v"(uv1), "v"(w1) : "vcc");
        return xd + static_cast<uint32_t>(r);
      };
      uint4 o;
      o.x = dig(xb.x, W0[0], W1[0]);
      o.y = dig(xb.y, W0[1], W1[1]);
      o.z = dig(xb.z, W0[2], W1[2]);
      o.w = dig(xb.w, W0[3], W1[3]);
      return o;
    };
    // does every chunk of every lane have its bit (and the step small tokens)?  (uniform)
    const bool all_fast = small && __ballot((okbits & 0xFFFFFu) != 0xFFFFFu) == 0;
    uint32_t l1tot = 0;
    const int* const uvp = &uvt[wave][r0l];
    // (the scheduling fences keep hipcc from hoisting all forty table reads of a step -- and with them forty registers -- to the
    // top: the kernel has 128.  A chunk's bit is read before it is replaced: one register for old and new.)
    if (__builtin_expect(all_fast, 1)) {
      int nx0 = uvp[0], nx1 = uvp[1];  // (a chunk's two products are read one chunk ahead)
#pragma unroll
      for (int n = 0; n < NSLOT; ++n) {
        const int uv0 = nx0, uv1 = nx1;
        if (n + 1 < NSLOT) nx0 = uvp[32 * (n + 1)], nx1 = uvp[32 * (n + 1) + 1];
        x[n] = fast_chunk(x[n], uv0, uv1);
        const int l1 = l1_of(x[n]);
        l1tot += static_cast<uint32_t>(l1);
        okbits = l1 <= limit ? okbits : okbits & ~(1u << n);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int n = 0; n < NSLOT; ++n) {
        const int uv0 = uvp[32 * n], uv1 = uvp[32 * n + 1];
        if (small && ((okbits >> n) & 1u)) x[n] = fast_chunk(x[n], uv0, uv1);
        else x[n] = slow_chunk(x[n], uv0, uv1);
        const int l1 = l1_of(x[n]);
        l1tot += static_cast<uint32_t>(l1);
        okbits = l1 <= limit ? okbits | (1u << n) : okbits & ~(1u << n);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const bool any_nz = __ballot(l1tot != 0) != 0;
    if (lane == 0)
      __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(any_nz ? 0 : 1), drs,
                                           static_cast<int>(static_cast<int64_t>(k) * a.B + g), 0, 16);
    if (__ballot(ovf_any) != 0 && a.overflow && lane == 0) a.overflow[g] = 1;
  };
  // the game leaves once per block (write-through, sc1): whole chunks; the last one only up to byte 15 624
  auto put_state = [&]() {
#pragma unroll
    for (int n = 0; n < NSLOT; ++n) {
      const int c = lane + TL * n;
      const u32x4 q{x[n].x ^ BIAS, x[n].y ^ BIAS, x[n].z ^ BIAS, x[n].w ^ BIAS};
      if (n < NSLOT - 1) {
        if (act) __builtin_amdgcn_raw_buffer_store_b128(q, srs, soff + 16 * c, 0, 16);
      } else {
        if (act && c < NCH - 1) __builtin_amdgcn_raw_buffer_store_b128(q, srs, soff + 16 * c, 0, 16);
        if (c == NCH - 1) {
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{q[0], q[1]}, srs, soff + 16 * c, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(q[2]), srs, soff + 16 * c + 8, 0, 16);
        }
      }
    }
  };
  int kb = 0;                                                  // first step of the block (uniform)
  int nb = a.ready ? wait_released(0) : (a.K < D ? a.K : D);   // its steps: released, not yet requested
  if (nb == 0) return;
  bool fresh = true;  // nothing stored since the last publish
  for (;;) {
    const bool with_poll = a.ready && kb + nb < a.K;  // uniform
    request(kb, kb + nb, with_poll);
    if (a.progress && !fresh) {  // the previous block's stores have left: publish its last step
      if (with_poll) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D) : "memory");
      if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");  // the tokens are in; only that progress store may be under way
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    arrived();
#pragma unroll 1
    for (int d = 0; d < nb; ++d) step(kb + d, d);
    put_state();
    kb += nb;
    fresh = false;
    if (kb >= a.K) break;
    nb = a.ready ? released(pollbuf[wave][lane], kb) : (a.K - kb < D ? a.K - kb : D);
    if (nb == 0) {  // nothing released beyond this block yet: the serial order
      if (a.progress) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(kb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      fresh = true;
      nb = wait_released(kb);
      if (nb == 0) return;
    }
  }
  if (a.progress) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's last stores have left
    if (lane == 0) __hip_atomic_store(a.progress + g, static_cast<uint32_t>(a.K), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
