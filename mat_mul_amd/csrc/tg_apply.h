// tg_apply.h -- what every kernel family of the apply entries shares (included inside namespace tg by tg_kernels.hip,
// first): the modes and their argument block, the fallback / hand-over counters, the alternating sweep, the byte fallback
// for any S and alignment (slow_*), and the 16-byte chunk helpers of the aligned kernels.

#define TG_MAX_ACTIONS 4096  // K / k / R per call

enum Mode { STEP = 0, MANY = 1, EXPAND = 2, GENF = 3 };

// Debug aid: workgroups of the packed/rows kernels that fell back to the exact byte-wise form
// (factors too large for the 16-bit path, or an int8 overflow in step_many).  A silent fallback is
// a 10-50x slowdown, so tests assert that ordinary inputs never take it (tg_debug_fallbacks).
__device__ unsigned long long g_fallback_workgroups = 0;
__device__ __forceinline__ void note_fallback() {
  if (threadIdx.x == 0) atomicAdd(&g_fallback_workgroups, 1ull);
}
// Debug aid: games the matrix-core pass of tg_step_many_i8 could not certify and handed to the lattice kernels
// (each costs a second pass; the reference's {-1,0,1} and the paper's {-2..2} vocabularies should stay at 0).
__device__ unsigned long long g_many_handovers = 0;

struct ApplyArgs {
  const int8_t* in;      // GENF: unused (state starts at zero)
  int8_t* out;
  const int8_t* actions; // (B, nact, 3S)
  uint8_t* done;         // STEP (B) / EXPAND (B,nact)
  int32_t* done_step;    // MANY (B)
  uint8_t* changed;      // EXPAND (B,nact), nullable
  uint8_t* overflow;     // (B) or EXPAND (B,nact), nullable
  int64_t B;
  int64_t in_stride;
  int64_t out_stride;
  int S;
  int nact;
  int shift;
  int only_flagged;      // MANY: redo only the games whose done_step is kNeedsExact (second pass after tg_mfma.h)
  int stream_out;        // EXPAND, S = 4 / 16: the children leave by non-temporal stores (output beyond kStreamOutBytes)
  uint64_t* keys;        // EXPAND (B,nact), nullable: the 64-bit key of every child (tg_expand_keyed_i8)
  int sweep;             // STEP, S = 16 / 25: 1 = the workgroups take the games in reverse order (sweep_index)
};

// Alternating sweeps.  A step kernel streams the whole batch through each XCD's 4 MiB L2; the next launch streams it
// again in the same order, so what the L2 still holds -- the END of the batch -- is evicted before that launch gets
// there: every launch reads everything from beyond L2.  With the direction alternating from launch to launch the tail
// of one sweep is the head of the next, and whatever part of an XCD's share fits its L2 is a hit.  Workgroup b runs on
// XCD b mod 8 (round-robin dispatch), so the order is reversed WITHIN each residue class: a game stays on its XCD.
__device__ __forceinline__ uint32_t sweep_index(uint32_t b, uint32_t n, int reverse) {
  if (!reverse) return b;
  const uint32_t x = b & 7u, t = b >> 3, tx = (n - x + 7u) >> 3;  // tx blocks have residue x
  return ((tx - 1u - t) << 3) | x;
}

// done_step value by which many_mfma_kernel hands a game to the lattice kernels (never a valid result)
constexpr int32_t kNeedsExact = INT32_MIN;

// =============================================================================================
// slow path: any S, any alignment.  One workgroup per game, one byte per thread-iteration.
// =============================================================================================
// One game (index b) by the whole workgroup.  nzf: TG_MAX_ACTIONS bytes of LDS (MANY only).
template <int MODE>
__device__ __forceinline__ void slow_game(const ApplyArgs& a, int64_t b, uint8_t* nzf) {
  const int S = a.S, S2 = S * S, N = S2 * S, A3 = 3 * S;
  const int tid = threadIdx.x;
  const int8_t* tok = a.actions + b * a.nact * A3;
  if constexpr (MODE == EXPAND) {
    const int8_t* src = a.in + b * a.in_stride;
    for (int c = 0; c < a.nact; ++c) {
      const int8_t* t = tok + c * A3;
      int8_t* dst = a.out + (b * a.nact + c) * a.out_stride;
      int nz = 0, chg = 0, ovf = 0;
      for (int e = tid; e < N; e += kBlock) {
        const int i = e / S2, r = e - i * S2, j = r / S, l = r - j * S;
        const int p = (t[i] - a.shift) * (t[S + j] - a.shift) * (t[2 * S + l] - a.shift);
        const int n = src[e] - p;
        dst[e] = static_cast<int8_t>(n);
        nz |= n & 255;
        chg |= p;
        ovf |= (n + 128);
      }
      nz = __syncthreads_or(nz);
      chg = __syncthreads_or(chg);
      ovf = __syncthreads_or(ovf & ~255);
      if (tid == 0) {
        a.done[b * a.nact + c] = nz ? 0 : 1;
        if (a.changed) a.changed[b * a.nact + c] = chg ? 1 : 0;
        if (a.overflow && ovf) a.overflow[b * a.nact + c] = 1;
      }
    }
  } else {
    if constexpr (MODE == MANY) {
      __syncthreads();
      for (int k = tid; k < a.nact; k += kBlock) nzf[k] = 0;
      __syncthreads();
    }
    const int8_t* src = (MODE == GENF) ? nullptr : a.in + b * a.in_stride;
    int8_t* dst = a.out + b * a.out_stride;
    int nz = 0, ovf = 0;
    for (int e = tid; e < N; e += kBlock) {
      const int i = e / S2, r = e - i * S2, j = r / S, l = r - j * S;
      int acc = (MODE == GENF) ? 0 : src[e];
      for (int k = 0; k < a.nact; ++k) {
        const int8_t* t = tok + k * A3;
        const int p = (t[i] - a.shift) * (t[S + j] - a.shift) * (t[2 * S + l] - a.shift);
        if constexpr (MODE == GENF) {
          acc += p;
        } else {
          acc -= p;
          ovf |= (acc + 128);
          if constexpr (MODE == MANY) {
            if (acc & 255) nzf[k] = 1;
          }
        }
      }
      if constexpr (MODE == GENF) ovf |= (acc + 128);
      dst[e] = static_cast<int8_t>(acc);
      nz |= acc & 255;
    }
    nz = __syncthreads_or(nz);
    ovf = __syncthreads_or(ovf & ~255);
    if (tid == 0) {
      if constexpr (MODE == STEP) a.done[b] = nz ? 0 : 1;
      if constexpr (MODE == MANY) {
        int first = -1;
        for (int k = 0; k < a.nact; ++k)
          if (!nzf[k]) { first = k; break; }
        a.done_step[b] = first;
      }
      if (a.overflow && ovf) a.overflow[b] = 1;
    }
    __syncthreads();
  }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void slow_kernel(ApplyArgs a) {
  __shared__ __attribute__((aligned(4))) uint8_t nzf[MODE == MANY ? TG_MAX_ACTIONS : 4];
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) slow_game<MODE>(a, b, nzf);
}

// =============================================================================================
// helpers of the aligned kernels: 16-byte chunks <-> 32-bit accumulators
// =============================================================================================
__device__ __forceinline__ void unpack16(const uint4& q, int (&acc)[16]) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[4 * d + t] = sbyte(w[d], t);
}

// narrow with wrap; nz |= any non-zero output byte; ovf |= bits >= 8 of (n+128) when out of range
__device__ __forceinline__ uint4 pack16(const int (&acc)[16], uint32_t& nz, int& ovf) {
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int t = 0; t < 4; ++t) ovf |= acc[4 * d + t] + 128;
    w[d] = pack4(acc[4 * d], acc[4 * d + 1], acc[4 * d + 2], acc[4 * d + 3]);
    nz |= w[d];
  }
  return uint4{w[0], w[1], w[2], w[3]};
}

template <int TAIL>
__device__ __forceinline__ uint4 load_chunk(const int8_t* p, bool tail) {
  if (TAIL != 0 && tail) {  // last chunk of the game: only TAIL bytes belong to it
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < TAIL; ++t) w[t >> 2] |= static_cast<uint32_t>(static_cast<uint8_t>(p[t])) << (8 * (t & 3));
    return uint4{w[0], w[1], w[2], w[3]};
  }
  return *reinterpret_cast<const uint4*>(p);
}

template <int TAIL>
__device__ __forceinline__ void store_chunk(int8_t* p, const uint4& q, bool tail) {
  if (TAIL != 0 && tail) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int t = 0; t < TAIL; ++t) p[t] = static_cast<int8_t>(w[t >> 2] >> (8 * (t & 3)));
    return;
  }
  *reinterpret_cast<uint4*>(p) = q;
}
