// tg_state.h -- the kernels that read or write whole states without arithmetic (included inside namespace tg by
// tg_kernels.hip, last): terminal check / nnz, the resets, the copies.

// =============================================================================================
// terminal check / nnz, and reset
// =============================================================================================

// Terminal check + nnz.  A team of `lpg` consecutive lanes (power of two <= 64, chosen on the host
// so that small games do not waste a wavefront: S=4 -> 4 lanes, 16 games per wavefront) owns one
// game; 16-byte loads when the layout allows it (vec16), bytes otherwise.
__global__ __launch_bounds__(kBlock) void done_kernel(const int8_t* state, uint8_t* done, int32_t* nnz,
                                                      int64_t B, int N, int64_t stride, int vec16, int lpg) {
  const int lt = threadIdx.x & (lpg - 1);
  const int64_t team = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) / lpg;
  const int64_t nteam = (static_cast<int64_t>(gridDim.x) * kBlock) / lpg;
  const int64_t rounds = (B + nteam - 1) / nteam;  // every lane runs the same number of rounds (shuffles)
  for (int64_t it = 0; it < rounds; ++it) {
    const int64_t g = team + it * nteam;
    const bool live = g < B;
    const int8_t* p = state + (live ? g : B - 1) * stride;
    int cnt = 0, body = 0;
    if (vec16) {
      body = N & ~15;
      const int step = 16 * lpg;
      int e = 16 * lt;
      for (; e + 3 * step < body; e += 4 * step) {  // four chunks in flight per lane (S=16: the game in one round trip)
        const uint4 q0 = *reinterpret_cast<const uint4*>(p + e), q1 = *reinterpret_cast<const uint4*>(p + e + step),
                    q2 = *reinterpret_cast<const uint4*>(p + e + 2 * step), q3 = *reinterpret_cast<const uint4*>(p + e + 3 * step);
        cnt += count_nonzero_bytes(q0) + count_nonzero_bytes(q1) + count_nonzero_bytes(q2) + count_nonzero_bytes(q3);
      }
      for (; e < body; e += step) cnt += count_nonzero_bytes(*reinterpret_cast<const uint4*>(p + e));
    }
    for (int e = body + lt; e < N; e += lpg) cnt += p[e] != 0;
    if (lpg == 64) cnt = wave_sum(cnt);  // (DPP: no LDS round trips; uniform)
    else
      for (int off = lpg >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lt == 0 && live) {
      done[g] = cnt == 0;
      if (nnz) nnz[g] = cnt;
    }
  }
}

// state_out[b] <- template (S^3 bytes) for b in [first, B).  One thread per 16-byte chunk of the
// whole batch (grid-stride); the template (<= 32 KiB) is served from L1/L2.  vec16 == 0: bytes.
__global__ __launch_bounds__(kBlock) void broadcast_kernel(const int8_t* start, int8_t* out, int64_t first,
                                                           int64_t B, int N, int64_t stride, int vec16) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t nthr = static_cast<int64_t>(gridDim.x) * kBlock;
  if (vec16) {
    const int nchunk = (N + 15) >> 4, tail = N & 15;
    const int64_t total = (B - first) * nchunk;
    if (total < (1ll << 31)) {  // the usual case: 32-bit index arithmetic (a 64-bit division is ~100 instructions)
      const uint32_t tot = static_cast<uint32_t>(total), nc = static_cast<uint32_t>(nchunk);
      for (uint32_t idx = static_cast<uint32_t>(tid); idx < tot; idx += static_cast<uint32_t>(nthr)) {
        const uint32_t gi = idx / nc, c = idx - gi * nc;
        int8_t* dst = out + (first + gi) * stride + 16 * c;
        if (tail && c == nc - 1) {
          for (int t = 0; t < tail; ++t) dst[t] = start[16 * c + t];
        } else {
          *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(start + 16 * c);
        }
      }
      return;
    }
    for (int64_t idx = tid; idx < total; idx += nthr) {
      const int64_t g = first + idx / nchunk;
      const int c = static_cast<int>(idx - (g - first) * nchunk);
      int8_t* dst = out + g * stride + 16 * c;
      if (tail && c == nchunk - 1) {
        for (int t = 0; t < tail; ++t) dst[t] = start[16 * c + t];
      } else {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(start + 16 * c);
      }
    }
  } else {
    const int64_t total = (B - first) * N;
    for (int64_t idx = tid; idx < total; idx += nthr) {
      const int64_t g = first + idx / N;
      const int e = static_cast<int>(idx - (g - first) * N);
      out[g * stride + e] = start[e];
    }
  }
}

// <n,n,n> tensor into ONE game slot (reference utils.py:158-160): entry [p][q][r] = 1 iff
// p = a*n+j, q = j*n+c, r = a*n+c for some a,j,c  <=>  p/n == r/n, q%n == r%n, p%n == q/n.
// tg_reset_matmul_i8 writes game 0 with this and broadcasts it to the other games.
__global__ __launch_bounds__(kBlock) void matmul_template_kernel(int8_t* dst, int n) {
  const int S = n * n, N = S * S * S;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < N; e += gridDim.x * kBlock) {
    const int p = e / (S * S), rem = e - p * S * S, q = rem / S, r = rem - q * S;
    dst[e] = (p / n == r / n) && (q % n == r % n) && (p % n == q / n);
  }
}

// dst[b] <- src[b] for b < B: one thread per 16-byte chunk of a game (the mapping of the step kernels without
// their arithmetic), grid = all chunks.  SH >= 0: chunks per game = 1 << SH (S = 4, 8, 16: shifts instead of a
// division).  The padding between games is neither read nor written.  vec16 == 0: byte granularity.
template <int NT>
__global__ __launch_bounds__(kBlock) void copy_kernel(const int8_t* src, int8_t* dst, int64_t B, int nchunk, int sh,
                                                      int tailb, int64_t sstride, int64_t dstride) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  int64_t g;
  int c;
  if (sh >= 0) {
    g = idx >> sh;
    c = static_cast<int>(idx) & (nchunk - 1);
  } else {
    g = idx / nchunk;
    c = static_cast<int>(idx - g * nchunk);
  }
  if (g >= B) return;
  const int8_t* s = src + g * sstride + 16 * c;
  int8_t* d = dst + g * dstride + 16 * c;
  if (tailb != 0 && c == nchunk - 1) {  // the game's last chunk holds only tailb bytes
    for (int t = 0; t < tailb; ++t) d[t] = s[t];
  } else {
    // (NT as a template parameter: behind a run-time flag hipcc merges the two loads / stores into a plain one)
    uint4 q;
    if constexpr (NT >= 1) {
      const v4u_t v = __builtin_nontemporal_load(reinterpret_cast<const v4u_t*>(s));
      q = uint4{v.x, v.y, v.z, v.w};
    } else {
      q = *reinterpret_cast<const uint4*>(s);
    }
    if constexpr (NT == 2) store16_nt(d, q);
    else *reinterpret_cast<uint4*>(d) = q;
  }
}

__global__ __launch_bounds__(kBlock) void copy_bytes_kernel(const int8_t* src, int8_t* dst, int64_t B, int N,
                                                            int64_t sstride, int64_t dstride) {
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x)
    for (int e = threadIdx.x; e < N; e += kBlock) dst[b * dstride + e] = src[b * sstride + e];
}
