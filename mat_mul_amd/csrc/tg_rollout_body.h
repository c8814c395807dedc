// The body of rollout_advance_kernel<W, M> and rollout_advance_slots_kernel<W> (tg_rollout.hip), included INSIDE both
// definitions: not a header of declarations.  It expects in scope `a` (RolloutArgs or RolloutSlotArgs), the item width
// W, M (the row mask is compiled in) and Q (the slot mode: M with the activity and the step index of every group taken
// from slot_state / solved_step / slot_step).  It is text and not a function because the code objects of the plain and
// the masked kernel are pinned: with the body behind an inlined call the register allocation of both changes (two more
// VGPRs, one more SGPR spill); included in place they are what they were (tools/disasm_diff.py).
  __shared__ __attribute__((aligned(16))) int8_t s_tok[kRollTokBytes];
  __shared__ int s_nnz[kRollMaxRows];
  __shared__ int s_ovf[kRollMaxRows];
  __shared__ uint8_t s_act[M ? kRollMaxRows : 1];  // per group of the workgroup (at most one group per row)
  __shared__ int s_step[Q ? kRollMaxRows : 1];     // Q: the step index of every group of the workgroup
  const int tid = threadIdx.x;
  const int S = a.S, S2 = S * S, N = S2 * S, A3 = 3 * S, T = a.T, n = a.n;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * a.gpw;
  const int ng = static_cast<int>(a.G - g0 < a.gpw ? a.G - g0 : a.gpw);  // >= 1: the grid is ceil(G / gpw)
  const int rows = ng * n;
  const int64_t b0 = g0 * n;
  bool mixed = false;  // some groups of this workgroup may be inactive: a workgroup of ONE group that goes on is active
  if constexpr (M) {
    bool any = false;
    for (int base = 0; base < ng; base += 64) {  // every wave over all the groups: the same answer in each
      const int lg = base + (tid & 63);
      bool act = lg < ng && a.solved_step[g0 + lg] < 0;
      if constexpr (Q) {
        const int st = lg < ng ? slot_step_of(a)[g0 + lg] : 0;
        act = act && slot_state_of(a)[g0 + lg] >= 0 && st < a.max_actions;
        if (tid < 64 && lg < ng) s_step[lg] = st;
      }
      if (tid < 64 && lg < ng) s_act[lg] = act;
      any |= act;
    }
    if (!__any(any)) return;
    mixed = Q || ng > 1;
    if constexpr (Q) __syncthreads();  // s_act and s_step are read from here on: the three words are not read again
  }

  // ---- the rows' tokens into LDS (and into the record of played actions), scalars + 1, the counters cleared
  if (a.words) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tokens + b0 * A3);
    const int wpr = A3 / 4;
    for (int x = tid; x < rows * wpr; x += kBlock) {
      if constexpr (Q) {
        if (!s_act[x / wpr / n]) continue;
      } else if (M && mixed && a.solved_step[g0 + x / wpr / n] >= 0) {
        continue;
      }
      const uint32_t t = src[x];
      reinterpret_cast<uint32_t*>(s_tok)[x] = t;
      if (a.actions) {
        const int r = x / wpr, c = x - r * wpr;
        const int step = Q ? s_step[r / n] : a.step;
        reinterpret_cast<uint32_t*>(a.actions + ((b0 + r) * a.max_actions + step) * A3)[c] = t;
      }
    }
  } else {
    const int8_t* src = a.tokens + b0 * A3;
    for (int x = tid; x < rows * A3; x += kBlock) {
      if constexpr (Q) {
        if (!s_act[x / A3 / n]) continue;
      } else if (M && mixed && a.solved_step[g0 + x / A3 / n] >= 0) {
        continue;
      }
      const int8_t t = src[x];
      s_tok[x] = t;
      if (a.actions) {
        const int r = x / A3, c = x - r * A3;
        const int step = Q ? s_step[r / n] : a.step;
        a.actions[((b0 + r) * a.max_actions + step) * A3 + c] = t;
      }
    }
  }
  if (a.scalars) {
    float* sc = a.scalars + b0 * a.dim_s;
    for (int x = tid; x < rows * a.dim_s; x += kBlock) {
      if constexpr (Q) {
        if (!s_act[x / a.dim_s / n]) continue;
      } else if (M && mixed && a.solved_step[g0 + x / a.dim_s / n] >= 0) {
        continue;
      }
      sc[x] += 1.0f;
    }
  }
  for (int r = tid; r < rows; r += kBlock) s_nnz[r] = 0, s_ovf[r] = 0;
  __syncthreads();

  // ---- the items: new head, history shift, per-row counts
  const int full = N / W;  // items of W whole bytes; item `full` (W == 4 only) is the N % 4 tail
  const int nkeep = T > 1 ? T - 1 : 1;  // frames loaded: 0 .. T - 2 move back by one; T == 1 loads the head alone
  const int total = rows * a.ipr;
  for (int it = tid; it < total; it += kBlock) {
    const int lr = it / a.ipr, c = it - lr * a.ipr;
    if (M && mixed && !s_act[lr / n]) continue;
    const int nb = c < full ? W : N - full * W;
    const int e0 = c * W;
    int8_t* const row = a.frames + (b0 + lr) * static_cast<int64_t>(T) * N + e0;
    uint32_t fr[TG_NET_MAX_T][W / 4];
#pragma unroll
    for (int t = 0; t < TG_NET_MAX_T - 1; ++t)
      if (t < nkeep) roll_load<W>(row + static_cast<int64_t>(t) * N, nb, fr[t]);

    const int8_t* const tk = s_tok + lr * A3;
    int i = e0 / S2, rem = e0 - i * S2, j = rem / S, l = rem - j * S;
    uint32_t uv = static_cast<uint32_t>(tk[i] - a.shift) * static_cast<uint32_t>(tk[S + j] - a.shift);
    uint32_t head[W / 4];
    int ovf = 0, cnt = 0;
#pragma unroll
    for (int d = 0; d < W / 4; ++d) {
      uint32_t out = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (4 * d + t < nb) {
          const int p = static_cast<int>(uv * static_cast<uint32_t>(tk[2 * S + l] - a.shift));
          const int nw = sbyte(fr[0][d], t) - p;  // 32-bit, then narrowed with wrap as tg_step_i8 does
          ovf |= nw + 128;
          out |= (static_cast<uint32_t>(nw) & 255u) << (8 * t);
          if (++l == S) {  // the row (i, j) of the tensor ends inside the item: next factors (tk[S] / tk[2S] past the
            l = 0;         // last element are in-row reads of v_0 / w_0 that are never used)
            if (++j == S) j = 0, ++i;
            uv = static_cast<uint32_t>(tk[i] - a.shift) * static_cast<uint32_t>(tk[S + j] - a.shift);
          }
        }
      }
      head[d] = out;
      cnt = count_nonzero_bytes(out, cnt);
    }
#pragma unroll
    for (int t = TG_NET_MAX_T - 2; t >= 0; --t)
      if (t < T - 1) roll_store<W>(row + static_cast<int64_t>(t + 1) * N, nb, fr[t]);
    roll_store<W>(row, nb, head);
    if (cnt) atomicAdd(&s_nnz[lr], cnt);
    if (ovf & ~255) s_ovf[lr] = 1;
  }
  __syncthreads();

  // ---- per row, then per group
  for (int r = tid; r < rows; r += kBlock) {
    if (M && mixed && !s_act[r / n]) continue;
    a.nnz[b0 + r] = s_nnz[r];
    if (a.overflow && s_ovf[r]) a.overflow[b0 + r] = 1;
    if (M && a.active) {  // the group's verdict again, per row: no third barrier
      const int* const grp = s_nnz + r / n * n;
      bool zero = false;
      for (int s = 0; s < n; ++s) zero |= grp[s] == 0;
      a.active[b0 + r] = zero ? 0 : 1;
    }
  }
  for (int lg = tid; lg < ng; lg += kBlock) {
    if (M && mixed && !s_act[lg]) continue;
    int best = s_nnz[lg * n], first = -1;
    for (int s = n - 1; s >= 0; --s) {
      const int v = s_nnz[lg * n + s];
      best = v < best ? v : best;
      first = v == 0 ? s : first;
    }
    const int64_t g = g0 + lg;
    const int old = a.best_nnz[g];
    a.best_nnz[g] = best < old ? best : old;
    if (best == 0) {
      a.hits[g] += 1;
      if (a.solved_step[g] < 0) a.solved_step[g] = Q ? s_step[lg] : a.step, a.solved_sample[g] = first;
    }
    if constexpr (Q) slot_step_of(a)[g] = s_step[lg] + 1;
  }
