// tg_s4.h -- S = 4 in registers (included inside namespace tg by tg_kernels.hip after tg_genfused.h): the step forms, the
// in-place step (s4_step_kernel), the fused step + model input (s4_step_emit_kernel), and the step_many / expand / generator
// kernels (s4_kernel, s4_expand_kernel).

// =============================================================================================
// S = 4 in registers: 4 lanes per game, lane q owns slice i = q (16 bytes = one dwordx4).
// Tokens: 12 bytes per action = three dwords (u | v | w), read by every lane of the game.
// =============================================================================================
struct S4Factors {
  int ui;        // -(u_i) for subtract modes, +u_i for GENF
  int v[4], w[4];
};

template <bool SUB>
__device__ __forceinline__ S4Factors s4_factors(const int* tok3, int q, int shift) {
  const uint32_t du = tok3[0], dv = tok3[1], dw = tok3[2];
  S4Factors f;
  f.ui = __builtin_amdgcn_sbfe(static_cast<int>(du), 8 * q, 8) - shift;
  if constexpr (SUB) f.ui = -f.ui;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f.v[t] = sbyte(dv, t) - shift;
    f.w[t] = sbyte(dw, t) - shift;
  }
  return f;
}

__device__ __forceinline__ void s4_rank1(int (&acc)[16], const S4Factors& f, int& chg) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int uv = mul24_pinned(f.ui, f.v[j]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int p = __mul24(uv, f.w[l]);
      acc[4 * j + l] += p;
      chg |= p;
    }
  }
}

// One step on one 16-byte slice (S = 4, lane q owns slice i = q), the body of tg_step_i8, of the child-per-team
// tg_expand_i8 and of the streamed stepper.  Packed form: the slice as 8 int16 pairs, 8 saturating v_pk_mad_i16.
// No range check on the factors is needed: with |factor| <= 255 (int8 token, |shift| <= 127, else the 32-bit form)
// u*v is formed exactly and SATURATES beyond int16, and so does (u v) w + x, so every case the 16-bit form cannot
// represent ends outside the int8 range -- exactly the cases where the true result overflows int8 (|x| <= 255 cannot
// bring a saturated product back).  Those lanes redo their slice in 32-bit (wrapped bytes + flag, as the contract
// wants); all others are exact.
// Round 3: the state enters BIASED -- byte b as b + 128 in [0, 255], zero-extended (x ^ 0x80808080, two v_perm_b32) --
// so "the result fits int8" is "the high byte of every int16 result is zero": the range test is an OR of the eight
// results (4 v_or3) instead of eight v_pk_add_u16 + the ORs, at the price of one XOR per output dword: 51 VALU ops per
// lane on the data path instead of 55 (3.58 against 3.69 us per launch at 131 072 games with the one-dword token load
// of s4_step_kernel, tools/s4_share_probe.hip: with 8 wavefronts per SIMD the arithmetic is on the launch's critical
// path).
// nz |= result bytes; ovf |= (n + 128) of the 32-bit form only (test ovf & ~255).
// the slice's 16 bytes as eight pairs of b + 128 (zero-extended): P[2d] = (b0, b1), P[2d+1] = (b2, b3) of dword d
__device__ __forceinline__ void s4_unpack_biased(const uint4& in_slice, uint32_t (&P)[8]) {
  const uint32_t x[4] = {in_slice.x, in_slice.y, in_slice.z, in_slice.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t xb = x[d] ^ 0x80808080u;
    P[2 * d] = __builtin_amdgcn_perm(0u, xb, 0x0c010c00u);
    P[2 * d + 1] = __builtin_amdgcn_perm(0u, xb, 0x0c030c02u);
  }
}

// the step on an unpacked slice (P from s4_unpack_biased; in_slice again for the rare 32-bit redo)
__device__ __forceinline__ uint4 s4_step_unpacked(const uint32_t (&P)[8], const uint4& in_slice, uint32_t du, uint32_t dv,
                                                  uint32_t dw, int q, int shift, uint32_t& nz, int& ovf) {
  const uint32_t shp = (static_cast<uint32_t>(shift) & 0xFFFFu) | (static_cast<uint32_t>(shift) << 16);
  const int ui = shift - __builtin_amdgcn_sbfe(static_cast<int>(du), 8 * q, 8);  // -(u_i)
  const uint32_t uip = __builtin_amdgcn_perm(static_cast<uint32_t>(ui), static_cast<uint32_t>(ui), 0x05040100u);
  const uint32_t yv = dv << 8, yw = dw << 8;
  const uint32_t vA = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0A050804u), shp);  // (v0, v1)
  const uint32_t vB = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0B070906u), shp);  // (v2, v3)
  const uint32_t wA = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0A050804u), shp);  // (w0, w1)
  const uint32_t wB = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0B070906u), shp);  // (w2, w3)
  const uint32_t uvA = pk_mad_i16_sat(vA, uip, 0u), uvB = pk_mad_i16_sat(vB, uip, 0u);
  uint32_t A[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {  // row j = d: -u v_j is the low (j even) or high (j odd) half of uvA / uvB
    const uint32_t uv = d < 2 ? uvA : uvB;
    if (d & 1) {
      A[2 * d] = pk_mad_i16_sat_hi(uv, wA, P[2 * d]);
      A[2 * d + 1] = pk_mad_i16_sat_hi(uv, wB, P[2 * d + 1]);
    } else {
      A[2 * d] = pk_mad_i16_sat_lo(uv, wA, P[2 * d]);
      A[2 * d + 1] = pk_mad_i16_sat_lo(uv, wB, P[2 * d + 1]);
    }
  }
  uint32_t w[4], ovf16 = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    ovf16 |= A[2 * d] | A[2 * d + 1];
    w[d] = __builtin_amdgcn_perm(A[2 * d + 1], A[2 * d], 0x06040200u) ^ 0x80808080u;
    nz |= w[d];
  }
  uint4 pk{w[0], w[1], w[2], w[3]};
  const bool wide_shift = static_cast<unsigned>(shift + 127) > 254u;  // uniform; factors may exceed 255
  if (__builtin_expect(wide_shift || (ovf16 & 0xFF00FF00u), 0)) {  // rare, per lane: exact 32-bit form of this slice
    const int cur[3] = {static_cast<int>(du), static_cast<int>(dv), static_cast<int>(dw)};
    const S4Factors f = s4_factors<true>(cur, q, shift);
    int acc[16], chg = 0;
    nz = 0;
    unpack16(in_slice, acc);
    s4_rank1(acc, f, chg);
    pk = pack16(acc, nz, ovf);
  }
  return pk;
}

__device__ __forceinline__ uint4 s4_step_slice(const uint4 in_slice, uint32_t du, uint32_t dv, uint32_t dw, int q,
                                               int shift, uint32_t& nz, int& ovf) {
  uint32_t P[8];
  s4_unpack_biased(in_slice, P);
  return s4_step_unpacked(P, in_slice, du, dv, dw, q, shift, nz, ovf);
}

// Digit form of the same step (round 3, second half): a dword of the slice -- row j, elements l = 0..3 -- is read as ONE
// base-256 integer whose digits are the biased bytes b_l = x_l + 128, and the game's w as the integer
// W = sum_l w_l 256^l (= the token dword minus shift * 0x01010101: tokens below 128 make that exact).  The update of
// the whole row is then linear in ONE 32-bit multiply-add,
//     X'_j = X_j + v_j * G  (mod 2^32),   G = -u_i * W,
// and X'_j is the packed result exactly when every digit b_l - u_i v_j w_l stays in [0, 255] (no carry or borrow
// crosses a byte).  That is guaranteed up front, not checked afterwards: all twelve token bytes <= 3 and
// 0 <= shift <= 3 bound every factor by F = max(shift, 3 - shift) <= 3, and the slice's L1 norm (four v_sad_u8 on the
// biased dwords, which need no unpacking either) bounds every |x_l|; L1 <= 127 - F^3 keeps all results inside int8.
// 3 VALU per dword (bias, v_mad_u64_u32, unbias) + 1 for the norm instead of 9 for unpack / two packed MADs / pack /
// range: ~31 instead of ~51 on the data path.  Lanes outside the guarantee (tokens of a wider vocabulary, large
// entries, other shifts) take s4_step_unpacked; results are identical wherever both apply (tests force each form).
// pre: the part that needs the state only (runs while the token dword is still on its way)
__device__ __forceinline__ uint32_t s4_digits_pre(const uint4& in_slice, uint32_t (&xb)[4]) {
  const uint32_t x[4] = {in_slice.x, in_slice.y, in_slice.z, in_slice.w};
  uint32_t l1 = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    xb[d] = x[d] ^ 0x80808080u;
    l1 = __builtin_amdgcn_sad_u8(xb[d], 0x80808080u, l1);
  }
  return l1;
}
// wave-uniform: the largest slice norm the digit form accepts under this shift, -1 when it never applies
// a * b mod 2^32 by v_mad_u64_u32 (full rate on gfx950: 4.9 issue cycles; hipcc's v_mul_lo_u32 is a quarter-rate instruction)
__device__ __forceinline__ uint32_t mul_lo_mad(uint32_t x, uint32_t y) {
  uint64_t r;
  asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(x), "v"(y) : "vcc");
  return static_cast<uint32_t>(r);
}

__host__ __device__ __forceinline__ int s4_digits_limit(int shift) {
  const int F = shift > 3 - shift ? shift : 3 - shift;
  return static_cast<unsigned>(shift) <= 3u ? 127 - F * F * F : -1;
}
// returns false when this lane must take the packed form; nz |= result bytes
__device__ __forceinline__ bool s4_step_digits(const uint32_t (&xb)[4], uint32_t l1, int limit, uint32_t du, uint32_t dv,
                                               uint32_t dw, int q, int shift, uint4& out, uint32_t& nz) {
  const uint32_t wide = (du | dv | dw) & 0xFCFCFCFCu;
  // -(u_i): byte q of du comes down by v_alignbyte_b32 (shifts by q BYTES: no 8 * q), then one SDWA subtract
  const uint32_t nui = static_cast<uint32_t>(shift) - (__builtin_amdgcn_alignbyte(du, du, static_cast<uint32_t>(q)) & 255u);
  const uint32_t W = dw - static_cast<uint32_t>(shift) * 0x01010101u;
  const uint32_t G = mul_lo_mad(nui, W);
  uint32_t o[4], vj[4];
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(vj[0]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(vj[1]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(vj[2]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(vj[3]) : "v"(dv), "s"(shift));
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = (xb[d] + vj[d] * G) ^ 0x80808080u;
  out = uint4{o[0], o[1], o[2], o[3]};
  nz |= o[0] | o[1] | o[2] | o[3];
  return wide == 0 && static_cast<int>(l1) <= limit;
}

// One step on one slice, digit form first and the packed form for the lanes it does not cover (the body shared by
// tg_expand_i8's child teams and the streamed stepper; s4_step_kernel spells the two halves out around its loads).
__device__ __forceinline__ uint4 s4_step_tiered(const uint4& in_slice, uint32_t du, uint32_t dv, uint32_t dw, int q, int shift,
                                                int digits_limit, uint32_t& nz, int& ovf) {
  uint32_t xb[4];
  const uint32_t l1 = s4_digits_pre(in_slice, xb);
  uint4 o;
  uint32_t dnz = 0;
  if (__builtin_expect(s4_step_digits(xb, l1, digits_limit, du, dv, dw, q, shift, o, dnz), 1)) {
    nz |= dnz;
    return o;
  }
  return s4_step_slice(in_slice, du, dv, dw, q, shift, nz, ovf);
}

// The resident stepper's form of the same step: the slice stays BIASED (x ^ 0x80808080) between steps and its L1 norm is
// carried -- the norm of the new slice is at once this step's zero test (l1 == 0) and the next step's precondition, so a step
// is four multiply-adds and four v_sad_u8 (s4_step_tiered: four xor in, four v_sad_u8, four multiply-adds, four xor out,
// three or).  A lane the digit form does not cover un-biases, takes s4_step_slice and biases again.
__device__ __forceinline__ void s4_step_biased(uint4& xb, uint32_t& l1, uint32_t du, uint32_t dv, uint32_t dw, int q, int shift,
                                               int digits_limit, int& ovf) {
  constexpr uint32_t BIAS = 0x80808080u;
  const uint32_t wide = (du | dv | dw) & 0xFCFCFCFCu;
  const uint32_t nui = static_cast<uint32_t>(shift) - (__builtin_amdgcn_alignbyte(du, du, static_cast<uint32_t>(q)) & 255u);
  const uint32_t W = dw - static_cast<uint32_t>(shift) * 0x01010101u;
  const uint32_t G = mul_lo_mad(nui, W);
  uint32_t vj[4];
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(vj[0]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(vj[1]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(vj[2]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(vj[3]) : "v"(dv), "s"(shift));
  uint4 o{xb.x + vj[0] * G, xb.y + vj[1] * G, xb.z + vj[2] * G, xb.w + vj[3] * G};
  if (__builtin_expect(!(wide == 0 && static_cast<int>(l1) <= digits_limit), 0)) {
    uint32_t nz = 0;
    const uint4 r = s4_step_slice(uint4{xb.x ^ BIAS, xb.y ^ BIAS, xb.z ^ BIAS, xb.w ^ BIAS}, du, dv, dw, q, shift, nz, ovf);
    o = uint4{r.x ^ BIAS, r.y ^ BIAS, r.z ^ BIAS, r.w ^ BIAS};
  }
  xb = o;
  l1 = __builtin_amdgcn_sad_u8(o.w, BIAS, __builtin_amdgcn_sad_u8(o.z, BIAS, __builtin_amdgcn_sad_u8(o.y, BIAS, __builtin_amdgcn_sad_u8(o.x, BIAS, 0u))));
}

// Reductions over the four lanes of a team (a DPP quad): two VALU instructions with the exchange folded in (v_add_u32_dpp /
// v_or_b32_dpp), every lane ends with the team's value.  team_any<4> does the same through a ballot: v_cmp + four v_and +
// two 64-bit compares per use -- a third of the resident stepper's step before round 4.
__device__ __forceinline__ uint32_t quad_sum(uint32_t x) {
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
  x += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
  return x;
}
__device__ __forceinline__ uint32_t quad_or(uint32_t x) {
  x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0xB1, 0xf, 0xf, false));
  x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x4E, 0xf, 0xf, false));
  return x;
}

// s4_step_biased for a caller that has tested the tokens of a whole BLOCK of steps at once (`wide`: some token byte of the
// block exceeds 3, team-uniform): the per-step or / and / compare of the twelve bytes leaves the step.
__device__ __forceinline__ void s4_step_biased_blk(uint4& xb, uint32_t& l1, uint32_t du, uint32_t dv, uint32_t dw, int q, int shift,
                                                   int digits_limit, bool wide, int& ovf) {
  constexpr uint32_t BIAS = 0x80808080u;
  const uint32_t nui = static_cast<uint32_t>(shift) - (__builtin_amdgcn_alignbyte(du, du, static_cast<uint32_t>(q)) & 255u);
  const uint32_t W = dw - static_cast<uint32_t>(shift) * 0x01010101u;
  const uint32_t G = mul_lo_mad(nui, W);
  uint32_t vj[4];
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(vj[0]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(vj[1]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(vj[2]) : "v"(dv), "s"(shift));
  asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(vj[3]) : "v"(dv), "s"(shift));
  uint4 o{xb.x + vj[0] * G, xb.y + vj[1] * G, xb.z + vj[2] * G, xb.w + vj[3] * G};
  if (__builtin_expect(wide || static_cast<int>(l1) > digits_limit, 0)) {
    uint32_t nz = 0;
    const uint4 r = s4_step_slice(uint4{xb.x ^ BIAS, xb.y ^ BIAS, xb.z ^ BIAS, xb.w ^ BIAS}, du, dv, dw, q, shift, nz, ovf);
    o = uint4{r.x ^ BIAS, r.y ^ BIAS, r.z ^ BIAS, r.w ^ BIAS};
  }
  xb = o;
  l1 = __builtin_amdgcn_sad_u8(o.w, BIAS, __builtin_amdgcn_sad_u8(o.z, BIAS, __builtin_amdgcn_sad_u8(o.y, BIAS, __builtin_amdgcn_sad_u8(o.x, BIAS, 0u))));
}

// The game's 12 token bytes as three dwords (u | v | w) in every lane of its 4-lane team from ONE dword load per lane:
// lane q loads dword min(q, 2) and the team exchanges them by DPP quad broadcasts (three v_mov_b32_dpp).  A
// global_load_dwordx3 per lane asks the memory pipeline for 48 bytes per game where 12 are distinct; with the token
// buffers of a rollout coming from beyond L2 that is 0.06 us of a 3.6 us launch at 131 072 games.
// blk_tok: the (wave-uniform) token base of the workgroup; team: the game's index within the workgroup.
__device__ __forceinline__ uint32_t s4_team_token_load(const int8_t* blk_tok, int team, int q) {
  const uint32_t off = __umul24(static_cast<uint32_t>(team), 12u) + 4u * static_cast<uint32_t>(q < 3 ? q : 2);  // scalar base + 32-bit lane offset
  return *reinterpret_cast<const uint32_t*>(blk_tok + off);
}
__device__ __forceinline__ void s4_team_token_bcast(uint32_t mine, uint32_t& du, uint32_t& dv, uint32_t& dw) {
  du = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(mine), 0x00, 0xf, 0xf, true));  // quad_perm [0,0,0,0]
  dv = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(mine), 0x55, 0xf, 0xf, true));  // [1,1,1,1]
  dw = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(mine), 0xAA, 0xf, 0xf, true));  // [2,2,2,2]
}
__device__ __forceinline__ void s4_team_tokens(const int8_t* blk_tok, int team, int q, uint32_t& du, uint32_t& dv, uint32_t& dw) {
  s4_team_token_bcast(s4_team_token_load(blk_tok, team, q), du, dv, dw);
}

// =============================================================================================
// tg_step_i8 at S = 4: the single step (round 3; s4_kernel below keeps step_many, gen_from_factors and the
// team-per-parent expand).  4 lanes per game, 16 games per wavefront; one token dword and one 16-byte slice per lane;
// no LDS, no barrier.  Everything that depends on blockIdx is SCALAR 64-bit math; the per-lane part is a 32-bit offset
// (host guarantees strides < 2^20).
//   NTL: the state is read by non-temporal loads (batches beyond the caches: the lines a launch reads are not worth a
//        place in the Infinity Cache when the next launch's reads evict them anyway);
//   TW:  a lane waits for its token before it requests its slice.  For batches far beyond the Infinity Cache only: the
//        wait halves the state requests a wavefront keeps in flight, and the HBM side serves the thinner stream better
//        (2 GiB of states: 815 -> 793 us, 512 MiB: 202 -> 188; at 256 MiB the same wait costs 8 %).
// =============================================================================================
// Its own slim argument block (64 bytes: two s_load_dwordx8, one scalar-load round trip) and 32-bit strides: with 8 wavefronts per SIMD
// every instruction in front of the loads, and every VALU instruction behind them, is on the launch's critical path
// (one VALU instruction per lane = 0.014 us of a 3.6 us launch at 131 072 games).
struct S4StepArgs {
  const int8_t* in;
  int8_t* out;
  const int8_t* actions;
  uint8_t* done;
  uint8_t* overflow;
  int64_t B;
  uint32_t stride;  // in == out stride (tg_step_i8 has one), < 2^20
  int shift;
  int digits_limit;  // s4_digits_limit(shift), from the host (a branch in front of the loads' consumers costs a block)
  int sweep;         // 1 = the workgroups take the games in reverse order (sweep_index); still 64 bytes of arguments
};

//   DIG: the digit form (s4_step_digits) first, the packed form for the lanes it does not cover; false only in the
//        A/B library (TG_S4_NO_DIGITS), for tests and measurements of the packed form alone.
template <bool NTL, bool TW, bool DIG = true>
__global__ __launch_bounds__(kBlock) void s4_step_kernel(S4StepArgs a) {
  constexpr int GPB = kBlock / 4;  // 64 games per workgroup
  const int64_t g0 = static_cast<int64_t>(sweep_index(blockIdx.x, gridDim.x, a.sweep)) * GPB;
  const int nlive = static_cast<int>(min(static_cast<int64_t>(GPB), a.B - g0));
  const int lg_raw = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool live = lg_raw < nlive;
  const int lg = live ? lg_raw : nlive - 1;  // dead lanes shadow the last live game, stores predicated off
  const uint32_t off = __umul24(static_cast<uint32_t>(lg), a.stride) + 16u * q;
  const int8_t* const in_blk = a.in + g0 * a.stride;
  uint32_t du, dv, dw;
  uint4 pk;
  auto load_state = [&]() {
    if constexpr (NTL) {
      const v4u_t v = __builtin_nontemporal_load(reinterpret_cast<const v4u_t*>(in_blk + off));
      pk = uint4{v.x, v.y, v.z, v.w};
    } else {
      pk = *reinterpret_cast<const uint4*>(in_blk + off);
    }
  };
  uint32_t P[8], xb[4], l1 = 0;
  auto state_only = [&]() {  // what can be done before the token is there
    if constexpr (DIG) l1 = s4_digits_pre(pk, xb);
    else s4_unpack_biased(pk, P);
  };
  if constexpr (TW) {  // token, wait, slice (the throttled order for batches far beyond the caches)
    s4_team_tokens(a.actions + g0 * 12, lg, q, du, dv, dw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    load_state();
    state_only();
  } else {
    // The slice FIRST, then the token dword: the states of an in-place rollout sit in L2 / the Infinity Cache, the
    // step's token block comes from wherever its producer left it -- so the slice is biased and measured (or
    // unpacked) while the token is still on its way (vmcnt retires in order).
    // Both requests and both waits are written out: hipcc otherwise issues the token load BEHIND the wait for the slice
    // (a sched_barrier does not hold it: the load is placed at instruction selection), which puts two memory round
    // trips in series.  The "+v" operands of the waits tie the consumers of each register to its wait.
    v4u_t sv;
    uint32_t mine;
    const int8_t* const tok_blk = a.actions + g0 * 12;
    const uint32_t toff = __umul24(static_cast<uint32_t>(lg), 12u) + min(4u * static_cast<uint32_t>(q), 8u);
    if constexpr (NTL) asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=&v"(sv) : "v"(off), "s"(in_blk) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(sv) : "v"(off), "s"(in_blk) : "memory");
    asm volatile("global_load_dword %0, %1, %2" : "=&v"(mine) : "v"(toff), "s"(tok_blk) : "memory");
    asm volatile("s_waitcnt vmcnt(1)" : "+v"(sv) : : "memory");
    pk = uint4{sv.x, sv.y, sv.z, sv.w};
    state_only();
    if constexpr (DIG)  // (l1 / P as operands: the state-only work stays in front of this wait)
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(mine), "+v"(l1) : : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(mine), "+v"(P[0]), "+v"(P[1]), "+v"(P[2]), "+v"(P[3]), "+v"(P[4]), "+v"(P[5]), "+v"(P[6]), "+v"(P[7]) : : "memory");
    s4_team_token_bcast(mine, du, dv, dw);
  }
  uint32_t nz = 0;
  int ovf = 0;
  if constexpr (DIG) {
    uint4 o;
    if (__builtin_expect(s4_step_digits(xb, l1, a.digits_limit, du, dv, dw, q, a.shift, o, nz), 1)) {
      pk = o;
    } else {
      nz = 0;
      pk = s4_step_slice(pk, du, dv, dw, q, a.shift, nz, ovf);
    }
  } else {
    pk = s4_step_unpacked(P, pk, du, dv, dw, q, a.shift, nz, ovf);
  }
  // (skipping the store of untouched slices, as the S >= 9 kernels do in place, is SLOWER here: 16-byte holes inside
  // 64-byte games turn full-line writes into partial ones -- 2.83 -> 3.05 us at BASELINE config 2)
  if (live) *reinterpret_cast<uint4*>(a.out + g0 * a.stride + off) = pk;
  // done: the OR of the team's four slices by two quad-permuting DPP ORs (every lane is active here; dead lanes hold
  // a copy of the last live game), then one byte per game through the workgroup's scalar base + a 32-bit lane offset
  // (the ballot form cost 8 VALU instructions on the q == 0 lanes, this costs 4 on all)
  uint32_t t1, t2;
  asm("s_nop 1\n\tv_or_b32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=&v"(t1) : "v"(nz));
  asm("s_nop 1\n\tv_or_b32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=&v"(t2) : "v"(t1));
  uint8_t* const done_blk = a.done + g0;
  if (q == 0 && live) done_blk[static_cast<uint32_t>(lg)] = t2 ? 0 : 1;
  // the flag is sticky and only ever set to 1: a lane whose slice overflowed stores it itself (rare), so the common
  // path carries no team reduction for it
  if (__builtin_expect((ovf & ~255) != 0, 0) && a.overflow && live) (a.overflow + g0)[lg] = 1;
}

// =============================================================================================
// tg_step_emit at S = 4 ("a fused step + emit model input kernel removes a full extra pass over the
// state"): one env step on the history ring AND the (B,T,4,4,4) float model input of the new state in one launch.
// The step writes the new head into ring slot (head+1) mod T; frame 0 of the output comes from the registers that hold
// it, frame 1 (the old head) from the registers the step read it into, older frames from the ring.
// Lane mapping: 4 lanes per game as in s4_step_kernel, but TRANSPOSED -- lane q holds dword q of every slice, i.e. the
// elements (i = d, j = q, l = 0..3) for d = 0..3 -- so that the four conversions of dword d leave as 16 contiguous
// output bytes per lane and 64 contiguous bytes per team (float32; 32 bytes for the 16-bit types): whole sectors per
// store instruction instead of 16-byte pieces 64 bytes apart.  The arithmetic is s4_step_slice's with the roles of u
// and v exchanged (the lane constant is -v_q, the dword index selects u_d).
// =============================================================================================
struct StepEmitArgs {
  int8_t* ring;
  const int8_t* actions;
  void* out;
  float* scalars;
  uint8_t* done;
  uint8_t* overflow;
  int64_t B;
  int64_t frame_stride;
  int64_t game_stride;
  int T;
  int head;
  int shift;
  float t_step;
};

// four int8 -> four float32 at dst (16 bytes); NT: non-temporal store
template <bool NT>
__device__ __forceinline__ void s4_emit_f32(float* dst, uint32_t w) {
  const uint4 o{__float_as_uint(static_cast<float>(sbyte(w, 0))), __float_as_uint(static_cast<float>(sbyte(w, 1))),
                __float_as_uint(static_cast<float>(sbyte(w, 2))), __float_as_uint(static_cast<float>(sbyte(w, 3)))};
  if constexpr (NT) store16_nt(dst, o);
  else *reinterpret_cast<uint4*>(dst) = o;
}
// four int8 -> two dwords of two 16-bit floats each
template <typename OutT>
__device__ __forceinline__ uint2 s4_cvt16(uint32_t w) {
  const float f0 = static_cast<float>(sbyte(w, 0)), f1 = static_cast<float>(sbyte(w, 1)), f2 = static_cast<float>(sbyte(w, 2)),
              f3 = static_cast<float>(sbyte(w, 3));
  uint32_t lo, hi;
  if constexpr (std::is_same<OutT, __half>::value) {
    typedef __fp16 h2_t __attribute__((ext_vector_type(2)));
    const h2_t x = __builtin_amdgcn_cvt_pkrtz(f0, f1), y = __builtin_amdgcn_cvt_pkrtz(f2, f3);  // |x| <= 128: exact
    __builtin_memcpy(&lo, &x, 4);
    __builtin_memcpy(&hi, &y, 4);
  } else {  // bfloat16 = the upper half of the float32 (at most 8 significant bits: exact)
    lo = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
    hi = __builtin_amdgcn_perm(__float_as_uint(f3), __float_as_uint(f2), 0x07060302u);
  }
  return uint2{lo, hi};
}
// One frame (the lane's dwords y[d] = elements (i = d, j = q, l = 0..3)) -> the output, `frame` = element (0, 0, 0) of
// this game's frame.  float32: dword d of lane q is 16 output bytes at element 16 d + 4 q -- 64 contiguous bytes per
// team and instruction.  16-bit types: a dword is only 8 output bytes, so the lanes of a PAIR (q, q ^ 1) exchange
// dwords (DPP quad_perm [1,0,3,2]) and the even lane stores rows d = 0, 2, the odd lane rows d = 1, 3, each as 16
// bytes covering (j = 2 p, 2 p + 1): again 16-byte stores and 64 contiguous bytes per team and instruction (8-byte
// stores ran the 2^20-game case at 0.65 of step + emit_frames).
template <typename OutT, bool NT>
__device__ __forceinline__ void s4_emit_frame(OutT* frame, const uint32_t (&y)[4], int q) {
  if constexpr (sizeof(OutT) == 4) {
#pragma unroll
    for (int d = 0; d < 4; ++d) s4_emit_f32<NT>(frame + 16 * d + 4 * q, y[d]);
  } else {
    const bool odd = (q & 1) != 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // rows d = 2 h (even lane) / 2 h + 1 (odd lane)
      const uint32_t give = odd ? y[2 * h] : y[2 * h + 1];   // what the partner stores of mine
      const uint32_t got = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(give), 0xB1, 0xf, 0xf, true));
      const uint32_t mine = odd ? y[2 * h + 1] : y[2 * h];
      const uint2 a = s4_cvt16<OutT>(odd ? got : mine), b = s4_cvt16<OutT>(odd ? mine : got);  // (j = 2p, j = 2p + 1)
      const uint4 o{a.x, a.y, b.x, b.y};
      OutT* const dst = frame + 16 * (2 * h + (odd ? 1 : 0)) + 4 * (q & ~1);
      if constexpr (NT) store16_nt(dst, o);
      else *reinterpret_cast<uint4*>(dst) = o;
    }
  }
}

template <typename OutT, bool NT>
__global__ __launch_bounds__(kBlock) void s4_step_emit_kernel(StepEmitArgs a) {
  constexpr int GPB = kBlock / 4;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * GPB;
  const int nlive = static_cast<int>(min(static_cast<int64_t>(GPB), a.B - g0));
  const int lg_raw = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool live = lg_raw < nlive;
  const int lg = live ? lg_raw : nlive - 1;
  uint32_t du, dv, dw;
  s4_team_tokens(a.actions + g0 * 12, lg, q, du, dv, dw);
  const int64_t g = g0 + lg;
  int8_t* const game = a.ring + g * a.game_stride;
  const int nxt = a.head + 1 < a.T ? a.head + 1 : 0;
  const int8_t* const src = game + a.head * a.frame_stride + 4 * q;
  uint32_t x[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) x[d] = *reinterpret_cast<const uint32_t*>(src + 16 * d);  // (i = d, j = q, l = 0..3)
  uint32_t nz = 0;
  int ovf = 0;
  // u and v exchanged: the lane's constant is -v_q, dword d takes u_d
  const uint4 nw = s4_step_tiered(uint4{x[0], x[1], x[2], x[3]}, dv, du, dw, q, a.shift, s4_digits_limit(a.shift), nz, ovf);
  const uint32_t y[4] = {nw.x, nw.y, nw.z, nw.w};
  // (`live` is uniform over a team, so the pair exchange of the 16-bit path stays inside the active lanes)
  OutT* const out = static_cast<OutT*>(a.out) + g * (a.T * 64);
  if (live) {
    int8_t* const dst = game + nxt * a.frame_stride + 4 * q;
#pragma unroll
    for (int d = 0; d < 4; ++d) *reinterpret_cast<uint32_t*>(dst + 16 * d) = y[d];
    s4_emit_frame<OutT, NT>(out, y, q);                    // frame 0: the new head
    if (a.T > 1) s4_emit_frame<OutT, NT>(out + 64, x, q);  // frame 1: the old head
    int slot = a.head;
    for (int f = 2; f < a.T; ++f) {                        // older frames from the ring
      slot = slot > 0 ? slot - 1 : a.T - 1;
      const int8_t* const old = game + slot * a.frame_stride + 4 * q;
      uint32_t z[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) z[d] = *reinterpret_cast<const uint32_t*>(old + 16 * d);
      s4_emit_frame<OutT, NT>(out + 64 * f, z, q);
    }
  }
  const bool any_nz = team_any<4>(nz != 0);
  if (q == 0 && live) {
    a.done[g] = any_nz ? 0 : 1;
    if (a.scalars) a.scalars[g] = a.t_step;
  }
  if (__builtin_expect((ovf & ~255) != 0, 0) && a.overflow && live) a.overflow[g] = 1;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void s4_kernel(ApplyArgs a) {
  // Addressing: everything that depends on blockIdx is SCALAR 64-bit math (SALU); the per-lane
  // part is a small 32-bit offset (host guarantees strides < 2^20).  At the BASELINE cfg2 shape
  // (65 536 games, ~2.5 us per launch) vector 64-bit multiplies were 0.5 us of the launch.
  constexpr int GPB = kBlock / 4;  // 64 games per workgroup
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * GPB;
  const int nlive = static_cast<int>(min(static_cast<int64_t>(GPB), a.B - g0));
  const int lg_raw = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool live = lg_raw < nlive;
  const int lg = live ? lg_raw : nlive - 1;  // dead lanes shadow the last live game, stores predicated off
  static_assert(MODE == MANY || MODE == GENF || MODE == EXPAND, "the single step is s4_step_kernel");
  const int nact = a.nact;
  const int* tok = reinterpret_cast<const int*>(a.actions + g0 * nact * 12) + lg * nact * 3;
  const int8_t* in_blk = a.in + g0 * a.in_stride;
  const uint32_t in_off = __umul24(lg, static_cast<uint32_t>(a.in_stride)) + 16u * q;
  uint4 pk{0, 0, 0, 0};
  if constexpr (MODE != GENF) pk = *reinterpret_cast<const uint4*>(in_blk + in_off);
  int ovf = 0;

  if constexpr (MODE == MANY || MODE == GENF) {
    int8_t* out_blk = a.out + g0 * a.out_stride;
    const uint32_t out_off = __umul24(lg, static_cast<uint32_t>(a.out_stride)) + 16u * q;
    {
      // exact 32-bit form: GENF always; MANY for teams the lattice form below hands over
      auto many_i32 = [&]() {
        int acc[16];
        unpack16(pk, acc);
        int done_step = -1;
        int t0 = tok[0], t1 = tok[1], t2 = tok[2];
        for (int k = 0; k < a.nact; ++k) {
          const int cur[3] = {t0, t1, t2};
          if (k + 1 < a.nact) {  // prefetch the next action's tokens
            t0 = tok[3 * (k + 1)];
            t1 = tok[3 * (k + 1) + 1];
            t2 = tok[3 * (k + 1) + 2];
          }
          const S4Factors f = s4_factors<MODE != GENF>(cur, q, a.shift);
          int chg = 0;
          s4_rank1(acc, f, chg);
          if constexpr (MODE == MANY) {
            uint32_t nz = 0;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
              nz |= static_cast<uint32_t>(acc[t]);
              ovf |= acc[t] + 128;
            }
            if (!team_any<4>((nz & 255) != 0) && done_step < 0) done_step = k;
          }
        }
        uint32_t nz = 0;
        const uint4 o = pack16(acc, nz, ovf);
        if (live) *reinterpret_cast<uint4*>(out_blk + out_off) = o;
        const bool any_ovf = team_any<4>((ovf & ~255) != 0);
        if (q == 0 && live) {
          if constexpr (MODE == MANY) (a.done_step + g0)[lg] = done_step;
          if (a.overflow && any_ovf) (a.overflow + g0)[lg] = 1;
        }
      };
      if constexpr (MODE == GENF) {
        many_i32();
      } else {
        // step_many on the saturating int16 lattice (tg_packed.h): x = 256 n + 128 per half, weights
        // 256 w, v_pk_mad_i16 clamp; the zero test is an OR, the int8 range check one test at the end.
        // Operands must be representable (every factor in [-128,127]); teams that are not, or that
        // leave the lattice (an int8 overflow), are redone by many_i32 from the untouched input.
        uint32_t A[8];
        unpack_pairs(pk, A);
#pragma unroll
        for (int p = 0; p < 8; ++p) A[p] = pk_add_u16(pk_lshl8_b16(A[p]), kLatticeZero);
        const uint32_t shp = __builtin_amdgcn_perm(static_cast<uint32_t>(a.shift), static_cast<uint32_t>(a.shift), 0x05040100u);
        uint32_t rng1 = 0, rng2 = 0;  // range accumulators: (x + 128) must stay below 256
        int done_step = -1;
        int t0 = tok[0], t1 = tok[1], t2 = tok[2];
        for (int k = 0; k < a.nact; ++k) {
          const uint32_t du = t0, dv = t1, dw = t2;
          if (k + 1 < a.nact) {
            t0 = tok[3 * (k + 1)];
            t1 = tok[3 * (k + 1) + 1];
            t2 = tok[3 * (k + 1) + 2];
          }
          const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(du), 8 * q, 8);  // -(u_i)
          rng1 |= static_cast<uint32_t>(ui + 128);
          const uint32_t yv = dv << 8, yw = dw << 8;
          const uint32_t vA = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0A050804u), shp);  // (v0, v1)
          const uint32_t vB = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0B070906u), shp);  // (v2, v3)
          uint32_t wA = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0A050804u), shp);        // (w0, w1)
          uint32_t wB = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0B070906u), shp);        // (w2, w3)
          rng2 |= pk_add_u16(vA, kLatticeZero) | pk_add_u16(vB, kLatticeZero) | pk_add_u16(wA, kLatticeZero) |
                  pk_add_u16(wB, kLatticeZero);
          const uint32_t uip = __builtin_amdgcn_perm(static_cast<uint32_t>(ui), static_cast<uint32_t>(ui), 0x05040100u);
          const uint32_t uvA = pk_mul_lo_u16(vA, uip), uvB = pk_mul_lo_u16(vB, uip);  // (-u v0, -u v1), (-u v2, -u v3)
          wA = pk_lshl8_b16(wA);
          wB = pk_lshl8_b16(wB);
          const uint32_t pr[4] = {__builtin_amdgcn_perm(uvA, uvA, 0x01000100u), __builtin_amdgcn_perm(uvA, uvA, 0x03020302u),
                                  __builtin_amdgcn_perm(uvB, uvB, 0x01000100u), __builtin_amdgcn_perm(uvB, uvB, 0x03020302u)};
          uint32_t nz = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            A[2 * j] = pk_mad_i16_sat(pr[j], wA, A[2 * j]);
            A[2 * j + 1] = pk_mad_i16_sat(pr[j], wB, A[2 * j + 1]);
            nz |= A[2 * j] | A[2 * j + 1];
          }
          if (!team_any<4>((nz & 0xFF00FF00u) != 0) && done_step < 0) done_step = k;
        }
        uint32_t off = (rng1 & ~0xFFu) | (rng2 & 0xFF00FF00u);
#pragma unroll
        for (int p = 0; p < 8; ++p) off |= (A[p] ^ kLatticeZero) & 0x00FF00FFu;
        const bool bad = team_any<4>(off != 0);
        if (!bad) {
          uint32_t w[4];
#pragma unroll
          for (int d = 0; d < 4; ++d) w[d] = __builtin_amdgcn_perm(A[2 * d + 1], A[2 * d], 0x07050301u);
          if (live) *reinterpret_cast<uint4*>(out_blk + out_off) = uint4{w[0], w[1], w[2], w[3]};
          if (q == 0 && live) (a.done_step + g0)[lg] = done_step;
        } else {
          if (threadIdx.x == (threadIdx.x & ~3)) atomicAdd(&g_fallback_workgroups, 1ull);  // one per team
          many_i32();
        }
      }
    }
  } else {  // EXPAND: child (g, k) lives at out + (g*nact + k) * out_stride
    int8_t* out_blk = a.out + g0 * a.nact * a.out_stride;
    const int64_t c0 = g0 * a.nact;
    // The parent slice stays in registers as 8 int16 pairs; a child costs 8 v_pk_mad_i16 and about 40
    // VALU ops in all.  int16 products need |factor| <= 31; a child with larger factors is redone by
    // its 4-lane team in 32-bit (child_i32).
    uint32_t Pp[8];
    unpack_pairs(pk, Pp);
    const uint32_t shp = __builtin_amdgcn_perm(static_cast<uint32_t>(a.shift), static_cast<uint32_t>(a.shift), 0x05040100u);
    int64_t child_off = static_cast<int64_t>(lg) * a.nact * a.out_stride + 16 * q;  // advanced by out_stride per child
    int t0 = tok[0], t1 = tok[1], t2 = tok[2];
    for (int k = 0; k < a.nact; ++k, child_off += a.out_stride) {
      const uint32_t du = t0, dv = t1, dw = t2;
      if (k + 1 < a.nact) {  // prefetch the next child's tokens
        t0 = tok[3 * (k + 1)];
        t1 = tok[3 * (k + 1) + 1];
        t2 = tok[3 * (k + 1) + 2];
      }
      const uint32_t child = static_cast<uint32_t>(lg) * static_cast<uint32_t>(a.nact) + k;  // < 64 * 4096
      const int ui = a.shift - __builtin_amdgcn_sbfe(static_cast<int>(du), 8 * q, 8);  // -(u_i)
      const uint32_t yv = dv << 8, yw = dw << 8, yu = du << 8;
      const uint32_t vA = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0A050804u), shp);
      const uint32_t vB = pk_sub_i16(__builtin_amdgcn_perm(dv, yv, 0x0B070906u), shp);
      const uint32_t wA = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0A050804u), shp);
      const uint32_t wB = pk_sub_i16(__builtin_amdgcn_perm(dw, yw, 0x0B070906u), shp);
      const uint32_t uA = pk_sub_i16(__builtin_amdgcn_perm(du, yu, 0x0A050804u), shp);
      const uint32_t uB = pk_sub_i16(__builtin_amdgcn_perm(du, yu, 0x0B070906u), shp);
      // range: every factor of the child in [-31, 31]  <=>  (f + 31) <= 62 per half; the test is on
      // (f + 32) & ~63 being zero, which admits exactly [-32, 31] (32^3 still fits int16)
      const uint32_t rng = (pk_add_u16(uA, 0x00200020u) | pk_add_u16(uB, 0x00200020u) | pk_add_u16(vA, 0x00200020u) |
                            pk_add_u16(vB, 0x00200020u) | pk_add_u16(wA, 0x00200020u) | pk_add_u16(wB, 0x00200020u)) &
                           0xFFC0FFC0u;
      // null action <=> u, v or w is the zero vector (the whole vector, not this lane's slice)
      const bool nonnull = ((uA | uB) != 0) && ((vA | vB) != 0) && ((wA | wB) != 0);
      uint4 o;
      uint32_t nz = 0, covf = 0;
      if (rng == 0) {  // team-uniform: all four lanes see the same 12 tokens
        const uint32_t uip = __builtin_amdgcn_perm(static_cast<uint32_t>(ui), static_cast<uint32_t>(ui), 0x05040100u);
        const uint32_t uvA = pk_mul_lo_u16(vA, uip), uvB = pk_mul_lo_u16(vB, uip);
        const uint32_t pr[4] = {__builtin_amdgcn_perm(uvA, uvA, 0x01000100u), __builtin_amdgcn_perm(uvA, uvA, 0x03020302u),
                                __builtin_amdgcn_perm(uvB, uvB, 0x01000100u), __builtin_amdgcn_perm(uvB, uvB, 0x03020302u)};
        uint32_t A[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          A[2 * j] = pk_mad_i16(pr[j], wA, Pp[2 * j]);
          A[2 * j + 1] = pk_mad_i16(pr[j], wB, Pp[2 * j + 1]);
        }
        o = pack_pairs(A, nz, covf);
        covf &= 0xFF00FF00u;
      } else {  // exact 32-bit form for this child
        const int cur[3] = {static_cast<int>(du), static_cast<int>(dv), static_cast<int>(dw)};
        const S4Factors f = s4_factors<true>(cur, q, a.shift);
        int acc[16], chg = 0, c32 = 0;
        unpack16(pk, acc);
        s4_rank1(acc, f, chg);
        o = pack16(acc, nz, c32);
        covf = static_cast<uint32_t>(c32) & ~255u;
      }
      if (live) *reinterpret_cast<uint4*>(out_blk + child_off) = o;
      const bool any_nz = team_any<4>(nz != 0);
      const bool any_ovf = team_any<4>(covf != 0);
      if (q == 0 && live) {
        (a.done + c0)[child] = any_nz ? 0 : 1;
        if (a.changed) (a.changed + c0)[child] = nonnull ? 1 : 0;
        if (a.overflow && any_ovf) (a.overflow + c0)[child] = 1;
      }
    }
  }
}

// tg_expand_i8 for S = 4 with one 4-lane team per CHILD: child ch = parent * k + c is just "a step of
// the parent's state with the child's action, written to slot ch", so consecutive teams write
// consecutive 64-byte children and a wavefront's store is 1 KiB of contiguous memory (the
// team-per-parent loop in s4_kernel<EXPAND> writes 64-byte pieces 64 k bytes apart).  The k teams of
// a parent read the same 16-byte parent slices: one request per wavefront, served from L1/L2.  A
// workgroup takes PB = 64 / k whole parents (k <= 64); lc / k by multiplication (recip = ceil(2^16 / k)).
// KEYS (tg_expand_keyed_i8): the 64-bit key of every child leaves with it -- the transposition-table filter of
// extend_tree (act.py:188-195) then needs no second pass over the children.
template <bool NT, bool KEYS = false>
__global__ __launch_bounds__(kBlock) void s4_expand_kernel(ApplyArgs a, int PB, int recip) {
  const int k = a.nact;
  const int lg = threadIdx.x >> 2, q = threadIdx.x & 3;
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * PB;
  const int nlc = static_cast<int>(min(static_cast<int64_t>(PB), a.B - p0)) * k;  // live children of this workgroup
  const bool live = lg < nlc;
  const int lc = live ? lg : nlc - 1;                      // dead teams shadow the last live child
  const int pl = (lc * recip) >> 16;                       // parent within the workgroup
  const int64_t c0 = p0 * k;                               // first child of the workgroup
  uint32_t du, dv, dw;
  s4_team_tokens(a.actions + c0 * 12, lc, q, du, dv, dw);
  const uint4 par = *reinterpret_cast<const uint4*>(a.in + p0 * a.in_stride +
                                                    (__umul24(pl, static_cast<uint32_t>(a.in_stride)) + 16u * q));
  uint32_t nz = 0;
  int ovf = 0;
  const uint4 o = s4_step_tiered(par, du, dv, dw, q, a.shift, s4_digits_limit(a.shift), nz, ovf);
  int8_t* const dst = a.out + c0 * a.out_stride + (__umul24(lc, static_cast<uint32_t>(a.out_stride)) + 16u * q);
  if (live) {
    if constexpr (NT) store16_nt(dst, o);
    else *reinterpret_cast<uint4*>(dst) = o;
  }
  const bool any_nz = team_any<4>(nz != 0);
  const bool any_ovf = team_any<4>((ovf & ~255) != 0);
  if constexpr (KEYS) {
    // the child's key while its four slices are in registers (tg_hash_u64's definition: slice q = chunk q); the team's
    // sum by two quad-permute exchanges per half
    uint64_t h = hash_chunk(o, q);
    auto quad_xor = [](uint64_t v, auto ctrl) {
      const uint32_t lo = __builtin_amdgcn_mov_dpp(static_cast<uint32_t>(v), decltype(ctrl)::value, 0xf, 0xf, true);
      const uint32_t hi = __builtin_amdgcn_mov_dpp(static_cast<uint32_t>(v >> 32), decltype(ctrl)::value, 0xf, 0xf, true);
      return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
    };
    h += quad_xor(h, std::integral_constant<int, 0xB1>{});  // lanes (1,0,3,2)
    h += quad_xor(h, std::integral_constant<int, 0x4E>{});  // lanes (2,3,0,1)
    if (q == 0 && live) (a.keys + c0)[lc] = hash_finish(h, 64);
  }
  if (q == 0 && live) {
    (a.done + c0)[lc] = any_nz ? 0 : 1;
    if (a.changed) {
      // null action <=> u, v or w is the zero vector <=> all four of its token bytes equal the shift
      const uint32_t zs = (static_cast<uint32_t>(a.shift) & 0xFFu) * 0x01010101u;
      const bool in8 = static_cast<unsigned>(a.shift + 128) < 256u;  // otherwise no token equals the shift
      (a.changed + c0)[lc] = (in8 && (du == zs || dv == zs || dw == zs)) ? 0 : 1;
    }
    if (a.overflow && any_ovf) (a.overflow + c0)[lc] = 1;
  }
}
