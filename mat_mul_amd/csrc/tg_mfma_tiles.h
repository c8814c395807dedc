// tg_mfma_tiles.h -- the matrix-core primitives shared by tg_mfma.h (generator, step_many), tg_genfused.h and
// tg_items.hip (demo items): operand geometry, the byte products of the B fragment, the column-tile map of a
// workgroup.  Included inside namespace tg after tg_device.h.
#pragma once

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <int S>
struct MGeo {
  static constexpr int N = S * S * S, S2 = S * S, A3 = 3 * S;
  static constexpr int NT = (S2 + 31) / 32;   // column tiles per game
  static constexpr int TROWS = 2 * S + 32;    // rows of T: u (S), v (S), w padded to 32
  static constexpr int NCHUNK = (N + 15) / 16;
  static constexpr int TAIL = N % 16;
  static constexpr int IMG = NCHUNK * 16;     // bytes of the output image
  static constexpr int UVLIM = 11;            // |u|, |v| <= 11: u * v fits int8
};

// bytes of dynamic LDS for R actions padded to Rp (a multiple of 32)
template <int S>
constexpr int mfma_lds_bytes(int Rp) { return MGeo<S>::TROWS * (Rp + 16) + MGeo<S>::IMG + 32; }

// 16 byte-wise products a[k] * b[k] (signed) -> bytes of the result.  The four dwords are
// independent chains interleaved so that an instruction never reads the register the previous one
// wrote with a byte dst_sel; the closing s_nop covers "VALU write -> MFMA operand".
__device__ __forceinline__ v4i bytemul16(const v4i a, const v4i b) {
  v4i d;
#define TG_BM(D, A, B, SEL, KEEP)                                                                     \
  "v_mul_i32_i24_sdwa " D ", sext(" A "), sext(" B ") dst_sel:" SEL " dst_unused:" KEEP " src0_sel:" SEL \
  " src1_sel:" SEL "\n\t"
  asm(TG_BM("%0", "%4", "%8", "BYTE_0", "UNUSED_PAD") TG_BM("%1", "%5", "%9", "BYTE_0", "UNUSED_PAD")
      TG_BM("%2", "%6", "%10", "BYTE_0", "UNUSED_PAD") TG_BM("%3", "%7", "%11", "BYTE_0", "UNUSED_PAD")
      TG_BM("%0", "%4", "%8", "BYTE_1", "UNUSED_PRESERVE") TG_BM("%1", "%5", "%9", "BYTE_1", "UNUSED_PRESERVE")
      TG_BM("%2", "%6", "%10", "BYTE_1", "UNUSED_PRESERVE") TG_BM("%3", "%7", "%11", "BYTE_1", "UNUSED_PRESERVE")
      TG_BM("%0", "%4", "%8", "BYTE_2", "UNUSED_PRESERVE") TG_BM("%1", "%5", "%9", "BYTE_2", "UNUSED_PRESERVE")
      TG_BM("%2", "%6", "%10", "BYTE_2", "UNUSED_PRESERVE") TG_BM("%3", "%7", "%11", "BYTE_2", "UNUSED_PRESERVE")
      TG_BM("%0", "%4", "%8", "BYTE_3", "UNUSED_PRESERVE") TG_BM("%1", "%5", "%9", "BYTE_3", "UNUSED_PRESERVE")
      TG_BM("%2", "%6", "%10", "BYTE_3", "UNUSED_PRESERVE") TG_BM("%3", "%7", "%11", "BYTE_3", "UNUSED_PRESERVE")
      "s_nop 1"
      : "=&v"(d.x), "=&v"(d.y), "=&v"(d.z), "=&v"(d.w)
      : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w));
#undef TG_BM
  return d;
}

// The same sixteen products for the ternary vocabulary {-1, 0, 1} by table lookup (gen_fused_kernel<.., LUT>): the u
// rows of T hold the code u + 1 (0, 1, 2), the v rows the code 4 m(v) with m(-1) = 0, m(+1) = 1, m(0) = 2, so
// code_u | code_v is a v_perm_b32 selector into an 8-byte pool: selectors 0..2 -> (+1, 0, -1) = u * (-1), 4..6 ->
// (-1, 0, +1) = u * (+1), and 8..10 (v = 0) replicate the sign bits of pool bytes 1, 3, 5, which are zero.  One v_or_b32
// (VOP2) + one v_perm_b32 per four products instead of four SDWA multiplies.
__device__ __forceinline__ v4i lutmul16(const v4i a, const v4i b, uint32_t pool_hi, uint32_t pool_lo) {
  v4i d;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    d[q] = static_cast<int>(__builtin_amdgcn_perm(pool_hi, pool_lo, static_cast<uint32_t>(a[q]) | static_cast<uint32_t>(b[q])));
  return d;
}
constexpr uint32_t kLutPoolLo = 0x00FF0001u, kLutPoolHi = 0x000100FFu;  // bytes 0..3 = (+1, 0, -1, 0), 4..7 = (-1, 0, +1, 0)
constexpr uint32_t kLutCodeV = 0x00040800u;                             // v code by u code: bytes (0, 8, 4, 0)

typedef __attribute__((address_space(3))) uint8_t lds_u8_t;
struct __attribute__((packed)) UnalignedU32 { uint32_t v; };  // gfx950 LDS takes unaligned dwords (ds_write_b32)

// ---- the tile phase shared by genf_mfma_kernel and gen_fused_kernel (tg_genfused.h) -----------------------------
// Which column tiles a wavefront owns, and where its lanes read their fragments: the same for every game.
template <int S, int NW_ = kBlock / 64>  // NW_ wavefronts share the NT column tiles of a game
struct TileMap {
  static constexpr int NW = NW_, TPW = (MGeo<S>::NT + NW - 1) / NW;
  int uoff[TPW], voff[TPW], ncol[TPW];
  int woff;
};

template <int S, int NW_>
__device__ __forceinline__ void make_tile_map(TileMap<S, NW_>& tm, int RS, int wave, int col, int h) {
  using G = MGeo<S>;
  constexpr int NW = NW_, TPW = TileMap<S, NW_>::TPW;
#pragma unroll
  for (int k = 0; k < TPW; ++k) {
    const int n = 32 * (wave + NW * k) + col;
    const int nn = n < G::S2 ? n : G::S2 - 1;  // columns past S^2 shadow the last one; never stored
    const int i = nn / S, j = nn - i * S;
    tm.uoff[k] = i * RS + 16 * h;
    tm.voff[k] = (S + j) * RS + 16 * h;
    tm.ncol[k] = n < G::S2 ? n : -1;
  }
  tm.woff = (2 * S + col) * RS + 16 * h;
}
