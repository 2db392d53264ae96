// The device half of the 16-bit token attention (token_attention_16.hip): the tile pipeline of the fp32 kernels
// (token_attention_common.hip.h) restated for bf16 / fp16 operands on the 16-bit matrix instructions.  Nothing here is
// shared with the fp32 kernels' device code, whose register allocation hangs on that header's spelling; the host-side
// checks, TaClips / ta_segment and ta_coord are that header's.
//
// An operand row is D consecutive 16-bit values; a 16-byte piece holds 8 of them.  A 64-key tile of K and of V is
// staged ROW-MAJOR in LDS with padded rows (Ta16Tile: KLD, VLD) and read two ways:
//   S^T = K Q^T   a = the K row 16 j + (lane & 15), 8 consecutive d per lane (ds_read_b128; D = 16: 4 d, ds_read_b64),
//                 b = the lane's own Q row at the same d.  v_mfma_f32_16x16x32 (D = 16: 16x16x16).  Lane (q, g) ends
//                 with the scores of the keys 16 j + 4 g + r, as in the fp32 kernel.
//   O^T = V^T P^T one k = 32 step takes the key blocks 2 s and 2 s + 1: element e of the lane's b operand is its own
//                 p of key 16 (2 s + (e >> 2)) + 4 g + (e & 3), rounded to the operand type in registers; the a operand
//                 is V read COLUMN-wise by two ds_read_b64_tr_b16, the 4-row x 16-column blocks of the rows
//                 16 (2 s) + 4 g ... + 3 and 16 (2 s + 1) + 4 g ... + 3 -- the same keys in the same elements.
//                 Lane (q, g) ends with O[q][16 d + 4 g + r]: one 8-byte store per d block.
// The transposed read gathers across lanes: it runs with EXEC all ones (the kernel's only branches around it are
// wave-uniform), every lane's address is 8-byte aligned and inside the tile (a tile always has its 64 rows: rows past
// the last key are zeros).
//
// Banks ((byte address / 4) mod 64, counted per lane group of the read) for the row strides of Ta16Tile, in dwords:
//   transposed read of V: a 32-lane half takes the 8 rows 8 n ... 8 n + 7 of a key block, 8 dwords (16 columns) each.
//     D = 64, stride 40: the rows start at banks 0 40 16 56 32 8 48 24 -- 8 disjoint runs of 8: conflict-free.
//     D = 32, stride 24: 0 24 48 8 32 56 16 40 -- conflict-free.   D = 16, stride 8 (no pad): 0 8 ... 56 -- conflict-free.
//   row read of K, ds_read_b128 (D >= 32), lane (row, g) at dword stride * row + 4 g; a group is the rows 0-3, 12-15 of
//   g and the rows 4-11 of g + 1:
//     D = 64, stride 40: 0 40 16 56 | 32 8 48 24 and 36 12 52 28 4 44 20 60 -- 16 disjoint runs of 4: conflict-free.
//     D = 32, stride 24: 0 24 48 8 | 32 56 16 40 and 36 60 20 44 4 28 52 12 -- conflict-free.
//   row read of K, ds_read_b64 (D = 16), a half is the 16 rows of g and g + 1 at dword stride * row + 2 g:
//     stride 12: 0 12 24 36 48 60 8 20 32 44 56 4 16 28 40 52, 4 banks a row -- conflict-free (unpadded, stride 8: 2-way).
#pragma once
#include "token_attention_common.hip.h"

namespace waldo {

typedef short ta_s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ta_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ta_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ta_f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ta_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ta_u32x2 __attribute__((ext_vector_type(2)));

// One 16-bit operand as it lies; strides in elements.
struct Ta16View {
  const uint16_t* p;
  int64_t sb, sn;
};
struct Ta16Views {
  Ta16View q, k1, v1, k2, v2;
};

// The element type's two conversions and its matrix instructions.  BF: bf16, else fp16.
template <bool BF>
struct Ta16Type {
  // fp32 -> the operand type, round to nearest even (a NaN stays a NaN), as 16 bits
  static __device__ __forceinline__ uint16_t round(float x) {
    if constexpr (BF) return __builtin_bit_cast(uint16_t, (__bf16)x);
    else return __builtin_bit_cast(uint16_t, (_Float16)x);
  }
  static __device__ __forceinline__ uint32_t round2(float lo, float hi) {
    return (uint32_t)round(lo) | ((uint32_t)round(hi) << 16);
  }
  // acc += a (16 x 32) b (32 x 16): 8 values per lane each
  static __device__ __forceinline__ ta_f32x4 mfma32(ta_u32x4 a, ta_u32x4 b, ta_f32x4 acc) {
    if constexpr (BF)
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ta_bf16x8, a), __builtin_bit_cast(ta_bf16x8, b),
                                                     acc, 0, 0, 0);
    else
      return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ta_f16x8, a), __builtin_bit_cast(ta_f16x8, b),
                                                    acc, 0, 0, 0);
  }
  // acc += a (16 x 16) b (16 x 16): 4 values per lane each (the scores of D = 16)
  static __device__ __forceinline__ ta_f32x4 mfma16(ta_u32x2 a, ta_u32x2 b, ta_f32x4 acc) {
    if constexpr (BF)
      return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(ta_s16x4, a), __builtin_bit_cast(ta_s16x4, b),
                                                       acc, 0, 0, 0);
    else
      return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(ta_f16x4, a), __builtin_bit_cast(ta_f16x4, b),
                                                   acc, 0, 0, 0);
  }
};

// A 64-row tile of D-value rows: in registers as 16-byte pieces dealt out to the threads, in LDS as padded rows.
template <int D>
struct Ta16Tile {
  static constexpr int KLD = D == 16 ? 24 : D + 16;   // LDS row of K, in values (48 / 96 / 160 bytes)
  static constexpr int VLD = D == 16 ? 16 : D + 16;   // LDS row of V (32 / 96 / 160 bytes)
  static constexpr int V8 = D / 8;                    // 16-byte pieces of a row
  static constexpr int PIECES = kTaK * V8;            // ... of a tile (128, 256, 512)
  static constexpr int PER = (PIECES + kBlock - 1) / kBlock;  // pieces per thread (1, 1, 2)
  static constexpr bool ALL = PIECES % kBlock == 0;   // every thread has PER pieces (D = 16: the first two waves have)
  static constexpr int JB = kTaK / 16, DB = D / 16;
  static constexpr int QW = D == 16 ? 2 : 4 * (D / 32);  // dwords of the lane's part of its Q row
  static_assert(KLD % 8 == 0 && VLD % 4 == 0, "16-byte row reads of K, 8-byte transposed reads of V");
};

__device__ __forceinline__ Ta16View ta16_view_at(const Ta16View& v, int64_t b, int hd) {
  return {v.p ? v.p + b * v.sb + hd : nullptr, v.sb, v.sn};
}
__device__ __forceinline__ Ta16Views ta16_views_at(const Ta16Views& v, int64_t qb, int64_t kb, int hd) {
  return {ta16_view_at(v.q, qb, hd), ta16_view_at(v.k1, kb, hd), ta16_view_at(v.v1, kb, hd), ta16_view_at(v.k2, kb, hd),
          ta16_view_at(v.v2, kb, hd)};
}

__device__ __forceinline__ ta_u32x4 ta16_load_piece(const uint16_t* p, bool live) {
  const ta_u32x4 zero4 = {0u, 0u, 0u, 0u};
  const ta_u32x4 x = *reinterpret_cast<const ta_u32x4*>(p);
  return live ? x : zero4;
}

// Piece i of this thread in a tile: its row and its first column.  (D = 16: a thread of the last two waves gets a
// piece past the tile; `mine` is wave-uniform.)
template <int D>
__device__ __forceinline__ void ta16_piece(int i, int& row, int& c8, bool& mine) {
  const int e = (int)threadIdx.x + i * kBlock;
  mine = Ta16Tile<D>::ALL || e < Ta16Tile<D>::PIECES;
  row = (e / Ta16Tile<D>::V8) & (kTaK - 1), c8 = (e % Ta16Tile<D>::V8) * 8;
}

// The fetch of tile `tile` of the keys, which run over the two segments, into registers (staged one tile later): per
// piece one select of the segment's pointer and one clamped index, every assignment unconditional.  Past the last key
// row 0 of the first segment is read and dropped for zeros.
template <int D>
__device__ __forceinline__ void ta16_fetch_kv(const Ta16Views& at, int tile, int Nk1, int Nk,
                                              ta_u32x4 (&kreg)[Ta16Tile<D>::PER], ta_u32x4 (&vreg)[Ta16Tile<D>::PER]) {
  const Ta16View k1 = at.k1, v1 = at.v1, k2 = at.k2, v2 = at.v2;
#pragma unroll
  for (int i = 0; i < Ta16Tile<D>::PER; ++i) {
    int row, c8;
    bool mine;
    ta16_piece<D>(i, row, c8, mine);
    const int key = tile * kTaK + row;
    const bool live = key < Nk, second = live && key >= Nk1;
    const int64_t idx = second ? key - Nk1 : (live ? key : 0);
    kreg[i] = ta16_load_piece((second ? k2.p + idx * k2.sn : k1.p + idx * k1.sn) + c8, live);
    vreg[i] = ta16_load_piece((second ? v2.p + idx * v2.sn : v1.p + idx * v1.sn) + c8, live);
  }
}

// The stage step: the fetched tiles to their padded LDS tiles (between the kernel's two barriers).
template <int D>
__device__ __forceinline__ void ta16_stage(uint16_t* sk, uint16_t* sv, const ta_u32x4 (&kreg)[Ta16Tile<D>::PER],
                                           const ta_u32x4 (&vreg)[Ta16Tile<D>::PER]) {
#pragma unroll
  for (int i = 0; i < Ta16Tile<D>::PER; ++i) {
    int row, c8;
    bool mine;
    ta16_piece<D>(i, row, c8, mine);
    if (mine) {
      *reinterpret_cast<ta_u32x4*>(sk + row * Ta16Tile<D>::KLD + c8) = kreg[i];
      *reinterpret_cast<ta_u32x4*>(sv + row * Ta16Tile<D>::VLD + c8) = vreg[i];
    }
  }
}

// The lane's part of its own Q row: the b operand of every step of the scores.  D >= 32: q[32 t + 8 g ... + 7] in
// dwords 4 t ... 4 t + 3 (a 16-byte load per t); D = 16: q[4 g ... + 3] in two dwords.
template <int D>
__device__ __forceinline__ void ta16_load_q(const uint16_t* row, int g, uint32_t (&qf)[Ta16Tile<D>::QW]) {
  if constexpr (D == 16) {
    const ta_u32x2 x = *reinterpret_cast<const ta_u32x2*>(row + 4 * g);
    qf[0] = x[0], qf[1] = x[1];
  } else {
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const ta_u32x4 x = *reinterpret_cast<const ta_u32x4*>(row + 32 * t + 8 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c) qf[4 * t + c] = x[c];
    }
  }
}

// S^T = K Q^T of one tile: `krows` is the tile's row (lane & 15) at the lane's first column (8 g; D = 16: 4 g).
template <int D, bool BF>
__device__ __forceinline__ void ta16_scores(const uint16_t* krows, const uint32_t (&qf)[Ta16Tile<D>::QW],
                                            ta_f32x4 (&s)[Ta16Tile<D>::JB]) {
  constexpr int JB = Ta16Tile<D>::JB, KLD = Ta16Tile<D>::KLD;
  if constexpr (D == 16) {
    const ta_u32x2 b = {qf[0], qf[1]};
#pragma unroll
    for (int j = 0; j < JB; ++j)
      s[j] = Ta16Type<BF>::mfma16(*reinterpret_cast<const ta_u32x2*>(krows + 16 * j * KLD), b, s[j]);
  } else {
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const ta_u32x4 b = {qf[4 * t], qf[4 * t + 1], qf[4 * t + 2], qf[4 * t + 3]};
      ta_u32x4 a[JB];
#pragma unroll
      for (int j = 0; j < JB; ++j) a[j] = *reinterpret_cast<const ta_u32x4*>(krows + 16 * j * KLD + 32 * t);
#pragma unroll
      for (int j = 0; j < JB; ++j) s[j] = Ta16Type<BF>::mfma32(a[j], b, s[j]);
    }
  }
}

// The transposed read: `p` is this lane's address in the 4-row x 16-column block of its 16-lane group (row (lane & 15)
// >> 2 of the block, columns 4 ((lane & 15) & 3) ...); the lane receives column (lane & 15) of the block's 4 rows.
__device__ __forceinline__ ta_u32x2 ta16_read_tr(const uint16_t* p) {
  typedef __attribute__((address_space(3))) ta_s16x4 lds_s16x4;
  return __builtin_bit_cast(ta_u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p));
}

// O^T += V^T P^T of one tile: `vblk` is the lane's transposed-read address in the block of the rows 4 g ... of key
// block 0 and the columns 0 ... 15; p[j][r] is the lane's weight of key 16 j + 4 g + r (fp32, rounded here).
template <int D, bool BF>
__device__ __forceinline__ void ta16_values(const uint16_t* vblk, const ta_f32x4 (&p)[Ta16Tile<D>::JB],
                                            ta_f32x4 (&o)[Ta16Tile<D>::DB]) {
  constexpr int JB = Ta16Tile<D>::JB, DB = Ta16Tile<D>::DB, VLD = Ta16Tile<D>::VLD;
#pragma unroll
  for (int s = 0; s < JB / 2; ++s) {
    const ta_u32x4 b = {Ta16Type<BF>::round2(p[2 * s][0], p[2 * s][1]), Ta16Type<BF>::round2(p[2 * s][2], p[2 * s][3]),
                        Ta16Type<BF>::round2(p[2 * s + 1][0], p[2 * s + 1][1]),
                        Ta16Type<BF>::round2(p[2 * s + 1][2], p[2 * s + 1][3])};
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const ta_u32x2 lo = ta16_read_tr(vblk + 16 * (2 * s) * VLD + 16 * d);
      const ta_u32x2 hi = ta16_read_tr(vblk + 16 * (2 * s + 1) * VLD + 16 * d);
      const ta_u32x4 a = {lo[0], lo[1], hi[0], hi[1]};
      o[d] = Ta16Type<BF>::mfma32(a, b, o[d]);
    }
  }
}

}  // namespace waldo
