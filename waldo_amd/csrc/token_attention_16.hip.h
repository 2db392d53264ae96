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

// ---------------------------------------------------------------- the backward (token_attention_16_bwd.hip)
//
// The two matrix kernels of the backward read BOTH staged tiles row-wise (S and dP are rows products) and one of them
// also column-wise (dQ: K; dK/dV: Q and dO), so both tiles take one row stride, Ta16BwdTile<D>::LD, which is the
// forward's K stride (KLD: 40 / 24 / 12 dwords).  Banks, in the terms of the analysis at the top:
//   row reads: the forward's K row reads at that stride -- conflict-free at all three D (the forward's unpadded V
//     stride of D = 16, 8 dwords, would be 2-way here).
//   transposed reads: D = 64, stride 40 and D = 32, stride 24 are the forward's V strides -- conflict-free.
//     D = 16, stride 12: the 8 rows of a half start at banks 0 12 24 36 48 60 8 20, runs of 8: the runs of the rows
//     0 / 5, 1 / 6 and 2 / 7 share 4 banks each (0-3, 12-15, 24-27) -- a 2-way conflict on 12 of the 64 banks.  No
//     stride serves both reads of 16-value rows without one: the transposed read wants 8 x odd dwords (8, 24, 40),
//     at which the 8-byte row reads of the rows r and r + 8 meet.  A D = 16 tile step makes 8 row reads (dQ) for 4
//     transposed ones, so the stride is the row reads'.
template <int D>
struct Ta16BwdTile {
  static constexpr int LD = Ta16Tile<D>::KLD;  // LDS row of either tile, in values (48 / 96 / 160 bytes)
  static_assert(LD % 8 == 0, "16-byte stage writes and row reads, 8-byte transposed reads");
};

// One 16-bit value as it is in fp32 (exact).
template <bool BF>
__device__ __forceinline__ float ta16_widen(uint32_t bits16) {
  if constexpr (BF) return __builtin_bit_cast(float, bits16 << 16);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}

// ta16_stage with the backward's stride for both tiles.
template <int D>
__device__ __forceinline__ void ta16_stage_bwd(uint16_t* s0, uint16_t* s1, const ta_u32x4 (&r0)[Ta16Tile<D>::PER],
                                               const ta_u32x4 (&r1)[Ta16Tile<D>::PER]) {
#pragma unroll
  for (int i = 0; i < Ta16Tile<D>::PER; ++i) {
    int row, c8;
    bool mine;
    ta16_piece<D>(i, row, c8, mine);
    if (mine) {
      *reinterpret_cast<ta_u32x4*>(s0 + row * Ta16BwdTile<D>::LD + c8) = r0[i];
      *reinterpret_cast<ta_u32x4*>(s1 + row * Ta16BwdTile<D>::LD + c8) = r1[i];
    }
  }
}

// The rows product, ta16_scores at the backward's stride: acc[j][r] += tile row (16 j + 4 g + r) . the lane's own
// register row `bf` (ta16_load_q's layout); `rows` is the tile's row (lane & 15) at the lane's first column.
template <int D, bool BF>
__device__ __forceinline__ void ta16_rows_product(const uint16_t* rows, const uint32_t (&bf)[Ta16Tile<D>::QW],
                                                  ta_f32x4 (&acc)[Ta16Tile<D>::JB]) {
  constexpr int JB = Ta16Tile<D>::JB, LD = Ta16BwdTile<D>::LD;
  if constexpr (D == 16) {
    const ta_u32x2 b = {bf[0], bf[1]};
#pragma unroll
    for (int j = 0; j < JB; ++j)
      acc[j] = Ta16Type<BF>::mfma16(*reinterpret_cast<const ta_u32x2*>(rows + 16 * j * LD), b, acc[j]);
  } else {
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const ta_u32x4 b = {bf[4 * t], bf[4 * t + 1], bf[4 * t + 2], bf[4 * t + 3]};
      ta_u32x4 a[JB];
#pragma unroll
      for (int j = 0; j < JB; ++j) a[j] = *reinterpret_cast<const ta_u32x4*>(rows + 16 * j * LD + 32 * t);
#pragma unroll
      for (int j = 0; j < JB; ++j) acc[j] = Ta16Type<BF>::mfma32(a[j], b, acc[j]);
    }
  }
}

// The columns product, ta16_values at the backward's stride: acc[d][r] += sum over the tile rows 16 j + 4 g' + r' of
// tile[row][16 d + 4 g + r] p[row], p[j][r] being the lane's fp32 weight of the row 16 j + 4 g + r, rounded here to the
// operand type; `blk` is the lane's transposed-read address (the block of the rows 4 g ... of row block 0).
template <int D, bool BF>
__device__ __forceinline__ void ta16_cols_product(const uint16_t* blk, const ta_f32x4 (&p)[Ta16Tile<D>::JB],
                                                  ta_f32x4 (&acc)[Ta16Tile<D>::DB]) {
  constexpr int JB = Ta16Tile<D>::JB, DB = Ta16Tile<D>::DB, LD = Ta16BwdTile<D>::LD;
#pragma unroll
  for (int s = 0; s < JB / 2; ++s) {
    const ta_u32x4 b = {Ta16Type<BF>::round2(p[2 * s][0], p[2 * s][1]), Ta16Type<BF>::round2(p[2 * s][2], p[2 * s][3]),
                        Ta16Type<BF>::round2(p[2 * s + 1][0], p[2 * s + 1][1]),
                        Ta16Type<BF>::round2(p[2 * s + 1][2], p[2 * s + 1][3])};
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const ta_u32x2 lo = ta16_read_tr(blk + 16 * (2 * s) * LD + 16 * d);
      const ta_u32x2 hi = ta16_read_tr(blk + 16 * (2 * s + 1) * LD + 16 * d);
      const ta_u32x4 a = {lo[0], lo[1], hi[0], hi[1]};
      acc[d] = Ta16Type<BF>::mfma32(a, b, acc[d]);
    }
  }
}

// One 8-byte store of four fp32 values rounded to the operand type.
template <bool BF>
__device__ __forceinline__ void ta16_store4(uint16_t* p, const ta_f32x4& x) {
  const ta_u32x2 w = {Ta16Type<BF>::round2(x[0], x[1]), Ta16Type<BF>::round2(x[2], x[3])};
  *reinterpret_cast<ta_u32x2*>(p) = w;
}

// ---------------------------------------------------------------- host: what the _dt entry points share

// The dtype's refusals, before anything else: the fp32 code names the fp32 entry point.
inline int ta16_check_dtype(const char* fn, const char* fp32_fn, int dtype) {
  if (dtype == WALDO_DTYPE_F32) {
    set_error("%s: dtype WALDO_DTYPE_F32 is served by %s", fn, fp32_fn);
    return WALDO_EINVAL;
  }
  if (dtype != WALDO_DTYPE_F16 && dtype != WALDO_DTYPE_BF16) {
    set_error("%s: unknown dtype %d", fn, dtype);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

// ta_check_strides for 16-bit rows: 16-byte pieces are 8 values.
inline int ta16_check_strides(const char* fn, const int64_t* strides, int nstr) {
  for (int i = 0; i < nstr; ++i)
    if (strides[i] < 0) {
      set_error("%s: negative stride", fn);
      return WALDO_EINVAL;
    }
  for (int i = 0; i < nstr; ++i)
    if (strides[i] % 8 != 0) {
      if (i & 1)
        set_error("%s: bad token stride %lld: rows are D consecutive 16-bit values a multiple of 8 values apart (a view "
                  "with a non-unit inner stride is not served)", fn, (long long)strides[i]);
      else
        set_error("%s: bad batch stride %lld: a multiple of 8 values (rows on 16-byte boundaries)", fn,
                  (long long)strides[i]);
      return WALDO_EINVAL;
    }
  return WALDO_OK;
}

// ta_check_shape for the dense 16-bit entry points: its refusals in its order and words, the strides held to 8 values.
inline int ta16_check_shape(const char* fn, const Ta16Views& v, float scale, int64_t B, int H, int D, int Nq, int Nk1,
                            int Nk2, int64_t blocks) {
  if (B < 0 || H < 1 || Nq < 0 || Nk1 < 1 || Nk2 < 0) {
    set_error("%s: bad shape B=%lld H=%d Nq=%d Nk1=%d Nk2=%d (B, Nq, Nk2 >= 0; H, Nk1 >= 1)", fn, (long long)B, H, Nq,
              Nk1, Nk2);
    return WALDO_EINVAL;
  }
  if (ta_check_head_scale(fn, D, scale) != WALDO_OK) return WALDO_EINVAL;
  if ((int64_t)Nk1 + Nk2 > INT32_MAX - kTaK || B * H > INT32_MAX || B * H * blocks > INT32_MAX) {
    set_error("%s: too large: B=%lld H=%d Nq=%d Nk1=%d Nk2=%d (Nk1 + Nk2 and the %d-row query blocks of all (b, h) stay "
              "below 2^31)", fn, (long long)B, H, Nq, Nk1, Nk2, kTaQ);
    return WALDO_EINVAL;
  }
  const int64_t strides[10] = {v.q.sb, v.q.sn, v.k1.sb, v.k1.sn, v.v1.sb, v.v1.sn, v.k2.sb, v.k2.sn, v.v2.sb, v.v2.sn};
  return ta16_check_strides(fn, strides, Nk2 > 0 ? 10 : 6);
}

// The views as the shared pointer check takes them (it looks at the addresses only).
inline TaViews ta16_as_checked(const Ta16Views& v) {
  auto f = [](const Ta16View& x) { return TaView{reinterpret_cast<const float*>(x.p), x.sb, x.sn}; };
  return {f(v.q), f(v.k1), f(v.v1), f(v.k2), f(v.v2)};
}

}  // namespace waldo
