// What the token attention's forward (token_attention.hip) and backward (token_attention_bwd.hip) share.  On the host:
// the description of the five operand views, their argument checks, the dispatch on the head dimension and the limits.
// On the device: the tile pipeline of the three tiled kernels (forward, dQ, dK/dV), written once -- the workgroup / lane
// coordinates, the fetch of the next tile into registers, the stage step into LDS, and one step of each of the two
// products on v_mfma_f32_16x16x4_f32.  The helpers are force-inlined templates on D that take the register arrays by
// reference and index them with compile-time constants only; a kernel is the sequence of these calls plus what is
// its own (the online softmax, the dS formula, the stores).  The per-clip entry points (waldo_token_attention_clips_*)
// are the same kernels instantiated with CLIPS: what differs is where a workgroup finds its rows (TaClips, ta_segment).
#pragma once
#include <initializer_list>
#include <type_traits>

#include "waldo_common.hip.h"

namespace waldo {

constexpr int kTaQ = 64;    // query rows per workgroup (16 per wavefront)
constexpr int kTaK = 64;    // keys per tile
constexpr int kTaPad = 4;   // floats added to an LDS row
static_assert(kTaQ == kTaK, "one tile shape: the dK/dV kernel stages queries where the other two stage keys");

typedef float ta_f32x4 __attribute__((ext_vector_type(4)));

// One operand as it lies: (token, head) rows of D consecutive floats, heads D apart; strides in floats.
struct TaView {
  const float* p;
  int64_t sb, sn;  // batch stride, token stride
};
// The five operand views, in the entry points' argument order (k2.p, v2.p: nullptr without a second segment).
struct TaViews {
  TaView q, k1, v1, k2, v2;
};

// The per-clip form (waldo_token_attention_clips_*): the operands are PACKED rows, (R, H, D) with no batch axis, and
// clip b's rows are [off[b], off[b + 1]) of a B + 1 entry table in device memory.  The kernels are the dense ones with
// another first step: where a dense workgroup takes its sequence from b and the lengths from the arguments, a clips
// workgroup reads its two table entries, clamped into [0, R] (ta_segment), and the host hands every view over with its
// token stride in the batch stride's place -- so "batch element" i of a view is its row i, and the views are moved to
// a clip's first row by the expression that moves them to a sequence.
struct TaClips {
  const int *q_off, *k_off;
  int Rq, Rk;  // the rows of q and of k / v: no table entry addresses a row past them
};

// ---------------------------------------------------------------- host

inline bool ta_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The head dimension's and the scale's refusals, and the strides' (n of them: batch, token, batch, token, ...).
inline int ta_check_head_scale(const char* fn, int D, float scale) {
  if (D != 16 && D != 32 && D != 64) {
    set_error("%s: bad head dimension D=%d (16, 32 or 64)", fn, D);
    return WALDO_EINVAL;
  }
  if (!(scale == scale) || scale == INFINITY || scale == -INFINITY) {
    set_error("%s: bad scale %g (finite)", fn, (double)scale);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

inline int ta_check_strides(const char* fn, const int64_t* strides, int nstr) {
  for (int i = 0; i < nstr; ++i)
    if (strides[i] < 0) {
      set_error("%s: negative stride", fn);
      return WALDO_EINVAL;
    }
  // a (token, head) row is D consecutive floats read in 16-byte pieces.  A token stride that is no whole number of
  // pieces is what a view with a non-unit inner stride (or rows off the 16-byte boundaries) would need: it has no
  // description here.  A batch stride only has to keep the rows of the next sequence on those boundaries.
  for (int i = 0; i < nstr; ++i)
    if (strides[i] % 4 != 0) {
      if (i & 1)
        set_error("%s: bad token stride %lld: rows are D consecutive floats a multiple of 4 floats apart (a view with a "
                  "non-unit inner stride is not served)", fn, (long long)strides[i]);
      else
        set_error("%s: bad batch stride %lld: a multiple of 4 floats (rows on 16-byte boundaries)", fn,
                  (long long)strides[i]);
      return WALDO_EINVAL;
    }
  return WALDO_OK;
}

// The refusals every entry point of the section shares, in the forward's order and words, up to the strides; `blocks`
// is the larger of the row blocks per (b, h) that the entry point's launches make.  WALDO_OK: go on.
inline int ta_check_shape(const char* fn, const TaViews& v, float scale, int64_t B, int H, int D, int Nq, int Nk1,
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
  return ta_check_strides(fn, strides, Nk2 > 0 ? 10 : 6);
}

// The same for the per-clip entry points, whose views come with a token stride alone (batch stride 0 here; see
// ta_clips_views): `blocks` is the larger of the row blocks per (clip, h) that the launches make, from the caller's
// bounds max_q_len / max_k_len on a clip's rows.
inline int ta_clips_check_shape(const char* fn, const TaViews& v, float scale, int64_t B, int H, int D, int64_t Rq,
                                int64_t Rk, int max_q_len, int max_k_len, int64_t blocks) {
  if (B < 0 || H < 1 || Rq < 0 || Rk < 0) {
    set_error("%s: bad shape B=%lld H=%d Rq=%lld Rk=%lld (B, Rq, Rk >= 0; H >= 1)", fn, (long long)B, H, (long long)Rq,
              (long long)Rk);
    return WALDO_EINVAL;
  }
  if (max_q_len < 0 || max_k_len < 0) {
    set_error("%s: bad clip bound max_q_len=%d max_k_len=%d (>= 0: no clip has more rows)", fn, max_q_len, max_k_len);
    return WALDO_EINVAL;
  }
  if (ta_check_head_scale(fn, D, scale) != WALDO_OK) return WALDO_EINVAL;
  if (Rq > INT32_MAX - kTaQ || Rk > INT32_MAX - kTaK || max_q_len > INT32_MAX - kTaQ || max_k_len > INT32_MAX - kTaK ||
      B * H > INT32_MAX || B * H * blocks > INT32_MAX) {
    set_error("%s: too large: B=%lld H=%d Rq=%lld Rk=%lld max_q_len=%d max_k_len=%d (the rows and the %d-row blocks of "
              "all (clip, h) stay below 2^31)", fn, (long long)B, H, (long long)Rq, (long long)Rk, max_q_len, max_k_len,
              kTaQ);
    return WALDO_EINVAL;
  }
  const int64_t strides[6] = {v.q.sb, v.q.sn, v.k1.sb, v.k1.sn, v.v1.sb, v.v1.sn};
  return ta_check_strides(fn, strides, 6);
}

// The three packed views of a per-clip entry point, for the checks: no second segment, batch stride 0.
inline TaViews ta_clips_views(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v, int64_t vs_n) {
  return {{q, 0, qs_n}, {k, 0, ks_n}, {v, 0, vs_n}, {nullptr, 0, 0}, {nullptr, 0, 0}};
}
// ... and for the kernels, after the checks: a view's row index in the batch index's place (TaClips).
inline void ta_clips_rows_as_batch(TaViews& v) { v.q.sb = v.q.sn, v.k1.sb = v.k1.sn, v.v1.sb = v.v1.sn; }

// The pointer refusals, after the shape's: drops the second segment's views where Nk2 == 0, then refuses a null view
// (or `rest_present` false: one of the entry point's other required pointers is null) and a view or a pointer of `rest`
// off the 16-byte boundaries (a null pointer of `rest` passes: one that is not wanted).
inline int ta_check_pointers(const char* fn, TaViews& v, int Nk2, bool rest_present,
                             std::initializer_list<const void*> rest) {
  if (Nk2 == 0) v.k2.p = v.v2.p = nullptr;
  if (!v.q.p || !v.k1.p || !v.v1.p || !rest_present || (Nk2 > 0 && (!v.k2.p || !v.v2.p))) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  bool aligned = ta_aligned16(v.q.p) && ta_aligned16(v.k1.p) && ta_aligned16(v.v1.p) && ta_aligned16(v.k2.p) &&
                 ta_aligned16(v.v2.p);
  for (const void* p : rest) aligned = aligned && ta_aligned16(p);
  if (!aligned) {
    set_error("%s: pointer not aligned to 16 bytes", fn);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

// f(std::integral_constant<int, D>) for the head dimension the shape check has let through.
template <class F>
inline void ta_for_head_dim(int D, F&& f) {
  if (D == 16) f(std::integral_constant<int, 16>{});
  else if (D == 32) f(std::integral_constant<int, 32>{});
  else f(std::integral_constant<int, 64>{});
}

// {query rows per workgroup (forward, dQ) = queries per tile (dK/dV), keys per tile (forward, dQ) = keys per workgroup
//  (dK/dV), the head dimensions served}: the first n of them to out, their count returned.
inline int ta_limits(int* out, int n) {
  const int limits[5] = {kTaQ, kTaK, 16, 32, 64};
  for (int i = 0; i < 5 && i < n && out; ++i) out[i] = limits[i];
  return 5;
}

// ---------------------------------------------------------------- device

// A 64-row tile of D-float rows, in registers (16-byte pieces dealt out to the threads) and in LDS (padded rows).
template <int D>
struct TaTile {
  static constexpr int LD = D + kTaPad;            // LDS row, floats
  static constexpr int V4 = D / 4;                 // 16-byte pieces of a row
  static constexpr int PER = kTaK * V4 / kBlock;   // pieces of a tile per thread (4, 2, 1)
  static constexpr int JB = kTaK / 16, DB = D / 16;  // 16-row blocks of a tile, 16-float blocks of a row
  static_assert(kTaK * V4 % kBlock == 0, "a tile is a whole number of pieces per thread");
};

// Where a lane works: workgroup (b, h, block of 64 rows), wavefront (16 of those rows), and inside the wavefront the
// row it owns from the first product to the store and the matrix instruction's k index g.
struct TaCoord {
  int64_t b;
  int h, block, wave, lane, row, g;
};

__device__ __forceinline__ TaCoord ta_coord(int blocks, int H) {
  TaCoord c;
  const int tid = threadIdx.x;
  c.lane = tid & (kWave - 1), c.wave = tid >> 6;
  c.row = c.lane & 15, c.g = c.lane >> 4;
  c.block = (int)(blockIdx.x % (unsigned)blocks);
  const int64_t bh = blockIdx.x / (unsigned)blocks;
  c.h = (int)(bh % H);
  c.b = bh / H;
  return c;
}

// The views moved to the first row of (b, h).
__device__ __forceinline__ TaView ta_view_at(const TaView& v, int64_t b, int hd) {
  return {v.p ? v.p + b * v.sb + hd : nullptr, v.sb, v.sn};
}
// (qb for the queries' view and kb for the keys' and values': the sequence b of both, or a clip's two first rows)
__device__ __forceinline__ TaViews ta_views_at(const TaViews& v, int64_t qb, int64_t kb, int hd) {
  return {ta_view_at(v.q, qb, hd), ta_view_at(v.k1, kb, hd), ta_view_at(v.v1, kb, hd), ta_view_at(v.k2, kb, hd),
          ta_view_at(v.v2, kb, hd)};
}

// Clip b's rows of a packed operand of R rows: [first, first + len), whatever the table holds -- both entries are
// clamped into [0, R] and an end before its start is an empty clip, so first + len <= R and no row past the operand is
// ever addressed.  A kernel reads a row of a segment only where len >= 1.
struct TaSegment {
  int first, len;
};
__device__ __forceinline__ TaSegment ta_segment(const int* off, int64_t b, int R) {
  const int lo = min(max(off[b], 0), R), hi = min(max(off[b + 1], 0), R);
  return {lo, max(hi - lo, 0)};
}

// 16 bytes through a clamped row: the load is unconditional, a dead row gives zeros (its scores are masked, and 0 * x
// must stay 0; the zeros as a named constant: see ta_fetch_kv).
__device__ __forceinline__ ta_f32x4 ta_load_piece(const float* p, bool live) {
  const ta_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const ta_f32x4 x = *reinterpret_cast<const ta_f32x4*>(p);
  return live ? x : zero4;
}

// The lane's own operand row, reg[t][c] = p[16 t + c]: with p at column 4 g, the b operand of the rows product.
template <int D>
__device__ __forceinline__ void ta_load_row(const float* p, bool live, ta_f32x4 (&reg)[TaTile<D>::DB]) {
#pragma unroll
  for (int t = 0; t < TaTile<D>::DB; ++t) reg[t] = ta_load_piece(p + 16 * t, live);
}

template <int N>
__device__ __forceinline__ void ta_zero(ta_f32x4 (&x)[N]) {
  const ta_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = zero4;
}

// Piece i of this thread in a tile: its row and its first column.
template <int D>
__device__ __forceinline__ void ta_piece(int i, int& row, int& c4) {
  const int e = (int)threadIdx.x + i * kBlock;
  row = e / TaTile<D>::V4, c4 = (e % TaTile<D>::V4) * 4;
}

// The fetch: tile `tile` of the keys, which run over the two segments, into registers, to be staged one tile later.
// Every index into the arrays is a compile-time constant and every assignment unconditional (a branch per segment that
// writes the arrays sends them to scratch memory); per piece there is one select of the segment's pointer and one
// clamped index.  Past the last key, row 0 of the first segment is read and dropped.
// The compiler's registers hang on the spelling: the select stays written out over the views' copies made before the
// loop, and the zeros are a named constant.  A helper around the select, the views read through `at` inside the loop or
// a zero literal in its place each cost the D = 16 forward 6 to 16 registers, one or two of its 7 waves per SIMD.
template <int D>
__device__ __forceinline__ void ta_fetch_kv(const TaViews& at, int tile, int Nk1, int Nk,
                                            ta_f32x4 (&kreg)[TaTile<D>::PER], ta_f32x4 (&vreg)[TaTile<D>::PER]) {
  const TaView k1 = at.k1, v1 = at.v1, k2 = at.k2, v2 = at.v2;
#pragma unroll
  for (int i = 0; i < TaTile<D>::PER; ++i) {
    int row, c4;
    ta_piece<D>(i, row, c4);
    const int key = tile * kTaK + row;
    const bool live = key < Nk, second = live && key >= Nk1;
    const int64_t idx = second ? key - Nk1 : (live ? key : 0);
    kreg[i] = ta_load_piece((second ? k2.p + idx * k2.sn : k1.p + idx * k1.sn) + c4, live);
    vreg[i] = ta_load_piece((second ? v2.p + idx * v2.sn : v1.p + idx * v1.sn) + c4, live);
  }
}

// The stage step: two fetched tiles to their padded LDS tiles (between the kernel's two barriers).
template <int D>
__device__ __forceinline__ void ta_stage(float* s0, float* s1, const ta_f32x4 (&r0)[TaTile<D>::PER],
                                         const ta_f32x4 (&r1)[TaTile<D>::PER]) {
#pragma unroll
  for (int i = 0; i < TaTile<D>::PER; ++i) {
    int row, c4;
    ta_piece<D>(i, row, c4);
    *reinterpret_cast<ta_f32x4*>(s0 + row * TaTile<D>::LD + c4) = r0[i];
    *reinterpret_cast<ta_f32x4*>(s1 + row * TaTile<D>::LD + c4) = r1[i];
  }
}

// Step t of a rows product, acc[j] += tile rows (16 j + row) . the lane's register row, over the columns
// 16 t + 4 g + c: `rows` is tile + row * LD + 4 g + 16 t (a 16-byte LDS read per j), `reg` the lane's piece t.  Lane
// (row, g) ends with the products of its row with the tile rows 16 j + 4 g + r in acc[j][r].
template <int D>
__device__ __forceinline__ void ta_rows_step(const float* rows, const ta_f32x4& reg, ta_f32x4 (&acc)[TaTile<D>::JB]) {
  constexpr int JB = TaTile<D>::JB;
  ta_f32x4 af[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) af[j] = *reinterpret_cast<const ta_f32x4*>(rows + 16 * j * TaTile<D>::LD);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < JB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j][c], reg[c], acc[j], 0, 0, 0);
}

// Step (j, r) of a columns product, acc[d] += tile column (16 d + row) x p over the tile rows 16 j + 4 g + r: `col`
// is tile + (16 j + 4 g + r) * LD + row, `p` the lane's p[j][r], which never leaves the registers.  Lane (row, g) ends
// with the columns 16 d + 4 g + r of its row in acc[d][r]: one 16-byte store each.
template <int D>
__device__ __forceinline__ void ta_cols_step(const float* col, float p, ta_f32x4 (&acc)[TaTile<D>::DB]) {
#pragma unroll
  for (int d = 0; d < TaTile<D>::DB; ++d) acc[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(col[16 * d], p, acc[d], 0, 0, 0);
}

}  // namespace waldo
