// Token attention on bf16 / fp16 operands, backward (include/waldo_hip.h "Token attention on 16-bit operands"): the
// gradients of softmax(scale q k^T) v in q and in the one or two key / value segments, from the forward's stored 16-bit
// out and its fp32 row statistics lse = m + log(l) (waldo_token_attention_fwd_lse_dt).  The structure is the fp32
// backward's (token_attention_bwd.hip): three launches at the most, no score-sized memory, no workspace but delta, NO
// ATOMICS -- every gradient element is summed by one lane in one order -- on the 16-bit matrix instructions and the tile
// pipeline of the 16-bit forward (token_attention_16.hip.h):
//   delta pass   delta[b, h, i] = sum_d dO[i, d] O[i, d]: one lane per (token, head) row, one fp32 fma chain over d in
//       ascending order, from the 16-bit grad_out and the STORED 16-bit out.
//   dQ kernel    a workgroup is one (b, h) and 64 query rows, a lane owns one row (q = lane & 15); the K and V tiles of
//       64 keys over both segments go by in LDS, the next one prefetched into registers (ta16_fetch_kv).  S^T = K Q^T
//       and dP^T = V dO^T are the forward's first product (a: the LDS row, b: the lane's own Q / dO row in registers),
//       dQ^T = K^T dS^T its second (a: K read column-wise by the transposed LDS read, b: dS rounded in registers).
//   dK/dV kernel the mirror image: a workgroup is one (b, h) and 64 keys indexed over both segments, a lane owns one key
//       whose K and V rows stay in registers and whose gradients go to segment 1 or 2 by its index; the Q and dO tiles
//       of 64 queries go by in LDS with that tile's lse and delta in fp32.  S = Q K^T and dP = dO V^T are the rows
//       product, dV^T = dO^T P and dK^T = Q^T dS the columns product on transposed reads of dO and Q.
// Both tiles of a kernel are now read row-wise, so they share one row stride (Ta16BwdTile; the bank analysis is there).
//
// The arithmetic: a recomputed score and dP are fp32 sums of exact 16-bit products; P = exp(scale S - lse) is fp32;
// delta as above; dS = P o (dP - delta) is fp32; dS and P are rounded to the element type ONLY as operands of dQ / dK
// and of dV; the three gradients are accumulated in fp32; scale multiplies the fp32 accumulators of dQ and dK once,
// after the sum; one rounding (nearest even) at the store.
//
// The transposed read gathers across lanes and runs with EXEC all ones: the only branches around it are wave-uniform
// (a wave whose rows or keys are all past the end only helps to stage).  Rows past Nq and keys past Nk are read
// through a clamped index and staged as zeros, their P is FORCED to 0 (not exp of an lse that was never read), and they
// are never stored.  A batch stride of 0 is read as it is: gradients are per batch element.
#include "token_attention_16.hip.h"

namespace waldo {

struct TokenAttention16BwdArgs {
  Ta16Views v;
  const uint16_t *out, *grad_out;
  const float* lse;
  float* delta;
  uint16_t *grad_q, *grad_k1, *grad_v1, *grad_k2, *grad_v2;  // contiguous (B, N, H, D); nullptr: not wanted
  int64_t rows;  // B Nq H: the (token, head) rows of out
  float scale;
  int H, Nq, Nk1, Nk, blocks;  // Nk = Nk1 + Nk2; blocks: the kernel's row blocks per (b, h)
};

template <int D, bool BF>
__global__ __launch_bounds__(kBlock) void token_attention_16_delta_kernel(TokenAttention16BwdArgs a) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= a.rows) return;
  const ta_u32x4* o = reinterpret_cast<const ta_u32x4*>(a.out + row * D);
  const ta_u32x4* g = reinterpret_cast<const ta_u32x4*>(a.grad_out + row * D);
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < D / 8; ++t) {
    const ta_u32x4 ox = o[t], gx = g[t];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s = __builtin_fmaf(ta16_widen<BF>(gx[c] & 0xffffu), ta16_widen<BF>(ox[c] & 0xffffu), s);
      s = __builtin_fmaf(ta16_widen<BF>(gx[c] >> 16), ta16_widen<BF>(ox[c] >> 16), s);
    }
  }
  const int h = (int)(row % a.H);
  const int64_t bi = row / a.H;
  const int64_t b = bi / a.Nq, i = bi % a.Nq;
  a.delta[(b * a.H + h) * a.Nq + i] = s;
}

template <int D, bool BF>
__global__ __launch_bounds__(kBlock) void token_attention_16_bwd_dq_kernel(TokenAttention16BwdArgs a) {
  constexpr int LD = Ta16BwdTile<D>::LD, PER = Ta16Tile<D>::PER, JB = Ta16Tile<D>::JB, DB = Ta16Tile<D>::DB,
                QW = Ta16Tile<D>::QW;
  __shared__ __attribute__((aligned(16))) uint16_t sk[kTaK * LD];
  __shared__ __attribute__((aligned(16))) uint16_t sv[kTaK * LD];

  const TaCoord c = ta_coord(a.blocks, a.H);
  const int Nq = a.Nq, Nk = a.Nk, Nk1 = a.Nk1;
  const int64_t orow = c.b * Nq;                  // first row of grad_out and grad_q
  const int64_t lrow = (c.b * a.H + c.h) * Nq;    // ... of lse and delta
  const int q0 = c.block * kTaQ + c.wave * 16;
  const bool wave_live = q0 < Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + c.row, Nq - 1);
  const Ta16Views at = ta16_views_at(a.v, c.b, c.b, c.h * D);

  // the lane's parts of its own Q and dO rows (the b operands of the two rows products); the row's lse and delta
  uint32_t qf[QW], gf[QW];
  ta16_load_q<D>(at.q.p + (int64_t)qrow * at.q.sn, c.g, qf);
  ta16_load_q<D>(a.grad_out + ((orow + qrow) * a.H + c.h) * D, c.g, gf);
  const float lse = a.lse[lrow + qrow];
  const float delta = a.delta[lrow + qrow];
  const uint16_t* krows = sk + c.row * LD + (D == 16 ? 4 : 8) * c.g;
  const uint16_t* vrows = sv + c.row * LD + (D == 16 ? 4 : 8) * c.g;
  const uint16_t* kblk = sk + (4 * c.g + (c.row >> 2)) * LD + 4 * (c.row & 3);

  ta_u32x4 kreg[PER], vreg[PER];  // the next tile's rows
  ta_f32x4 dq[DB];
  ta_zero(dq);

  const int tiles = (Nk + kTaK - 1) / kTaK;
  ta16_fetch_kv<D>(at, 0, Nk1, Nk, kreg, vreg);
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta16_stage_bwd<D>(sk, sv, kreg, vreg);
    __syncthreads();
    if (tile + 1 < tiles) ta16_fetch_kv<D>(at, tile + 1, Nk1, Nk, kreg, vreg);
    if (!wave_live) continue;  // wave-uniform: the transposed reads below run with every lane

    // S^T = K Q^T and dP^T = V dO^T: lane (q, g) gets the keys 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
    ta_zero(s), ta_zero(dp);
    ta16_rows_product<D, BF>(krows, qf, s);
    ta16_rows_product<D, BF>(vrows, gf, dp);

    // dS = P (dP - delta), in place of S; a key past the end has P = 0
    const int key0 = tile * kTaK + 4 * c.g;
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = key0 + 16 * j + r < Nk ? __expf(s[j][r] * a.scale - lse) : 0.0f;
        s[j][r] = p * (dp[j][r] - delta);
      }

    // dQ^T = K^T dS^T
    ta16_cols_product<D, BF>(kblk, s, dq);
  }
  if (!wave_live) return;
  if (q0 + c.row < Nq) {
    uint16_t* op = a.grad_q + ((orow + (q0 + c.row)) * a.H + c.h) * D + 4 * c.g;
#pragma unroll
    for (int d = 0; d < DB; ++d) ta16_store4<BF>(op + 16 * d, dq[d] * a.scale);
  }
}

// The dK/dV kernel's fetch: tile `tile` of the queries' Q rows (through the view) and dO rows (dense) into registers,
// with one row statistic pair per thread of the first wavefront's 64; ta16_fetch_kv's rules, one segment.
template <int D>
__device__ __forceinline__ void ta16_fetch_qg(const uint16_t* qp0, int64_t qs_n, const uint16_t* gp0, int64_t gs_n,
                                              const float* lsep, const float* deltap, int tile, int Nq,
                                              ta_u32x4 (&qreg)[Ta16Tile<D>::PER], ta_u32x4 (&greg)[Ta16Tile<D>::PER],
                                              float& lreg, float& dreg) {
#pragma unroll
  for (int i = 0; i < Ta16Tile<D>::PER; ++i) {
    int row, c8;
    bool mine;
    ta16_piece<D>(i, row, c8, mine);
    const int query = tile * kTaQ + row;
    const bool live = query < Nq;
    const int64_t idx = live ? query : 0;
    qreg[i] = ta16_load_piece(qp0 + idx * qs_n + c8, live);
    greg[i] = ta16_load_piece(gp0 + idx * gs_n + c8, live);
  }
  const int query = tile * kTaQ + ((int)threadIdx.x & (kTaQ - 1));
  const bool live = query < Nq;
  const float lx = lsep[live ? query : 0], dx = deltap[live ? query : 0];
  lreg = live ? lx : 0.0f;
  dreg = live ? dx : 0.0f;
}

template <int D, bool BF>
__global__ __launch_bounds__(kBlock) void token_attention_16_bwd_dkv_kernel(TokenAttention16BwdArgs a) {
  constexpr int LD = Ta16BwdTile<D>::LD, PER = Ta16Tile<D>::PER, JB = Ta16Tile<D>::JB, DB = Ta16Tile<D>::DB,
                QW = Ta16Tile<D>::QW;
  static_assert(kTaQ <= kBlock, "one thread per row statistic of a tile");
  __shared__ __attribute__((aligned(16))) uint16_t sq[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) uint16_t sg[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) float slse[kTaQ];
  __shared__ __attribute__((aligned(16))) float sdelta[kTaQ];

  const TaCoord c = ta_coord(a.blocks, a.H);
  const int Nq = a.Nq, Nk = a.Nk, Nk1 = a.Nk1;
  const int64_t lrow = (c.b * a.H + c.h) * Nq;  // first of lse and delta
  const int tid = threadIdx.x;
  const int k0 = c.block * kTaK + c.wave * 16;
  const bool wave_live = k0 < Nk;  // wave-uniform: a wave past the last key only helps to stage
  const int key = k0 + c.row;
  const bool key_live = key < Nk, second = key_live && key >= Nk1;
  const int64_t kidx = second ? key - Nk1 : (key_live ? key : 0);

  // the lane's parts of its key's K and V rows, from the key's segment (the b operands of the two rows products);
  // zeros past the last key, read through the clamped index (that key's column of S and dP is never stored)
  uint32_t kf[QW], vf[QW];
  {
    const Ta16View k1 = a.v.k1, v1 = a.v.v1, k2 = a.v.k2, v2 = a.v.v2;
    const uint16_t* kp = (second ? k2.p + c.b * k2.sb + kidx * k2.sn : k1.p + c.b * k1.sb + kidx * k1.sn) + c.h * D;
    const uint16_t* vp = (second ? v2.p + c.b * v2.sb + kidx * v2.sn : v1.p + c.b * v1.sb + kidx * v1.sn) + c.h * D;
    ta16_load_q<D>(kp, c.g, kf);
    ta16_load_q<D>(vp, c.g, vf);
#pragma unroll
    for (int i = 0; i < QW; ++i) kf[i] = key_live ? kf[i] : 0u, vf[i] = key_live ? vf[i] : 0u;
  }

  const uint16_t* qp0 = a.v.q.p + c.b * a.v.q.sb + c.h * D;
  const uint16_t* gp0 = a.grad_out + (c.b * Nq * a.H + c.h) * D;
  const float* lsep = a.lse + lrow;
  const float* deltap = a.delta + lrow;
  const uint16_t* qrows = sq + c.row * LD + (D == 16 ? 4 : 8) * c.g;
  const uint16_t* grows = sg + c.row * LD + (D == 16 ? 4 : 8) * c.g;
  const uint16_t* qblk = sq + (4 * c.g + (c.row >> 2)) * LD + 4 * (c.row & 3);
  const uint16_t* gblk = sg + (4 * c.g + (c.row >> 2)) * LD + 4 * (c.row & 3);

  // the next tile's Q and dO rows and row statistics
  ta_u32x4 qreg[PER], greg[PER];
  float lreg, dreg;
  ta_f32x4 dk[DB], dv[DB];
  ta_zero(dk), ta_zero(dv);

  const int tiles = (Nq + kTaQ - 1) / kTaQ;
  ta16_fetch_qg<D>(qp0, a.v.q.sn, gp0, (int64_t)a.H * D, lsep, deltap, 0, Nq, qreg, greg, lreg, dreg);
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta16_stage_bwd<D>(sq, sg, qreg, greg);
    if (tid < kTaQ) slse[tid] = lreg, sdelta[tid] = dreg;
    __syncthreads();
    if (tile + 1 < tiles)
      ta16_fetch_qg<D>(qp0, a.v.q.sn, gp0, (int64_t)a.H * D, lsep, deltap, tile + 1, Nq, qreg, greg, lreg, dreg);
    if (!wave_live) continue;  // wave-uniform: the transposed reads below run with every lane

    // S = Q K^T and dP = dO V^T: lane (key, g) gets the queries 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
    ta_zero(s), ta_zero(dp);
    ta16_rows_product<D, BF>(qrows, kf, s);
    ta16_rows_product<D, BF>(grows, vf, dp);

    // P into dp's place and dS into s's; a query past the end has P = 0 (not exp of an lse that was never read)
    const int query0 = tile * kTaQ + 4 * c.g;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const ta_f32x4 l4 = *reinterpret_cast<const ta_f32x4*>(slse + 16 * j + 4 * c.g);
      const ta_f32x4 d4 = *reinterpret_cast<const ta_f32x4*>(sdelta + 16 * j + 4 * c.g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = query0 + 16 * j + r < Nq ? __expf(s[j][r] * a.scale - l4[r]) : 0.0f;
        s[j][r] = p * (dp[j][r] - d4[r]);
        dp[j][r] = p;
      }
    }

    // dV^T = dO^T P and dK^T = Q^T dS
    ta16_cols_product<D, BF>(gblk, dp, dv);
    ta16_cols_product<D, BF>(qblk, s, dk);
  }
  if (!wave_live || !key_live) return;
  // the key's gradients go to its segment: (B, Nk1, H, D) or (B, Nk2, H, D), either of which may not be wanted
  const int64_t nseg = second ? Nk - Nk1 : Nk1;
  const int64_t at = ((c.b * nseg + kidx) * a.H + c.h) * D + 4 * c.g;
  uint16_t* gk = second ? a.grad_k2 : a.grad_k1;
  uint16_t* gv = second ? a.grad_v2 : a.grad_v1;
  if (gk) {
#pragma unroll
    for (int d = 0; d < DB; ++d) ta16_store4<BF>(gk + at + 16 * d, dk[d] * a.scale);
  }
  if (gv) {
#pragma unroll
    for (int d = 0; d < DB; ++d) ta16_store4<BF>(gv + at + 16 * d, dv[d]);
  }
}

namespace {

template <bool BF>
void ta16_bwd_launch(int D, hipStream_t st, TokenAttention16BwdArgs a, int64_t B, int64_t qblocks, int64_t kblocks) {
  const dim3 block(kBlock);
  ta_for_head_dim(D, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    token_attention_16_delta_kernel<kD, BF><<<dim3((unsigned)((a.rows + kBlock - 1) / kBlock)), block, 0, st>>>(a);
    if (a.grad_q) {
      a.blocks = (int)qblocks;
      token_attention_16_bwd_dq_kernel<kD, BF><<<dim3((unsigned)(B * a.H * qblocks)), block, 0, st>>>(a);
    }
    if (a.grad_k1 || a.grad_v1 || a.grad_k2 || a.grad_v2) {
      a.blocks = (int)kblocks;
      token_attention_16_bwd_dkv_kernel<kD, BF><<<dim3((unsigned)(B * a.H * kblocks)), block, 0, st>>>(a);
    }
  });
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_token_attention_bwd_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b,
                                            int64_t k1s_n, const void* v1, int64_t v1s_b, int64_t v1s_n, const void* k2,
                                            int64_t k2s_b, int64_t k2s_n, const void* v2, int64_t v2s_b, int64_t v2s_n,
                                            const void* out, const void* grad_out, const float* lse, float* delta,
                                            void* grad_q, void* grad_k1, void* grad_v1, void* grad_k2, void* grad_v2,
                                            float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2, int dtype,
                                            waldo_stream_t stream) {
  const char* fn = "waldo_token_attention_bwd_dt";
  if (ta16_check_dtype(fn, "waldo_token_attention_bwd", dtype) != WALDO_OK) return WALDO_EINVAL;
  auto u = [](const void* p) { return static_cast<const uint16_t*>(p); };
  auto w = [](void* p) { return static_cast<uint16_t*>(p); };
  Ta16Views v{{u(q), qs_b, qs_n}, {u(k1), k1s_b, k1s_n}, {u(v1), v1s_b, v1s_n}, {u(k2), k2s_b, k2s_n},
              {u(v2), v2s_b, v2s_n}};
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  const int64_t kblocks = ((int64_t)(Nk1 > 0 ? Nk1 : 0) + (Nk2 > 0 ? Nk2 : 0) + kTaK - 1) / kTaK;
  if (ta16_check_shape(fn, v, scale, B, H, D, Nq, Nk1, Nk2, qblocks > kblocks ? qblocks : kblocks) != WALDO_OK)
    return WALDO_EINVAL;
  // the delta pass: a thread per (token, head) row in blocks of kBlock
  const int64_t rows = B * Nq * H;
  if ((rows + kBlock - 1) / kBlock > INT32_MAX) {
    set_error("%s: too large: B=%lld H=%d Nq=%d Nk1=%d Nk2=%d (the rows of out stay below 2^31 blocks of %d)", fn,
              (long long)B, H, Nq, Nk1, Nk2, kBlock);
    return WALDO_EINVAL;
  }
  if (B == 0 || Nq == 0) return WALDO_OK;
  if (Nk2 == 0) grad_k2 = grad_v2 = nullptr;
  if (!grad_q && !grad_k1 && !grad_v1 && !grad_k2 && !grad_v2) return WALDO_OK;
  TaViews chk = ta16_as_checked(v);
  if (ta_check_pointers(fn, chk, Nk2, out && grad_out && lse && delta,
                        {out, grad_out, lse, delta, grad_q, grad_k1, grad_v1, grad_k2, grad_v2}) != WALDO_OK)
    return WALDO_EINVAL;
  if (Nk2 == 0) v.k2 = v.v2 = {nullptr, 0, 0};
  TokenAttention16BwdArgs a{};
  a.v = v, a.out = u(out), a.grad_out = u(grad_out), a.lse = lse, a.delta = delta;
  a.grad_q = w(grad_q), a.grad_k1 = w(grad_k1), a.grad_v1 = w(grad_v1), a.grad_k2 = w(grad_k2), a.grad_v2 = w(grad_v2);
  a.rows = rows, a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2;
  if (dtype == WALDO_DTYPE_BF16) ta16_bwd_launch<true>(D, (hipStream_t)stream, a, B, qblocks, kblocks);
  else ta16_bwd_launch<false>(D, (hipStream_t)stream, a, B, qblocks, kblocks);
  return launch_status(fn);
}
