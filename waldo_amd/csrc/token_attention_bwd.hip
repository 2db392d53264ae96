// Token attention, backward (include/waldo_hip.h "Token attention"): the gradients of softmax(scale q k^T) v in q and in
// the one or two key / value segments, from the forward's out and row statistics lse = m + log(l).  Per (b, h), fp32:
//   P = exp(scale S - lse),  dP = dO V^T,  delta = rowsum(dO o O),  dS = P o (dP - delta),
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO.
// No score-sized memory and NO ATOMICS: every gradient element is summed by one lane in one order, so the gradients are
// a function of the inputs alone.  The price is that S is computed twice more, once per matrix kernel:
//   delta pass   one read of out and grad_out, a lane per (token, head) row -> delta (B, H, Nq).
//   dQ kernel    the forward's structure (token_attention.hip) used twice.  A workgroup is one (b, h) and kTaQ query
//       rows, a lane owns one query row (q = lane & 15), the K and V tiles go by in LDS.  S^T = K Q^T and dP^T = V dO^T
//       have the operands of the forward's first product (a: the LDS row, b: the lane's own Q / dO row in registers);
//       lane (q, g) ends with the keys 16 j + 4 g + r of both, forms dS in place, and dQ^T = K^T dS^T has the operands
//       of the forward's second product: dS never leaves the registers and the lane ends with dQ[q][16 db + 4 g + r].
//   dK/dV kernel the mirror image.  A workgroup is one (b, h) and kTaK keys, indexed over both segments; a lane owns
//       one key (lane & 15) whose K and V rows stay in registers; the Q and dO tiles go by in LDS with that tile's lse
//       and delta.  S = Q K^T and dP = dO V^T (a: the LDS row, b: the register row) leave lane (key, g) with the
//       queries 16 j + 4 g + r; dV^T = dO^T P and dK^T = Q^T dS take those registers as b.
// The tile pipeline of the two matrix kernels -- fetch, stage, the steps of the two products -- is
// token_attention_common.hip.h's, shared with the forward; here are the kernels' sequences of them, the dK/dV kernel's
// own fetch (one segment, with the row statistics), the dS formula and the stores.
// All products run on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain).  Rows past Nq / Nk are read through a
// clamped index, staged as zeros, their P forced to 0, and never stored.
#include "token_attention_common.hip.h"

namespace waldo {

struct TokenAttentionBwdArgs {
  TaViews v;
  const float *out, *grad_out, *lse;
  float* delta;
  float *grad_q, *grad_k1, *grad_v1, *grad_k2, *grad_v2;
  int64_t rows;  // B Nq H: the (token, head) rows of out
  float scale;
  int H, Nq, Nk1, Nk, blocks;  // Nk = Nk1 + Nk2; blocks: the kernel's row blocks per (b, h)
  TaClips clips;               // CLIPS: the lengths are the clip's own, Nq / Nk1 / Nk are not read
};

// CLIPS, in all three kernels (the forward's, token_attention.hip): b is a clip of packed rows, out / grad_out / grad_q
// are (Rq, H D), grad_k / grad_v (Rk, H D) and lse / delta (H, Rq).  A workgroup whose block starts at or past its
// clip's last row leaves before the first barrier; the dK/dV workgroup of a clip without queries walks no tile and
// stores the zeros it started from.

// delta[b, h, i] = sum_d grad_out[b, i, h, d] out[b, i, h, d]: one lane per row, ONE fma chain in the order in which the
// matrix instruction sums dP = dO . V in the two kernels below (d = 16 t + 4 g + c: t, then c, then the instruction's
// k index g).  Where a row has one key, P = 1 and O = V: delta and dP are then the same chain and dS = P (dP - delta)
// is exactly 0, as it is in exact arithmetic -- two different orders would leave a rounding residue in dQ and dK.
template <int D, bool CLIPS>
__global__ __launch_bounds__(kBlock) void token_attention_delta_kernel(TokenAttentionBwdArgs a) {
  constexpr int DB = D / 16;
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= a.rows) return;
  const ta_f32x4* o = reinterpret_cast<const ta_f32x4*>(a.out + row * D);
  const ta_f32x4* g = reinterpret_cast<const ta_f32x4*>(a.grad_out + row * D);
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < DB; ++t) {
    ta_f32x4 ox[4], gx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ox[k] = o[4 * t + k], gx[k] = g[4 * t + k];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) s = __builtin_fmaf(gx[k][c], ox[k][c], s);
  }
  const int h = (int)(row % a.H);
  const int64_t bi = row / a.H;
  if (CLIPS) {
    a.delta[(int64_t)h * a.clips.Rq + bi] = s;
    return;
  }
  const int64_t b = bi / a.Nq, i = bi % a.Nq;
  a.delta[(b * a.H + h) * a.Nq + i] = s;
}

template <int D, bool CLIPS>
__global__ __launch_bounds__(kBlock) void token_attention_bwd_dq_kernel(TokenAttentionBwdArgs a) {
  constexpr int LD = TaTile<D>::LD, PER = TaTile<D>::PER, JB = TaTile<D>::JB, DB = TaTile<D>::DB;
  __shared__ __attribute__((aligned(16))) float sk[kTaK * LD];
  __shared__ __attribute__((aligned(16))) float sv[kTaK * LD];

  const TaCoord c = ta_coord(a.blocks, a.H);
  const TaSegment qs = CLIPS ? ta_segment(a.clips.q_off, c.b, a.clips.Rq) : TaSegment{0, a.Nq};
  const TaSegment ks = CLIPS ? ta_segment(a.clips.k_off, c.b, a.clips.Rk) : TaSegment{0, a.Nk};
  const int Nq = qs.len, Nk = ks.len, Nk1 = CLIPS ? Nk : a.Nk1;
  if (CLIPS && c.block * kTaQ >= Nq) return;
  const int64_t qb = CLIPS ? (int64_t)qs.first : c.b, kb = CLIPS ? (int64_t)ks.first : c.b;
  const int64_t orow = CLIPS ? (int64_t)qs.first : c.b * Nq;                                    // first row of grad_out
  const int64_t lrow = CLIPS ? (int64_t)c.h * a.clips.Rq + qs.first : (c.b * a.H + c.h) * Nq;  // ... of lse and delta
  const int q0 = c.block * kTaQ + c.wave * 16;
  const bool wave_live = q0 < Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + c.row, Nq - 1);
  const TaViews at = ta_views_at(a.v, qb, kb, c.h * D);

  // Q[q][16 t + 4 g + c] and dO[q][16 t + 4 g + c]; the row's lse and delta
  ta_f32x4 qf[DB], gf[DB];
  ta_load_row<D>(at.q.p + (int64_t)qrow * at.q.sn + 4 * c.g, true, qf);
  ta_load_row<D>(a.grad_out + ((orow + qrow) * a.H + c.h) * D + 4 * c.g, true, gf);
  const float lse = a.lse[lrow + qrow];
  const float delta = a.delta[lrow + qrow];
  const float* krows = sk + c.row * LD + 4 * c.g;   // K[16 j + q][16 t + 4 g + c], and V at
  const float* vrows = sv + c.row * LD + 4 * c.g;   //   the same place
  const float* kcols = sk + 4 * c.g * LD + c.row;   // K[16 j + 4 g + r][16 d + q]

  ta_f32x4 kreg[PER], vreg[PER];  // the next tile's rows
  ta_f32x4 dq[DB];
  ta_zero(dq);

  const int tiles = (Nk + kTaK - 1) / kTaK;
  if (!CLIPS || tiles > 0) ta_fetch_kv<D>(at, 0, Nk1, Nk, kreg, vreg);  // (a clip without keys has no row 0 to read)
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta_stage<D>(sk, sv, kreg, vreg);
    __syncthreads();
    if (tile + 1 < tiles) ta_fetch_kv<D>(at, tile + 1, Nk1, Nk, kreg, vreg);
    if (!wave_live) continue;

    // S^T = K Q^T and dP^T = V dO^T: lane (q, g) gets the keys 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
    ta_zero(s), ta_zero(dp);
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      ta_rows_step<D>(krows + 16 * t, qf[t], s);
      ta_rows_step<D>(vrows + 16 * t, gf[t], dp);
    }

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
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) ta_cols_step<D>(kcols + (16 * j + r) * LD, s[j][r], dq);
  }
  if (!wave_live) return;
  if (q0 + c.row < Nq) {
    float* op = a.grad_q + ((orow + (q0 + c.row)) * a.H + c.h) * D + 4 * c.g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(op + 16 * d) = dq[d] * a.scale;
  }
}

// The dK/dV kernel's fetch: tile `tile` of the queries' Q rows (through the view) and dO rows (dense) into registers,
// with one row statistic pair per thread of the first wavefront's 64; ta_fetch_kv's rules, one segment.
template <int D>
__device__ __forceinline__ void ta_fetch_qg(const float* qp0, int64_t qs_n, const float* gp0, int64_t gs_n,
                                            const float* lsep, const float* deltap, int tile, int Nq,
                                            ta_f32x4 (&qreg)[TaTile<D>::PER], ta_f32x4 (&greg)[TaTile<D>::PER],
                                            float& lreg, float& dreg) {
#pragma unroll
  for (int i = 0; i < TaTile<D>::PER; ++i) {
    int row, c4;
    ta_piece<D>(i, row, c4);
    const int query = tile * kTaQ + row;
    const bool live = query < Nq;
    const int64_t idx = live ? query : 0;
    qreg[i] = ta_load_piece(qp0 + idx * qs_n + c4, live);
    greg[i] = ta_load_piece(gp0 + idx * gs_n + c4, live);
  }
  const int query = tile * kTaQ + ((int)threadIdx.x & (kTaQ - 1));
  const bool live = query < Nq;
  const float lx = lsep[live ? query : 0], dx = deltap[live ? query : 0];
  lreg = live ? lx : 0.0f;
  dreg = live ? dx : 0.0f;
}

template <int D, bool CLIPS>
__global__ __launch_bounds__(kBlock) void token_attention_bwd_dkv_kernel(TokenAttentionBwdArgs a) {
  constexpr int LD = TaTile<D>::LD, PER = TaTile<D>::PER, JB = TaTile<D>::JB, DB = TaTile<D>::DB;
  static_assert(kTaQ <= kBlock, "one thread per row statistic of a tile");
  __shared__ __attribute__((aligned(16))) float sq[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) float sg[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) float slse[kTaQ];
  __shared__ __attribute__((aligned(16))) float sdelta[kTaQ];

  const TaCoord c = ta_coord(a.blocks, a.H);
  const TaSegment qs = CLIPS ? ta_segment(a.clips.q_off, c.b, a.clips.Rq) : TaSegment{0, a.Nq};
  const TaSegment ks = CLIPS ? ta_segment(a.clips.k_off, c.b, a.clips.Rk) : TaSegment{0, a.Nk};
  const int Nq = qs.len, Nk = ks.len, Nk1 = CLIPS ? Nk : a.Nk1;
  if (CLIPS && c.block * kTaK >= Nk) return;
  const int64_t qb = CLIPS ? (int64_t)qs.first : c.b, kb = CLIPS ? (int64_t)ks.first : c.b;
  const int64_t lrow = CLIPS ? (int64_t)c.h * a.clips.Rq + qs.first : (c.b * a.H + c.h) * Nq;  // first of lse and delta
  const int tid = threadIdx.x;
  const int k0 = c.block * kTaK + c.wave * 16;
  const bool wave_live = k0 < Nk;  // wave-uniform: a wave past the last key only helps to stage
  const int key = k0 + c.row;
  const bool key_live = key < Nk, second = key_live && key >= Nk1;
  const int64_t kidx = second ? key - Nk1 : (key_live ? key : 0);

  // K[key][16 t + 4 g + c] and V[key][16 t + 4 g + c], from the key's segment; zeros past the last key
  ta_f32x4 kf[DB], vf[DB];
  {
    const TaView k1 = a.v.k1, v1 = a.v.v1, k2 = a.v.k2, v2 = a.v.v2;
    const float* kp = (second ? k2.p + kb * k2.sb + kidx * k2.sn : k1.p + kb * k1.sb + kidx * k1.sn) + c.h * D + 4 * c.g;
    const float* vp = (second ? v2.p + kb * v2.sb + kidx * v2.sn : v1.p + kb * v1.sb + kidx * v1.sn) + c.h * D + 4 * c.g;
    ta_load_row<D>(kp, key_live, kf);
    ta_load_row<D>(vp, key_live, vf);
  }

  const float* qp0 = a.v.q.p + qb * a.v.q.sb + c.h * D;
  const float* gp0 = a.grad_out + ((CLIPS ? (int64_t)qs.first * a.H : c.b * Nq * a.H) + c.h) * D;
  const float* lsep = a.lse + lrow;
  const float* deltap = a.delta + lrow;
  const float* qrows = sq + c.row * LD + 4 * c.g;   // Q[16 j + key][16 t + 4 g + c], and dO at
  const float* grows = sg + c.row * LD + 4 * c.g;   //   the same place
  const float* qcols = sq + 4 * c.g * LD + c.row;   // Q[16 j + 4 g + r][16 d + key], and dO at
  const float* gcols = sg + 4 * c.g * LD + c.row;   //   the same place

  // the next tile's Q and dO rows and row statistics
  ta_f32x4 qreg[PER], greg[PER];
  float lreg, dreg;
  ta_f32x4 dk[DB], dv[DB];
  ta_zero(dk), ta_zero(dv);

  const int tiles = (Nq + kTaQ - 1) / kTaQ;
  if (!CLIPS || tiles > 0)  // (a clip without queries has no row 0 to read)
    ta_fetch_qg<D>(qp0, a.v.q.sn, gp0, (int64_t)a.H * D, lsep, deltap, 0, Nq, qreg, greg, lreg, dreg);
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta_stage<D>(sq, sg, qreg, greg);
    if (tid < kTaQ) slse[tid] = lreg, sdelta[tid] = dreg;
    __syncthreads();
    if (tile + 1 < tiles)
      ta_fetch_qg<D>(qp0, a.v.q.sn, gp0, (int64_t)a.H * D, lsep, deltap, tile + 1, Nq, qreg, greg, lreg, dreg);
    if (!wave_live) continue;

    // S = Q K^T and dP = dO V^T: lane (key, g) gets the queries 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
    ta_zero(s), ta_zero(dp);
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      ta_rows_step<D>(qrows + 16 * t, kf[t], s);
      ta_rows_step<D>(grows + 16 * t, vf[t], dp);
    }

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
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ta_cols_step<D>(gcols + (16 * j + r) * LD, dp[j][r], dv);
        ta_cols_step<D>(qcols + (16 * j + r) * LD, s[j][r], dk);
      }
  }
  if (!wave_live || !key_live) return;
  // the key's gradients go to its segment: (B, Nk1, H, D) or (B, Nk2, H, D), either of which may not be wanted
  const int64_t nseg = second ? Nk - Nk1 : Nk1;
  const int64_t at = (((CLIPS ? (int64_t)ks.first : c.b * nseg) + kidx) * a.H + c.h) * D + 4 * c.g;
  float* gk = second ? a.grad_k2 : a.grad_k1;
  float* gv = second ? a.grad_v2 : a.grad_v1;
  if (gk) {
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(gk + at + 16 * d) = dk[d] * a.scale;
  }
  if (gv) {
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(gv + at + 16 * d) = dv[d];
  }
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_token_attention_bwd_limits(int* out, int n) { return ta_limits(out, n); }

extern "C" int waldo_token_attention_bwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                         int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                                         int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n,
                                         const float* out, const float* grad_out, const float* lse, float* delta,
                                         float* grad_q, float* grad_k1, float* grad_v1, float* grad_k2, float* grad_v2,
                                         float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                         waldo_stream_t stream) {
  const char* fn = "waldo_token_attention_bwd";
  TaViews v = {{q, qs_b, qs_n}, {k1, k1s_b, k1s_n}, {v1, v1s_b, v1s_n}, {k2, k2s_b, k2s_n}, {v2, v2s_b, v2s_n}};
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  const int64_t kblocks = ((int64_t)(Nk1 > 0 ? Nk1 : 0) + (Nk2 > 0 ? Nk2 : 0) + kTaK - 1) / kTaK;
  if (ta_check_shape(fn, v, scale, B, H, D, Nq, Nk1, Nk2, qblocks > kblocks ? qblocks : kblocks) != WALDO_OK)
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
  if (ta_check_pointers(fn, v, Nk2, out && grad_out && lse && delta,
                        {out, grad_out, lse, delta, grad_q, grad_k1, grad_v1, grad_k2, grad_v2}) != WALDO_OK)
    return WALDO_EINVAL;
  TokenAttentionBwdArgs a{};
  a.v = v, a.out = out, a.grad_out = grad_out, a.lse = lse, a.delta = delta;
  a.grad_q = grad_q, a.grad_k1 = grad_k1, a.grad_v1 = grad_v1, a.grad_k2 = grad_k2, a.grad_v2 = grad_v2;
  a.rows = rows, a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(kBlock);
  ta_for_head_dim(D, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    token_attention_delta_kernel<kD, false><<<dim3((unsigned)((rows + kBlock - 1) / kBlock)), block, 0, st>>>(a);
    if (grad_q) {
      a.blocks = (int)qblocks;
      token_attention_bwd_dq_kernel<kD, false><<<dim3((unsigned)(B * H * qblocks)), block, 0, st>>>(a);
    }
    if (grad_k1 || grad_v1 || grad_k2 || grad_v2) {
      a.blocks = (int)kblocks;
      token_attention_bwd_dkv_kernel<kD, false><<<dim3((unsigned)(B * H * kblocks)), block, 0, st>>>(a);
    }
  });
  return launch_status(fn);
}

extern "C" int waldo_token_attention_clips_bwd(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v,
                                               int64_t vs_n, const int* q_off, const int* k_off, const float* out,
                                               const float* grad_out, const float* lse, float* delta, float* grad_q,
                                               float* grad_k, float* grad_v, float scale, int64_t B, int H, int D,
                                               int64_t Rq, int64_t Rk, int max_q_len, int max_k_len,
                                               waldo_stream_t stream) {
  const char* fn = "waldo_token_attention_clips_bwd";
  TaViews vw = ta_clips_views(q, qs_n, k, ks_n, v, vs_n);
  const int64_t qblocks = ((int64_t)(max_q_len > 0 ? max_q_len : 0) + kTaQ - 1) / kTaQ;
  const int64_t kblocks = ((int64_t)(max_k_len > 0 ? max_k_len : 0) + kTaK - 1) / kTaK;
  if (ta_clips_check_shape(fn, vw, scale, B, H, D, Rq, Rk, max_q_len, max_k_len,
                           qblocks > kblocks ? qblocks : kblocks) != WALDO_OK)
    return WALDO_EINVAL;
  // the delta pass: a thread per (row, head) of out in blocks of kBlock
  const int64_t rows = Rq * H;
  if ((rows + kBlock - 1) / kBlock > INT32_MAX) {
    set_error("%s: too large: H=%d Rq=%lld (the rows of out stay below 2^31 blocks of %d)", fn, H, (long long)Rq, kBlock);
    return WALDO_EINVAL;
  }
  if (B == 0 || Rq == 0) return WALDO_OK;
  if (!grad_q && !grad_k && !grad_v) return WALDO_OK;
  if (ta_check_pointers(fn, vw, 0, out && grad_out && lse && delta && q_off && k_off,
                        {out, grad_out, lse, delta, grad_q, grad_k, grad_v}) != WALDO_OK)
    return WALDO_EINVAL;
  ta_clips_rows_as_batch(vw);
  TokenAttentionBwdArgs a{};
  a.v = vw, a.out = out, a.grad_out = grad_out, a.lse = lse, a.delta = delta;
  a.grad_q = grad_q, a.grad_k1 = grad_k, a.grad_v1 = grad_v;
  a.rows = rows, a.scale = scale, a.H = H;
  a.clips = {q_off, k_off, (int)Rq, (int)Rk};
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(kBlock);
  ta_for_head_dim(D, [&](auto d) {
    constexpr int kD = decltype(d)::value;
    token_attention_delta_kernel<kD, true><<<dim3((unsigned)((rows + kBlock - 1) / kBlock)), block, 0, st>>>(a);
    if (grad_q && qblocks > 0) {
      a.blocks = (int)qblocks;
      token_attention_bwd_dq_kernel<kD, true><<<dim3((unsigned)(B * H * qblocks)), block, 0, st>>>(a);
    }
    if ((grad_k || grad_v) && kblocks > 0) {
      a.blocks = (int)kblocks;
      token_attention_bwd_dkv_kernel<kD, true><<<dim3((unsigned)(B * H * kblocks)), block, 0, st>>>(a);
    }
  });
  return launch_status(fn);
}
