// Token attention (include/waldo_hip.h "Token attention"): softmax(scale q k^T) v over one or two key / value segments,
// flash style -- no score matrix in memory, no workspace, no atomics.  Replaces the reference's matmul -> scale ->
// softmax -> matmul of FullAttention / ObjAttention (models/modules/transform.py:109-117, 175-185) with the permutes and
// cats around it: every operand is read through its strides where it lies.
//
// A workgroup is one (b, h) and kTaQ = 64 query rows, 16 per wavefront; the keys go by in tiles of kTaK = 64, staged in
// LDS (K and V, rows padded by 4 floats: the 16 rows a b128 read touches fall into 16 different bank quads).  Both
// products run on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain), and both TRANSPOSED, so that a lane owns
// one query row (q = lane & 15) from the scores to the output and the softmax needs two cross-lane steps per tile:
//   S^T (16 keys x 16 queries) = K Q^T:  a = K[16 j + (lane & 15)][d],  b = Q[lane & 15][d],  d = 16 t + 4 g + c with
//       g = lane >> 4 the instruction's k index: a lane's four d of a step are consecutive -- K from LDS and Q from
//       memory are 16-byte loads.  Lane (q, g) ends up with the scores of keys 16 j + 4 g + r, r = 0..3.
//   O^T (16 d x 16 queries) = V^T P^T:   a = V[16 j + 4 g + r][16 db + (lane & 15)],  b = P[q][16 j + 4 g + r] -- the
//       register the lane already holds: P never leaves the registers.  Lane (q, g) ends up with O[q][16 db + 4 g + r]:
//       four consecutive floats, one 16-byte store.
// The kTaK / 16 score blocks and the D / 16 output blocks are independent accumulator chains (the MFMA's dependent
// latency), and several workgroups share a CU.  The next tile's K and V rows are in flight (registers) while the
// current one is computed.
//
// The tile pipeline -- fetch, stage, the steps of the two products -- is token_attention_common.hip.h's, shared with the
// backward; here are the kernel's sequence of them and the online softmax between the two products.
//
// The _lse entry point is the same kernel template with one more store: the row's m + log(l) of the scaled scores, which
// the backward (token_attention_bwd.hip) rebuilds the probabilities from.
//
// The waldo_token_attention_clips_* entry points (include/waldo_hip.h "Token attention over clips") run the same
// template with CLIPS: b is a clip of PACKED rows whose first row and length come from offset tables in device memory.
#include "token_attention_common.hip.h"

namespace waldo {

struct TokenAttentionArgs {
  TaViews v;
  float *out, *lse;
  float scale;
  int H, Nq, Nk1, Nk, qblocks;  // Nk = Nk1 + Nk2
  TaClips clips;                // CLIPS: the lengths are the clip's own, Nq / Nk1 / Nk are not read
};

// CLIPS: b is a clip of packed rows (TaClips).  Its lengths come from the tables, a workgroup whose block starts at or
// past the clip's last query leaves before the first barrier (workgroup-uniform), out is (Rq, H D) and lse (H, Rq).  A
// clip without keys has no tile: o = 0 and l = 0 give its rows 0 * inf = NaN, the softmax of a row with every key
// masked.  Everything between is the dense kernel, which is the instantiation without a table read.
template <int D, bool LSE, bool CLIPS>
__global__ __launch_bounds__(kBlock) void token_attention_fwd_kernel(TokenAttentionArgs a) {
  constexpr int LD = TaTile<D>::LD, PER = TaTile<D>::PER, JB = TaTile<D>::JB, DB = TaTile<D>::DB;
  __shared__ __attribute__((aligned(16))) float sk[kTaK * LD];
  __shared__ __attribute__((aligned(16))) float sv[kTaK * LD];

  const TaCoord c = ta_coord(a.qblocks, a.H);
  const TaSegment qs = CLIPS ? ta_segment(a.clips.q_off, c.b, a.clips.Rq) : TaSegment{0, a.Nq};
  const TaSegment ks = CLIPS ? ta_segment(a.clips.k_off, c.b, a.clips.Rk) : TaSegment{0, a.Nk};
  const int Nq = qs.len, Nk = ks.len, Nk1 = CLIPS ? Nk : a.Nk1;
  if (CLIPS && c.block * kTaQ >= Nq) return;
  const int64_t qb = CLIPS ? (int64_t)qs.first : c.b, kb = CLIPS ? (int64_t)ks.first : c.b;
  const int64_t orow = CLIPS ? (int64_t)qs.first : c.b * Nq;                                        // first row of out
  const int64_t lrow = CLIPS ? (int64_t)c.h * a.clips.Rq + qs.first : (c.b * a.H + c.h) * Nq;      // ... and of lse
  const int q0 = c.block * kTaQ + c.wave * 16;
  const bool wave_live = q0 < Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + c.row, Nq - 1);
  const TaViews at = ta_views_at(a.v, qb, kb, c.h * D);

  ta_f32x4 qf[DB];  // Q[q][16 t + 4 g + c]
  ta_load_row<D>(at.q.p + (int64_t)qrow * at.q.sn + 4 * c.g, true, qf);
  const float* krows = sk + c.row * LD + 4 * c.g;    // K[16 j + q][16 t + 4 g + c]
  const float* vcols = sv + 4 * c.g * LD + c.row;    // V[16 j + 4 g + r][16 d + q]

  ta_f32x4 kreg[PER], vreg[PER];  // the next tile's rows
  ta_f32x4 o[DB];
  ta_zero(o);
  float m = -INFINITY, l = 0.0f;  // the row's running maximum; THIS LANE's part of its running sum

  const int tiles = (Nk + kTaK - 1) / kTaK;
  if (!CLIPS || tiles > 0) ta_fetch_kv<D>(at, 0, Nk1, Nk, kreg, vreg);  // (a clip without keys has no row 0 to read)
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta_stage<D>(sk, sv, kreg, vreg);
    __syncthreads();
    if (tile + 1 < tiles) ta_fetch_kv<D>(at, tile + 1, Nk1, Nk, kreg, vreg);
    if (!wave_live) continue;

    // S^T = K Q^T: lane (q, g) gets the keys 16 j + 4 g + r
    ta_f32x4 s[JB];
    ta_zero(s);
#pragma unroll
    for (int t = 0; t < DB; ++t) ta_rows_step<D>(krows + 16 * t, qf[t], s);

    // scale, mask the keys past the end, the tile's row maximum (4 JB values here, the rest in the lanes q + 16 g')
    const int key0 = tile * kTaK + 4 * c.g;
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = key0 + 16 * j + r < Nk ? s[j][r] * a.scale : -INFINITY;
        s[j][r] = x;
        tmax = fmaxf(tmax, x);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mnew = fmaxf(m, tmax);     // finite: every tile holds a live key
    const float alpha = __expf(m - mnew);  // (the first tile: exp(-inf) = 0 on o = 0, l = 0)
    m = mnew;
    float psum = 0.0f;
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(s[j][r] - mnew);
        s[j][r] = p;
        psum += p;
      }
    l = l * alpha + psum;
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] *= alpha;

    // O^T = V^T P^T
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) ta_cols_step<D>(vcols + (16 * j + r) * LD, s[j][r], o);
  }

  if (!wave_live) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q0 + c.row < Nq) {
    const float inv = 1.0f / l;
    float* op = a.out + ((orow + (q0 + c.row)) * a.H + c.h) * D + 4 * c.g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(op + 16 * d) = o[d] * inv;
    if (LSE && c.g == 0) a.lse[lrow + (q0 + c.row)] = m + logf(l);
  }
}

namespace {

template <bool LSE>
int token_attention_fwd_host(const char* fn, TaViews v, float* out, float* lse, float scale, int64_t B, int H, int D,
                             int Nq, int Nk1, int Nk2, waldo_stream_t stream) {
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  if (ta_check_shape(fn, v, scale, B, H, D, Nq, Nk1, Nk2, qblocks) != WALDO_OK) return WALDO_EINVAL;
  if (B == 0 || Nq == 0) return WALDO_OK;
  if (ta_check_pointers(fn, v, Nk2, out && (!LSE || lse), {out}) != WALDO_OK) return WALDO_EINVAL;
  TokenAttentionArgs a{};
  a.v = v, a.out = out, a.lse = lse;
  a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2, a.qblocks = (int)qblocks;
  const dim3 grid((unsigned)(B * H * qblocks));
  ta_for_head_dim(D, [&](auto d) {
    token_attention_fwd_kernel<decltype(d)::value, LSE, false><<<grid, dim3(kBlock), 0, (hipStream_t)stream>>>(a);
  });
  return launch_status(fn);
}

// The per-clip forward: the grid is sized by the caller's bound on a clip's queries, nothing here reads the tables.
template <bool LSE>
int token_attention_clips_fwd_host(const char* fn, TaViews v, const int* q_off, const int* k_off, float* out, float* lse,
                                   float scale, int64_t B, int H, int D, int64_t Rq, int64_t Rk, int max_q_len,
                                   int max_k_len, waldo_stream_t stream) {
  const int64_t qblocks = ((int64_t)(max_q_len > 0 ? max_q_len : 0) + kTaQ - 1) / kTaQ;
  if (ta_clips_check_shape(fn, v, scale, B, H, D, Rq, Rk, max_q_len, max_k_len, qblocks) != WALDO_OK)
    return WALDO_EINVAL;
  if (B == 0 || Rq == 0) return WALDO_OK;
  if (ta_check_pointers(fn, v, 0, out && (!LSE || lse) && q_off && k_off, {out}) != WALDO_OK) return WALDO_EINVAL;
  if (qblocks == 0) return WALDO_OK;  // no clip has a query
  ta_clips_rows_as_batch(v);
  TokenAttentionArgs a{};
  a.v = v, a.out = out, a.lse = lse;
  a.scale = scale, a.H = H, a.qblocks = (int)qblocks;
  a.clips = {q_off, k_off, (int)Rq, (int)Rk};
  const dim3 grid((unsigned)(B * H * qblocks));
  ta_for_head_dim(D, [&](auto d) {
    token_attention_fwd_kernel<decltype(d)::value, LSE, true><<<grid, dim3(kBlock), 0, (hipStream_t)stream>>>(a);
  });
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_token_attention_limits(int* out, int n) { return ta_limits(out, n); }

extern "C" int waldo_token_attention_fwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                         int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                                         int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n,
                                         float* out, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                         waldo_stream_t stream) {
  return token_attention_fwd_host<false>(
      "waldo_token_attention_fwd", {{q, qs_b, qs_n}, {k1, k1s_b, k1s_n}, {v1, v1s_b, v1s_n}, {k2, k2s_b, k2s_n},
                                    {v2, v2s_b, v2s_n}}, out, nullptr, scale, B, H, D, Nq, Nk1, Nk2, stream);
}

extern "C" int waldo_token_attention_fwd_lse(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                             int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n,
                                             const float* k2, int64_t k2s_b, int64_t k2s_n, const float* v2,
                                             int64_t v2s_b, int64_t v2s_n, float* out, float* lse, float scale, int64_t B,
                                             int H, int D, int Nq, int Nk1, int Nk2, waldo_stream_t stream) {
  return token_attention_fwd_host<true>(
      "waldo_token_attention_fwd_lse", {{q, qs_b, qs_n}, {k1, k1s_b, k1s_n}, {v1, v1s_b, v1s_n}, {k2, k2s_b, k2s_n},
                                        {v2, v2s_b, v2s_n}}, out, lse, scale, B, H, D, Nq, Nk1, Nk2, stream);
}

extern "C" int waldo_token_attention_clips_fwd(const float* q, int64_t qs_n, const float* k, int64_t ks_n, const float* v,
                                               int64_t vs_n, const int* q_off, const int* k_off, float* out, float scale,
                                               int64_t B, int H, int D, int64_t Rq, int64_t Rk, int max_q_len,
                                               int max_k_len, waldo_stream_t stream) {
  return token_attention_clips_fwd_host<false>("waldo_token_attention_clips_fwd",
                                               ta_clips_views(q, qs_n, k, ks_n, v, vs_n), q_off, k_off, out, nullptr,
                                               scale, B, H, D, Rq, Rk, max_q_len, max_k_len, stream);
}

extern "C" int waldo_token_attention_clips_fwd_lse(const float* q, int64_t qs_n, const float* k, int64_t ks_n,
                                                   const float* v, int64_t vs_n, const int* q_off, const int* k_off,
                                                   float* out, float* lse, float scale, int64_t B, int H, int D,
                                                   int64_t Rq, int64_t Rk, int max_q_len, int max_k_len,
                                                   waldo_stream_t stream) {
  return token_attention_clips_fwd_host<true>("waldo_token_attention_clips_fwd_lse",
                                              ta_clips_views(q, qs_n, k, ks_n, v, vs_n), q_off, k_off, out, lse, scale,
                                              B, H, D, Rq, Rk, max_q_len, max_k_len, stream);
}
