// Token attention on bf16 / fp16 operands (include/waldo_hip.h "Token attention", the _dt entry points): the forward of
// token_attention.hip -- the same workgroup (one (b, h), 64 query rows, 16 per wavefront), the same 64-key tiles, the
// same two TRANSPOSED products that let a lane own one query row from the scores to the store, the same online softmax
// -- on the 16-bit matrix instructions with fp32 accumulation (token_attention_16.hip.h).  The backward of the dense form
// is token_attention_16_bwd.hip.
//
// The arithmetic: a score is an fp32 sum of exact 16-bit products; scale, mask, the running maximum and the running sum
// l are fp32, and l sums the UNROUNDED p; p is rounded to the operand type only as the operand of the second product; o
// is accumulated and rescaled in fp32; one rounding to the operand type at the store.  Rows past the last key are
// zeros in LDS and their scores -inf.  No atomics, no workspace: the same bits from run to run.
//
// The _lse entry point is the same template with LSE: one more store, the row's m + log(l) of the scaled scores in
// fp32, from which the backward rebuilds the probabilities; out has the bits of the plain instance.
//
// The per-clip entry point is the same template with CLIPS (TaClips, ta_segment), as in the fp32 kernel; it has no _lse
// form (its backward stays the framework's recompute).
#include "token_attention_16.hip.h"

namespace waldo {

struct TokenAttention16Args {
  Ta16Views v;
  uint16_t* out;
  float* lse;  // LSE: (B, H, Nq)
  float scale;
  int H, Nq, Nk1, Nk, qblocks;  // Nk = Nk1 + Nk2
  TaClips clips;                // CLIPS: the lengths are the clip's own, Nq / Nk1 / Nk are not read
};

template <int D, bool BF, bool CLIPS, bool LSE>
__global__ __launch_bounds__(kBlock) void token_attention_16_fwd_kernel(TokenAttention16Args a) {
  constexpr int KLD = Ta16Tile<D>::KLD, VLD = Ta16Tile<D>::VLD, PER = Ta16Tile<D>::PER, JB = Ta16Tile<D>::JB,
                DB = Ta16Tile<D>::DB, QW = Ta16Tile<D>::QW;
  __shared__ __attribute__((aligned(16))) uint16_t sk[kTaK * KLD];
  __shared__ __attribute__((aligned(16))) uint16_t sv[kTaK * VLD];

  const TaCoord c = ta_coord(a.qblocks, a.H);
  const TaSegment qs = CLIPS ? ta_segment(a.clips.q_off, c.b, a.clips.Rq) : TaSegment{0, a.Nq};
  const TaSegment ks = CLIPS ? ta_segment(a.clips.k_off, c.b, a.clips.Rk) : TaSegment{0, a.Nk};
  const int Nq = qs.len, Nk = ks.len, Nk1 = CLIPS ? Nk : a.Nk1;
  if (CLIPS && c.block * kTaQ >= Nq) return;  // workgroup-uniform
  const int64_t qb = CLIPS ? (int64_t)qs.first : c.b, kb = CLIPS ? (int64_t)ks.first : c.b;
  const int64_t orow = CLIPS ? (int64_t)qs.first : c.b * Nq;  // first row of out
  const int q0 = c.block * kTaQ + c.wave * 16;
  const bool wave_live = q0 < Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + c.row, Nq - 1);
  const Ta16Views at = ta16_views_at(a.v, qb, kb, c.h * D);

  uint32_t qf[QW];
  ta16_load_q<D>(at.q.p + (int64_t)qrow * at.q.sn, c.g, qf);
  const uint16_t* krows = sk + c.row * KLD + (D == 16 ? 4 : 8) * c.g;
  const uint16_t* vblk = sv + (4 * c.g + (c.row >> 2)) * VLD + 4 * (c.row & 3);

  ta_u32x4 kreg[PER], vreg[PER];  // the next tile's rows
  ta_f32x4 o[DB];
  ta_zero(o);
  float m = -INFINITY, l = 0.0f;  // the row's running maximum; THIS LANE's part of its running sum

  const int tiles = (Nk + kTaK - 1) / kTaK;
  if (!CLIPS || tiles > 0) ta16_fetch_kv<D>(at, 0, Nk1, Nk, kreg, vreg);  // (a clip without keys has no row 0 to read)
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
    ta16_stage<D>(sk, sv, kreg, vreg);
    __syncthreads();
    if (tile + 1 < tiles) ta16_fetch_kv<D>(at, tile + 1, Nk1, Nk, kreg, vreg);
    if (!wave_live) continue;  // wave-uniform: the transposed reads below run with every lane

    ta_f32x4 s[JB];
    ta_zero(s);
    ta16_scores<D, BF>(krows, qf, s);

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
        psum += p;  // the unrounded p
      }
    l = l * alpha + psum;
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] *= alpha;

    ta16_values<D, BF>(vblk, s, o);
  }

  if (!wave_live) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q0 + c.row < Nq) {
    const float inv = 1.0f / l;
    uint16_t* op = a.out + ((orow + (q0 + c.row)) * a.H + c.h) * D + 4 * c.g;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const ta_f32x4 x = o[d] * inv;
      const ta_u32x2 w = {Ta16Type<BF>::round2(x[0], x[1]), Ta16Type<BF>::round2(x[2], x[3])};
      *reinterpret_cast<ta_u32x2*>(op + 16 * d) = w;
    }
    if constexpr (LSE) {
      if (c.g == 0) a.lse[(c.b * a.H + c.h) * Nq + (q0 + c.row)] = m + logf(l);
    }
  }
}

namespace {

template <bool CLIPS, bool LSE, class Grid>
void ta16_launch(int D, int dtype, Grid grid, hipStream_t st, const TokenAttention16Args& a) {
  ta_for_head_dim(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    if (dtype == WALDO_DTYPE_BF16) token_attention_16_fwd_kernel<DD, true, CLIPS, LSE><<<grid, dim3(kBlock), 0, st>>>(a);
    else token_attention_16_fwd_kernel<DD, false, CLIPS, LSE><<<grid, dim3(kBlock), 0, st>>>(a);
  });
}

// The dense forward's host half, with or without the row statistics.
template <bool LSE>
int ta16_fwd_host(const char* fn, const char* fp32_fn, Ta16Views v, void* out, float* lse, float scale, int64_t B, int H,
                  int D, int Nq, int Nk1, int Nk2, int dtype, waldo_stream_t stream) {
  if (ta16_check_dtype(fn, fp32_fn, dtype) != WALDO_OK) return WALDO_EINVAL;
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  if (ta16_check_shape(fn, v, scale, B, H, D, Nq, Nk1, Nk2, qblocks) != WALDO_OK) return WALDO_EINVAL;
  if (B == 0 || Nq == 0) return WALDO_OK;
  TaViews chk = ta16_as_checked(v);
  if (ta_check_pointers(fn, chk, Nk2, out != nullptr && (!LSE || lse != nullptr), {out, lse}) != WALDO_OK)
    return WALDO_EINVAL;
  if (Nk2 == 0) v.k2 = v.v2 = {nullptr, 0, 0};
  TokenAttention16Args a{};
  a.v = v, a.out = static_cast<uint16_t*>(out), a.lse = lse;
  a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2, a.qblocks = (int)qblocks;
  ta16_launch<false, LSE>(D, dtype, dim3((unsigned)(B * H * qblocks)), (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_token_attention_dt_limits(int* out, int n) { return ta_limits(out, n); }

extern "C" int waldo_token_attention_fwd_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b,
                                            int64_t k1s_n, const void* v1, int64_t v1s_b, int64_t v1s_n, const void* k2,
                                            int64_t k2s_b, int64_t k2s_n, const void* v2, int64_t v2s_b, int64_t v2s_n,
                                            void* out, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                            int dtype, waldo_stream_t stream) {
  auto u = [](const void* p) { return static_cast<const uint16_t*>(p); };
  return ta16_fwd_host<false>("waldo_token_attention_fwd_dt", "waldo_token_attention_fwd",
                              {{u(q), qs_b, qs_n}, {u(k1), k1s_b, k1s_n}, {u(v1), v1s_b, v1s_n}, {u(k2), k2s_b, k2s_n},
                               {u(v2), v2s_b, v2s_n}},
                              out, nullptr, scale, B, H, D, Nq, Nk1, Nk2, dtype, stream);
}

extern "C" int waldo_token_attention_fwd_lse_dt(const void* q, int64_t qs_b, int64_t qs_n, const void* k1, int64_t k1s_b,
                                                int64_t k1s_n, const void* v1, int64_t v1s_b, int64_t v1s_n,
                                                const void* k2, int64_t k2s_b, int64_t k2s_n, const void* v2,
                                                int64_t v2s_b, int64_t v2s_n, void* out, float* lse, float scale,
                                                int64_t B, int H, int D, int Nq, int Nk1, int Nk2, int dtype,
                                                waldo_stream_t stream) {
  auto u = [](const void* p) { return static_cast<const uint16_t*>(p); };
  return ta16_fwd_host<true>("waldo_token_attention_fwd_lse_dt", "waldo_token_attention_fwd_lse",
                             {{u(q), qs_b, qs_n}, {u(k1), k1s_b, k1s_n}, {u(v1), v1s_b, v1s_n}, {u(k2), k2s_b, k2s_n},
                              {u(v2), v2s_b, v2s_n}},
                             out, lse, scale, B, H, D, Nq, Nk1, Nk2, dtype, stream);
}

extern "C" int waldo_token_attention_clips_fwd_dt(const void* q, int64_t qs_n, const void* k, int64_t ks_n, const void* v,
                                                  int64_t vs_n, const int* q_off, const int* k_off, void* out,
                                                  float scale, int64_t B, int H, int D, int64_t Rq, int64_t Rk,
                                                  int max_q_len, int max_k_len, int dtype, waldo_stream_t stream) {
  const char* fn = "waldo_token_attention_clips_fwd_dt";
  if (ta16_check_dtype(fn, "waldo_token_attention_clips_fwd", dtype) != WALDO_OK) return WALDO_EINVAL;
  auto u = [](const void* p) { return static_cast<const uint16_t*>(p); };
  Ta16Views vw{{u(q), 0, qs_n}, {u(k), 0, ks_n}, {u(v), 0, vs_n}, {nullptr, 0, 0}, {nullptr, 0, 0}};
  const int64_t qblocks = ((int64_t)(max_q_len > 0 ? max_q_len : 0) + kTaQ - 1) / kTaQ;
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
      B * H > INT32_MAX || B * H * qblocks > INT32_MAX) {
    set_error("%s: too large: B=%lld H=%d Rq=%lld Rk=%lld max_q_len=%d max_k_len=%d (the rows and the %d-row blocks of "
              "all (clip, h) stay below 2^31)", fn, (long long)B, H, (long long)Rq, (long long)Rk, max_q_len, max_k_len,
              kTaQ);
    return WALDO_EINVAL;
  }
  const int64_t strides[6] = {0, qs_n, 0, ks_n, 0, vs_n};
  if (ta16_check_strides(fn, strides, 6) != WALDO_OK) return WALDO_EINVAL;
  if (B == 0 || Rq == 0) return WALDO_OK;
  TaViews chk = ta16_as_checked(vw);
  if (ta_check_pointers(fn, chk, 0, out && q_off && k_off, {out}) != WALDO_OK) return WALDO_EINVAL;
  if (qblocks == 0) return WALDO_OK;  // no clip has a query
  vw.q.sb = vw.q.sn, vw.k1.sb = vw.k1.sn, vw.v1.sb = vw.v1.sn;  // a view's row index in the batch index's place
  TokenAttention16Args a{};
  a.v = vw, a.out = static_cast<uint16_t*>(out);
  a.scale = scale, a.H = H, a.qblocks = (int)qblocks;
  a.clips = {q_off, k_off, (int)Rq, (int)Rk};
  ta16_launch<true, false>(D, dtype, dim3((unsigned)(B * H * qblocks)), (hipStream_t)stream, a);
  return launch_status(fn);
}
