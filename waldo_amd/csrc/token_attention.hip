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
// The _lse entry point is the same kernel template with one more store: the row's m + log(l) of the scaled scores, which
// the backward (token_attention_bwd.hip) rebuilds the probabilities from.
#include "token_attention_common.hip.h"

namespace waldo {

struct TokenAttentionArgs {
  const float *q, *k1, *v1, *k2, *v2;
  float *out, *lse;
  int64_t qs_b, qs_n, k1s_b, k1s_n, v1s_b, v1s_n, k2s_b, k2s_n, v2s_b, v2s_n;
  float scale;
  int H, Nq, Nk1, Nk, qblocks;  // Nk = Nk1 + Nk2
};

template <int D, bool LSE>
__global__ __launch_bounds__(kBlock) void token_attention_fwd_kernel(TokenAttentionArgs a) {
  constexpr int LD = D + kTaPad;          // LDS row, floats
  constexpr int V4 = D / 4;               // 16-byte pieces of a row
  constexpr int PER = kTaK * V4 / kBlock; // pieces of a tile per thread (4, 2, 1)
  constexpr int JB = kTaK / 16, DB = D / 16;
  static_assert(kTaK * V4 % kBlock == 0, "a tile is a whole number of pieces per thread");
  __shared__ __attribute__((aligned(16))) float sk[kTaK * LD];
  __shared__ __attribute__((aligned(16))) float sv[kTaK * LD];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int qi = lane & 15, g = lane >> 4;
  const int qb = (int)(blockIdx.x % (unsigned)a.qblocks);
  const int64_t bh = blockIdx.x / (unsigned)a.qblocks;
  const int h = (int)(bh % a.H);
  const int64_t b = bh / a.H;
  const int q0 = qb * kTaQ + wave * 16;
  const bool wave_live = q0 < a.Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + qi, a.Nq - 1);

  // Q[q][16 t + 4 g + c]
  ta_f32x4 qf[DB];
  {
    const float* qp = a.q + b * a.qs_b + (int64_t)qrow * a.qs_n + h * D + 4 * g;
#pragma unroll
    for (int t = 0; t < DB; ++t) qf[t] = *reinterpret_cast<const ta_f32x4*>(qp + 16 * t);
  }

  const float* k1p = a.k1 + b * a.k1s_b + h * D;
  const float* v1p = a.v1 + b * a.v1s_b + h * D;
  const float* k2p = a.k2 ? a.k2 + b * a.k2s_b + h * D : nullptr;
  const float* v2p = a.v2 ? a.v2 + b * a.v2s_b + h * D : nullptr;

  // the next tile's rows, in registers: every index below is a compile-time constant and every assignment
  // unconditional (a branch per segment that writes the arrays sends them to scratch memory)
  ta_f32x4 kreg[PER], vreg[PER];
  const ta_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#define WALDO_TA_FETCH(TILE)                                                                              \
  _Pragma("unroll") for (int i = 0; i < PER; ++i) {                                                       \
    const int e = tid + i * kBlock, row = e / V4, c4 = (e % V4) * 4;                                      \
    const int key = (TILE) * kTaK + row;                                                                  \
    const bool live = key < a.Nk, second = live && key >= a.Nk1;                                          \
    /* past the last key: row 0 of the first segment is read and dropped (the scores are masked; 0 * v */ \
    /* must stay 0, so the rows staged are zeros)                                                      */ \
    const int64_t idx = second ? key - a.Nk1 : (live ? key : 0);                                          \
    const float* kp = (second ? k2p + idx * a.k2s_n : k1p + idx * a.k1s_n) + c4;                          \
    const float* vp = (second ? v2p + idx * a.v2s_n : v1p + idx * a.v1s_n) + c4;                          \
    const ta_f32x4 kx = *reinterpret_cast<const ta_f32x4*>(kp);                                           \
    const ta_f32x4 vx = *reinterpret_cast<const ta_f32x4*>(vp);                                           \
    kreg[i] = live ? kx : zero4;                                                                          \
    vreg[i] = live ? vx : zero4;                                                                          \
  }

  ta_f32x4 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o[d] = (ta_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;  // the row's running maximum; THIS LANE's part of its running sum

  const int tiles = (a.Nk + kTaK - 1) / kTaK;
  WALDO_TA_FETCH(0)
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + i * kBlock, row = e / V4, c4 = (e % V4) * 4;
      *reinterpret_cast<ta_f32x4*>(sk + row * LD + c4) = kreg[i];
      *reinterpret_cast<ta_f32x4*>(sv + row * LD + c4) = vreg[i];
    }
    __syncthreads();
    if (tile + 1 < tiles) {
      WALDO_TA_FETCH(tile + 1)
    }
    if (!wave_live) continue;

    ta_f32x4 s[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) s[j] = (ta_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      ta_f32x4 kf[JB];
#pragma unroll
      for (int j = 0; j < JB; ++j) kf[j] = *reinterpret_cast<const ta_f32x4*>(sk + (16 * j + qi) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][c], qf[t][c], s[j], 0, 0, 0);
    }

    // scale, mask the keys past the end, the tile's row maximum (4 JB values here, the rest in the lanes q + 16 g')
    const int key0 = tile * kTaK + 4 * g;
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = key0 + 16 * j + r < a.Nk ? s[j][r] * a.scale : -INFINITY;
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

#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vp = sv + (16 * j + 4 * g + r) * LD + qi;
#pragma unroll
        for (int d = 0; d < DB; ++d) o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * d], s[j][r], o[d], 0, 0, 0);
      }
  }

#undef WALDO_TA_FETCH
  if (!wave_live) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q0 + qi < a.Nq) {
    const float inv = 1.0f / l;
    float* op = a.out + ((b * a.Nq + (q0 + qi)) * a.H + h) * D + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(op + 16 * d) = o[d] * inv;
    if (LSE && g == 0) a.lse[(b * a.H + h) * a.Nq + (q0 + qi)] = m + logf(l);
  }
}

namespace {

template <bool LSE>
int token_attention_fwd_host(const char* fn, const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                             int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                             int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n, float* out,
                             float* lse, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                             waldo_stream_t stream) {
  const int64_t strides[10] = {qs_b, qs_n, k1s_b, k1s_n, v1s_b, v1s_n, k2s_b, k2s_n, v2s_b, v2s_n};
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  if (ta_check_shape(fn, strides, scale, B, H, D, Nq, Nk1, Nk2, qblocks) != WALDO_OK) return WALDO_EINVAL;
  if (B == 0 || Nq == 0) return WALDO_OK;
  if (!q || !k1 || !v1 || !out || (LSE && !lse) || (Nk2 > 0 && (!k2 || !v2))) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!ta_aligned16(q) || !ta_aligned16(k1) || !ta_aligned16(v1) || !ta_aligned16(out) ||
      (Nk2 > 0 && (!ta_aligned16(k2) || !ta_aligned16(v2)))) {
    set_error("%s: pointer not aligned to 16 bytes", fn);
    return WALDO_EINVAL;
  }
  TokenAttentionArgs a{};
  a.q = q, a.k1 = k1, a.v1 = v1, a.k2 = Nk2 > 0 ? k2 : nullptr, a.v2 = Nk2 > 0 ? v2 : nullptr, a.out = out;
  a.lse = lse;
  a.qs_b = qs_b, a.qs_n = qs_n, a.k1s_b = k1s_b, a.k1s_n = k1s_n, a.v1s_b = v1s_b, a.v1s_n = v1s_n;
  a.k2s_b = k2s_b, a.k2s_n = k2s_n, a.v2s_b = v2s_b, a.v2s_n = v2s_n;
  a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2, a.qblocks = (int)qblocks;
  const dim3 grid((unsigned)(B * H * qblocks));
  hipStream_t st = (hipStream_t)stream;
  if (D == 16) token_attention_fwd_kernel<16, LSE><<<grid, dim3(kBlock), 0, st>>>(a);
  else if (D == 32) token_attention_fwd_kernel<32, LSE><<<grid, dim3(kBlock), 0, st>>>(a);
  else token_attention_fwd_kernel<64, LSE><<<grid, dim3(kBlock), 0, st>>>(a);
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_token_attention_limits(int* out, int n) {
  const int limits[5] = {kTaQ, kTaK, 16, 32, 64};
  for (int i = 0; i < 5 && i < n && out; ++i) out[i] = limits[i];
  return 5;
}

extern "C" int waldo_token_attention_fwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                         int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                                         int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n,
                                         float* out, float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                         waldo_stream_t stream) {
  return token_attention_fwd_host<false>("waldo_token_attention_fwd", q, qs_b, qs_n, k1, k1s_b, k1s_n, v1, v1s_b, v1s_n,
                                         k2, k2s_b, k2s_n, v2, v2s_b, v2s_n, out, nullptr, scale, B, H, D, Nq, Nk1, Nk2,
                                         stream);
}

extern "C" int waldo_token_attention_fwd_lse(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                             int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n,
                                             const float* k2, int64_t k2s_b, int64_t k2s_n, const float* v2,
                                             int64_t v2s_b, int64_t v2s_n, float* out, float* lse, float scale, int64_t B,
                                             int H, int D, int Nq, int Nk1, int Nk2, waldo_stream_t stream) {
  return token_attention_fwd_host<true>("waldo_token_attention_fwd_lse", q, qs_b, qs_n, k1, k1s_b, k1s_n, v1, v1s_b,
                                        v1s_n, k2, k2s_b, k2s_n, v2, v2s_b, v2s_n, out, lse, scale, B, H, D, Nq, Nk1,
                                        Nk2, stream);
}
