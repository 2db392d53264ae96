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
// All products run on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain).  Rows past Nq / Nk are read through a
// clamped index, staged as zeros, their P forced to 0, and never stored.
#include "token_attention_common.hip.h"

namespace waldo {

struct TokenAttentionBwdArgs {
  const float *q, *k1, *v1, *k2, *v2;
  const float *out, *grad_out, *lse;
  float* delta;
  float *grad_q, *grad_k1, *grad_v1, *grad_k2, *grad_v2;
  int64_t qs_b, qs_n, k1s_b, k1s_n, v1s_b, v1s_n, k2s_b, k2s_n, v2s_b, v2s_n;
  int64_t rows;  // B Nq H: the (token, head) rows of out
  float scale;
  int H, Nq, Nk1, Nk, blocks;  // Nk = Nk1 + Nk2; blocks: the kernel's row blocks per (b, h)
};

// delta[b, h, i] = sum_d grad_out[b, i, h, d] out[b, i, h, d]: one lane per row, ONE fma chain in the order in which the
// matrix instruction sums dP = dO . V in the two kernels below (d = 16 t + 4 g + c: t, then c, then the instruction's
// k index g).  Where a row has one key, P = 1 and O = V: delta and dP are then the same chain and dS = P (dP - delta)
// is exactly 0, as it is in exact arithmetic -- two different orders would leave a rounding residue in dQ and dK.
template <int D>
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
  const int64_t b = bi / a.Nq, i = bi % a.Nq;
  a.delta[(b * a.H + h) * a.Nq + i] = s;
}

template <int D>
__global__ __launch_bounds__(kBlock) void token_attention_bwd_dq_kernel(TokenAttentionBwdArgs a) {
  constexpr int LD = D + kTaPad;
  constexpr int V4 = D / 4;
  constexpr int PER = kTaK * V4 / kBlock;
  constexpr int JB = kTaK / 16, DB = D / 16;
  static_assert(kTaK * V4 % kBlock == 0, "a tile is a whole number of pieces per thread");
  __shared__ __attribute__((aligned(16))) float sk[kTaK * LD];
  __shared__ __attribute__((aligned(16))) float sv[kTaK * LD];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int qi = lane & 15, g = lane >> 4;
  const int qb = (int)(blockIdx.x % (unsigned)a.blocks);
  const int64_t bh = blockIdx.x / (unsigned)a.blocks;
  const int h = (int)(bh % a.H);
  const int64_t b = bh / a.H;
  const int q0 = qb * kTaQ + wave * 16;
  const bool wave_live = q0 < a.Nq;  // wave-uniform: a wave past the last row only helps to stage
  const int qrow = min(q0 + qi, a.Nq - 1);

  // Q[q][16 t + 4 g + c] and dO[q][16 t + 4 g + c]; the row's lse and delta
  ta_f32x4 qf[DB], gf[DB];
  {
    const float* qp = a.q + b * a.qs_b + (int64_t)qrow * a.qs_n + h * D + 4 * g;
    const float* gp = a.grad_out + ((b * a.Nq + qrow) * a.H + h) * D + 4 * g;
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      qf[t] = *reinterpret_cast<const ta_f32x4*>(qp + 16 * t);
      gf[t] = *reinterpret_cast<const ta_f32x4*>(gp + 16 * t);
    }
  }
  const float lse = a.lse[(b * a.H + h) * a.Nq + qrow];
  const float delta = a.delta[(b * a.H + h) * a.Nq + qrow];

  const float* k1p = a.k1 + b * a.k1s_b + h * D;
  const float* v1p = a.v1 + b * a.v1s_b + h * D;
  const float* k2p = a.k2 ? a.k2 + b * a.k2s_b + h * D : nullptr;
  const float* v2p = a.v2 ? a.v2 + b * a.v2s_b + h * D : nullptr;

  // the next tile's rows, in registers: compile-time indices, unconditional assignments (the forward's WALDO_TA_FETCH)
  ta_f32x4 kreg[PER], vreg[PER];
  const ta_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#define WALDO_TA_FETCH(TILE)                                                       \
  _Pragma("unroll") for (int i = 0; i < PER; ++i) {                                \
    const int e = tid + i * kBlock, row = e / V4, c4 = (e % V4) * 4;               \
    const int key = (TILE) * kTaK + row;                                           \
    const bool live = key < a.Nk, second = live && key >= a.Nk1;                   \
    const int64_t idx = second ? key - a.Nk1 : (live ? key : 0);                   \
    const float* kp = (second ? k2p + idx * a.k2s_n : k1p + idx * a.k1s_n) + c4;   \
    const float* vp = (second ? v2p + idx * a.v2s_n : v1p + idx * a.v1s_n) + c4;   \
    const ta_f32x4 kx = *reinterpret_cast<const ta_f32x4*>(kp);                    \
    const ta_f32x4 vx = *reinterpret_cast<const ta_f32x4*>(vp);                    \
    kreg[i] = live ? kx : zero4;                                                   \
    vreg[i] = live ? vx : zero4;                                                   \
  }

  ta_f32x4 dq[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) dq[d] = zero4;

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

    // S^T = K Q^T and dP^T = V dO^T: lane (q, g) gets the keys 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) s[j] = zero4, dp[j] = zero4;
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      ta_f32x4 kf[JB];
#pragma unroll
      for (int j = 0; j < JB; ++j) kf[j] = *reinterpret_cast<const ta_f32x4*>(sk + (16 * j + qi) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][c], qf[t][c], s[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < JB; ++j) kf[j] = *reinterpret_cast<const ta_f32x4*>(sv + (16 * j + qi) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) dp[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][c], gf[t][c], dp[j], 0, 0, 0);
    }

    // dS = P (dP - delta), in place of S; a key past the end has P = 0
    const int key0 = tile * kTaK + 4 * g;
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = key0 + 16 * j + r < a.Nk ? __expf(s[j][r] * a.scale - lse) : 0.0f;
        s[j][r] = p * (dp[j][r] - delta);
      }

    // dQ^T = K^T dS^T
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* kp = sk + (16 * j + 4 * g + r) * LD + qi;
#pragma unroll
        for (int d = 0; d < DB; ++d) dq[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[16 * d], s[j][r], dq[d], 0, 0, 0);
      }
  }
#undef WALDO_TA_FETCH
  if (!wave_live) return;
  if (q0 + qi < a.Nq) {
    float* op = a.grad_q + ((b * a.Nq + (q0 + qi)) * a.H + h) * D + 4 * g;
#pragma unroll
    for (int d = 0; d < DB; ++d) *reinterpret_cast<ta_f32x4*>(op + 16 * d) = dq[d] * a.scale;
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void token_attention_bwd_dkv_kernel(TokenAttentionBwdArgs a) {
  constexpr int LD = D + kTaPad;
  constexpr int V4 = D / 4;
  constexpr int PER = kTaQ * V4 / kBlock;
  constexpr int JB = kTaQ / 16, DB = D / 16;
  static_assert(kTaQ * V4 % kBlock == 0, "a tile is a whole number of pieces per thread");
  static_assert(kTaQ <= kBlock, "one thread per row statistic of a tile");
  __shared__ __attribute__((aligned(16))) float sq[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) float sg[kTaQ * LD];
  __shared__ __attribute__((aligned(16))) float slse[kTaQ];
  __shared__ __attribute__((aligned(16))) float sdelta[kTaQ];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int ki = lane & 15, g = lane >> 4;
  const int kb = (int)(blockIdx.x % (unsigned)a.blocks);
  const int64_t bh = blockIdx.x / (unsigned)a.blocks;
  const int h = (int)(bh % a.H);
  const int64_t b = bh / a.H;
  const int k0 = kb * kTaK + wave * 16;
  const bool wave_live = k0 < a.Nk;  // wave-uniform: a wave past the last key only helps to stage
  const int key = k0 + ki;
  const bool key_live = key < a.Nk, second = key_live && key >= a.Nk1;
  const int64_t kidx = second ? key - a.Nk1 : (key_live ? key : 0);

  // K[key][16 t + 4 g + c] and V[key][16 t + 4 g + c], from the key's segment; zeros past the last key
  ta_f32x4 kf[DB], vf[DB];
  const ta_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  {
    const float* kp = (second ? a.k2 + b * a.k2s_b + kidx * a.k2s_n : a.k1 + b * a.k1s_b + kidx * a.k1s_n) + h * D + 4 * g;
    const float* vp = (second ? a.v2 + b * a.v2s_b + kidx * a.v2s_n : a.v1 + b * a.v1s_b + kidx * a.v1s_n) + h * D + 4 * g;
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      const ta_f32x4 kx = *reinterpret_cast<const ta_f32x4*>(kp + 16 * t);
      const ta_f32x4 vx = *reinterpret_cast<const ta_f32x4*>(vp + 16 * t);
      kf[t] = key_live ? kx : zero4;
      vf[t] = key_live ? vx : zero4;
    }
  }

  const float* qp0 = a.q + b * a.qs_b + h * D;
  const float* gp0 = a.grad_out + (b * a.Nq * a.H + h) * D;
  const float* lsep = a.lse + (b * a.H + h) * a.Nq;
  const float* deltap = a.delta + (b * a.H + h) * a.Nq;

  // the next tile's Q and dO rows and row statistics, in registers (compile-time indices, unconditional assignments)
  ta_f32x4 qreg[PER], greg[PER];
  float lreg, dreg;
#define WALDO_TA_FETCH(TILE)                                                                              \
  _Pragma("unroll") for (int i = 0; i < PER; ++i) {                                                       \
    const int e = tid + i * kBlock, row = e / V4, c4 = (e % V4) * 4;                                      \
    const int query = (TILE) * kTaQ + row;                                                                \
    const bool live = query < a.Nq;                                                                       \
    const int64_t idx = live ? query : 0;                                                                 \
    const ta_f32x4 qx = *reinterpret_cast<const ta_f32x4*>(qp0 + idx * a.qs_n + c4);                      \
    const ta_f32x4 gx = *reinterpret_cast<const ta_f32x4*>(gp0 + idx * a.H * D + c4);                     \
    qreg[i] = live ? qx : zero4;                                                                          \
    greg[i] = live ? gx : zero4;                                                                          \
  }                                                                                                       \
  {                                                                                                       \
    const int query = (TILE) * kTaQ + (tid & (kTaQ - 1));                                                 \
    const bool live = query < a.Nq;                                                                       \
    const float lx = lsep[live ? query : 0], dx = deltap[live ? query : 0];                               \
    lreg = live ? lx : 0.0f;                                                                              \
    dreg = live ? dx : 0.0f;                                                                              \
  }

  ta_f32x4 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) dk[d] = zero4, dv[d] = zero4;

  const int tiles = (a.Nq + kTaQ - 1) / kTaQ;
  WALDO_TA_FETCH(0)
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + i * kBlock, row = e / V4, c4 = (e % V4) * 4;
      *reinterpret_cast<ta_f32x4*>(sq + row * LD + c4) = qreg[i];
      *reinterpret_cast<ta_f32x4*>(sg + row * LD + c4) = greg[i];
    }
    if (tid < kTaQ) slse[tid] = lreg, sdelta[tid] = dreg;
    __syncthreads();
    if (tile + 1 < tiles) {
      WALDO_TA_FETCH(tile + 1)
    }
    if (!wave_live) continue;

    // S = Q K^T and dP = dO V^T: lane (key, g) gets the queries 16 j + 4 g + r
    ta_f32x4 s[JB], dp[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) s[j] = zero4, dp[j] = zero4;
#pragma unroll
    for (int t = 0; t < DB; ++t) {
      ta_f32x4 rf[JB];
#pragma unroll
      for (int j = 0; j < JB; ++j) rf[j] = *reinterpret_cast<const ta_f32x4*>(sq + (16 * j + ki) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rf[j][c], kf[t][c], s[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < JB; ++j) rf[j] = *reinterpret_cast<const ta_f32x4*>(sg + (16 * j + ki) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) dp[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rf[j][c], vf[t][c], dp[j], 0, 0, 0);
    }

    // P into dp's place and dS into s's; a query past the end has P = 0 (not exp of an lse that was never read)
    const int query0 = tile * kTaQ + 4 * g;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const ta_f32x4 l4 = *reinterpret_cast<const ta_f32x4*>(slse + 16 * j + 4 * g);
      const ta_f32x4 d4 = *reinterpret_cast<const ta_f32x4*>(sdelta + 16 * j + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = query0 + 16 * j + r < a.Nq ? __expf(s[j][r] * a.scale - l4[r]) : 0.0f;
        s[j][r] = p * (dp[j][r] - d4[r]);
        dp[j][r] = p;
      }
    }

    // dV^T = dO^T P and dK^T = Q^T dS
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* gp = sg + (16 * j + 4 * g + r) * LD + ki;
        const float* qp = sq + (16 * j + 4 * g + r) * LD + ki;
#pragma unroll
        for (int d = 0; d < DB; ++d) dv[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(gp[16 * d], dp[j][r], dv[d], 0, 0, 0);
#pragma unroll
        for (int d = 0; d < DB; ++d) dk[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(qp[16 * d], s[j][r], dk[d], 0, 0, 0);
      }
  }
#undef WALDO_TA_FETCH
  if (!wave_live || !key_live) return;
  // the key's gradients go to its segment: (B, Nk1, H, D) or (B, Nk2, H, D), either of which may not be wanted
  const int64_t nseg = second ? a.Nk - a.Nk1 : a.Nk1;
  const int64_t at = ((b * nseg + kidx) * a.H + h) * D + 4 * g;
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

extern "C" int waldo_token_attention_bwd_limits(int* out, int n) {
  // {query rows per workgroup of the dQ kernel = queries per tile of the dK/dV kernel, keys per tile of the dQ kernel =
  //  keys per workgroup of the dK/dV kernel, the head dimensions served}
  const int limits[5] = {kTaQ, kTaK, 16, 32, 64};
  for (int i = 0; i < 5 && i < n && out; ++i) out[i] = limits[i];
  return 5;
}

extern "C" int waldo_token_attention_bwd(const float* q, int64_t qs_b, int64_t qs_n, const float* k1, int64_t k1s_b,
                                         int64_t k1s_n, const float* v1, int64_t v1s_b, int64_t v1s_n, const float* k2,
                                         int64_t k2s_b, int64_t k2s_n, const float* v2, int64_t v2s_b, int64_t v2s_n,
                                         const float* out, const float* grad_out, const float* lse, float* delta,
                                         float* grad_q, float* grad_k1, float* grad_v1, float* grad_k2, float* grad_v2,
                                         float scale, int64_t B, int H, int D, int Nq, int Nk1, int Nk2,
                                         waldo_stream_t stream) {
  const char* fn = "waldo_token_attention_bwd";
  const int64_t strides[10] = {qs_b, qs_n, k1s_b, k1s_n, v1s_b, v1s_n, k2s_b, k2s_n, v2s_b, v2s_n};
  const int64_t qblocks = ((int64_t)Nq + kTaQ - 1) / kTaQ;
  const int64_t kblocks = ((int64_t)(Nk1 > 0 ? Nk1 : 0) + (Nk2 > 0 ? Nk2 : 0) + kTaK - 1) / kTaK;
  if (ta_check_shape(fn, strides, scale, B, H, D, Nq, Nk1, Nk2, qblocks > kblocks ? qblocks : kblocks) != WALDO_OK)
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
  if (!q || !k1 || !v1 || !out || !grad_out || !lse || !delta || (Nk2 > 0 && (!k2 || !v2))) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const void* ptrs[14] = {q, k1, v1, Nk2 > 0 ? k2 : nullptr, Nk2 > 0 ? v2 : nullptr, out, grad_out, lse, delta,
                          grad_q, grad_k1, grad_v1, grad_k2, grad_v2};
  for (const void* p : ptrs)
    if (!ta_aligned16(p)) {
      set_error("%s: pointer not aligned to 16 bytes", fn);
      return WALDO_EINVAL;
    }
  TokenAttentionBwdArgs a{};
  a.q = q, a.k1 = k1, a.v1 = v1, a.k2 = Nk2 > 0 ? k2 : nullptr, a.v2 = Nk2 > 0 ? v2 : nullptr;
  a.out = out, a.grad_out = grad_out, a.lse = lse, a.delta = delta;
  a.grad_q = grad_q, a.grad_k1 = grad_k1, a.grad_v1 = grad_v1, a.grad_k2 = grad_k2, a.grad_v2 = grad_v2;
  a.qs_b = qs_b, a.qs_n = qs_n, a.k1s_b = k1s_b, a.k1s_n = k1s_n, a.v1s_b = v1s_b, a.v1s_n = v1s_n;
  a.k2s_b = k2s_b, a.k2s_n = k2s_n, a.v2s_b = v2s_b, a.v2s_n = v2s_n;
  a.rows = rows, a.scale = scale, a.H = H, a.Nq = Nq, a.Nk1 = Nk1, a.Nk = Nk1 + Nk2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(kBlock);
  {
    const dim3 grid((unsigned)((rows + kBlock - 1) / kBlock));
    if (D == 16) token_attention_delta_kernel<16><<<grid, block, 0, st>>>(a);
    else if (D == 32) token_attention_delta_kernel<32><<<grid, block, 0, st>>>(a);
    else token_attention_delta_kernel<64><<<grid, block, 0, st>>>(a);
  }
  if (grad_q) {
    a.blocks = (int)qblocks;
    const dim3 grid((unsigned)(B * H * qblocks));
    if (D == 16) token_attention_bwd_dq_kernel<16><<<grid, block, 0, st>>>(a);
    else if (D == 32) token_attention_bwd_dq_kernel<32><<<grid, block, 0, st>>>(a);
    else token_attention_bwd_dq_kernel<64><<<grid, block, 0, st>>>(a);
  }
  if (grad_k1 || grad_v1 || grad_k2 || grad_v2) {
    a.blocks = (int)kblocks;
    const dim3 grid((unsigned)(B * H * kblocks));
    if (D == 16) token_attention_bwd_dkv_kernel<16><<<grid, block, 0, st>>>(a);
    else if (D == 32) token_attention_bwd_dkv_kernel<32><<<grid, block, 0, st>>>(a);
    else token_attention_bwd_dkv_kernel<64><<<grid, block, 0, st>>>(a);
  }
  return launch_status(fn);
}
