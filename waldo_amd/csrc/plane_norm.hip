// Plane norm (include/waldo_hip.h "Plane norm"): the non-convolution work of one UNet level (the reference's
// models/modules/conv.py: conv -> CustomNorm("ln2d") = GroupNorm(C, C) -> GELU, then torch.cat with the skip) as one
// entry point each way.  Statistics are per (n, c) PLANE of H W values.
//
// A thread keeps its share of a plane in REGISTERS, so the statistics are a true two-pass (sum -> mean, a correction
// of the mean from the residuals, then the squared residuals): never E[x^2] - E[x]^2.  Three regimes by H W
// (waldo_plane_norm_limits reports the boundaries):
//   H W <= 512            one WAVEFRONT per plane, four planes per workgroup, up to 8 values per lane; no barrier;
//   H W <= 2048 / 8192    one WORKGROUP per plane, up to 8 / 32 values per thread; x read once;
//   H W >  8192           the plane is cut into chunks of 8192, one workgroup each (a plane per workgroup would leave
//                         most of the 256 CUs idle at the recipe's 128 planes of 512 x 1024): launch 1 leaves every
//                         chunk's (mean, M2) -- backward: (sum dz, sum dz xhat) -- in the workspace, launch 2 (one
//                         thread per plane) combines a plane's chunks in ascending order (Chan's pairwise update),
//                         launch 3 reads the chunk again and writes.  Two reads and one write of x-sized data.
// Every sum has a fixed order (in-lane slots ascending, a butterfly over the wavefront, waves 0..3, chunks ascending):
// no atomics, the same bits from run to run.  16-byte loads and stores when every plane base and H W allow them
// (decided on the host, uniform over the launch), element accesses otherwise.
#include "waldo_common.hip.h"

namespace waldo {

namespace {

constexpr int kWaveR = 8;                   // values of a lane, wavefront regime
constexpr int kWaveMax = kWave * kWaveR;    // 512
constexpr int kMidR = 8;                    // values of a thread, small workgroup regime
constexpr int kMidMax = kBlock * kMidR;     // 2048
constexpr int kBigR = 32;                   // values of a thread, large workgroup regime and chunks
constexpr int kChunk = kBlock * kBigR;      // 8192
constexpr int kWaves = kBlock / kWave;
constexpr int64_t kMaxHW = (int64_t)1 << 30;
constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;

enum Mode { kResident = 0, kPartial = 1, kApply = 2 };

__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

struct Args {
  const float* x;
  int64_t xs_n, xs_c;
  const float* gamma;
  const float* beta;
  float eps;
  float* out;        // forward: the concatenated output; backward: grad_x
  int64_t os_n;      // batch stride of out (its channels are H W apart)
  float* mean;
  float* rstd;
  const float* go;   // backward: grad_out
  int64_t gs_n, gs_c;
  float* sums;       // backward: (P, 2)
  float* ws;         // chunk records: (P, S, 2)
  int64_t P;         // planes = N C
  int C, S;
  int64_t HW;
};

// slot k of thread t among T: vector form = 4 consecutive elements per 16-byte access, consecutive threads adjacent
template <int T, bool VEC>
__device__ __forceinline__ int slot_index(int t, int k) {
  return VEC ? ((((k >> 2) * T + t) << 2) + (k & 3)) : k * T + t;
}

// n % 4 == 0 and p 16-byte aligned with VEC (the host's decision): i < n implies i + 3 < n.  Slots past n read as 0.
template <int R, int T, bool VEC>
__device__ __forceinline__ void load_slots(const float* __restrict__ p, int n, int t, float (&v)[R]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
      const int i = (q * T + t) << 2;
      f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (i < n) w = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = w[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * T + t;
      v[k] = i < n ? p[i] : 0.0f;
    }
  }
}

template <int R, int T, bool VEC>
__device__ __forceinline__ void store_slots(float* __restrict__ p, int n, int t, const float (&v)[R]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
      const int i = (q * T + t) << 2;
      if (i < n) *reinterpret_cast<f32x4*>(p + i) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * T + t;
      if (i < n) p[i] = v[k];
    }
  }
}

// the sums of a and b over the T threads of a group (a wavefront, or the workgroup: waves in the order 0..3), in all
template <int T>
__device__ __forceinline__ void group_sum2(float& a, float& b, float (*sh)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  if constexpr (T == kBlock) {
    __syncthreads();  // (sh may still be read from the previous call)
    if ((threadIdx.x & (kWave - 1)) == 0) {
      sh[threadIdx.x / kWave][0] = a;
      sh[threadIdx.x / kWave][1] = b;
    }
    __syncthreads();
    a = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
    b = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
  }
}

// mean and M2 = sum (v - mean)^2 of the n resident values: two passes over the registers, the mean corrected by the
// mean of the residuals (a constant plane then has mean == its value and M2 == 0 exactly)
template <int R, int T, bool VEC>
__device__ __forceinline__ void resident_stat(const float (&v)[R], int n, int t, float (*sh)[2], float& mean, float& m2) {
  float s = 0.0f, unused = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) s += v[k];
  group_sum2<T>(s, unused, sh);
  const float m0 = s / (float)n;
  float c = 0.0f, q = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const float d = slot_index<T, VEC>(t, k) < n ? v[k] - m0 : 0.0f;
    c += d;
    q += d * d;
  }
  group_sum2<T>(c, q, sh);
  const float dm = c / (float)n;
  mean = m0 + dm;
  m2 = fmaxf(q - c * dm, 0.0f);
}

__device__ __forceinline__ float gelu(float z) { return 0.5f * z * (1.0f + erff(z * kRsqrt2)); }
__device__ __forceinline__ float gelu_grad(float z) {
  return 0.5f * (1.0f + erff(z * kRsqrt2)) + z * (kRsqrt2Pi * expf(-0.5f * z * z));
}

// which plane and chunk this group works on; false: nothing (a wavefront past the last plane)
template <int T>
__device__ __forceinline__ bool locate(const Args& a, int64_t& plane, int& chunk, int& t) {
  if constexpr (T == kWave) {
    plane = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
    chunk = 0;
    t = threadIdx.x & (kWave - 1);
    return plane < a.P;
  } else {
    plane = (int64_t)blockIdx.x / a.S;
    chunk = (int)((int64_t)blockIdx.x - plane * a.S);
    t = threadIdx.x;
    return true;
  }
}

template <int R, int T, bool VEC, int MODE>
__global__ __launch_bounds__(kBlock) void plane_norm_fwd_kernel(Args a) {
  __shared__ float sh[kWaves][2];
  int64_t plane;
  int chunk, t;
  if (!locate<T>(a, plane, chunk, t)) return;  // (wave-uniform; the wavefront regime has no barrier)
  const int64_t bn = plane / a.C;
  const int c = (int)(plane - bn * a.C);
  const int64_t start = (int64_t)chunk * kChunk;
  const int n = (int)min64(T * R, a.HW - start);
  float v[R];
  load_slots<R, T, VEC>(a.x + bn * a.xs_n + c * a.xs_c + start, n, t, v);
  float mean, rstd;
  if constexpr (MODE != kApply) {
    float m2;
    resident_stat<R, T, VEC>(v, n, t, sh, mean, m2);
    if constexpr (MODE == kPartial) {
      if (t == 0) {
        a.ws[(plane * a.S + chunk) * 2] = mean;
        a.ws[(plane * a.S + chunk) * 2 + 1] = m2;
      }
      return;
    }
    rstd = 1.0f / sqrtf(m2 / (float)n + a.eps);
    if (t == 0) {
      a.mean[plane] = mean;
      a.rstd[plane] = rstd;
    }
  } else {
    mean = a.mean[plane];
    rstd = a.rstd[plane];
  }
  const float g = a.gamma[c], b = a.beta[c];
#pragma unroll
  for (int k = 0; k < R; ++k) v[k] = gelu((v[k] - mean) * rstd * g + b);
  store_slots<R, T, VEC>(a.out + bn * a.os_n + c * a.HW + start, n, t, v);
}

// one thread per plane: the chunks' (mean, M2) combined in ascending order
__global__ __launch_bounds__(kBlock) void plane_norm_fwd_finish_kernel(Args a) {
  const int64_t plane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (plane >= a.P) return;
  const float* rec = a.ws + plane * a.S * 2;
  float na = (float)min64(kChunk, a.HW), mean = rec[0], m2 = rec[1];
  for (int s = 1; s < a.S; ++s) {
    const float nb = (float)min64(kChunk, a.HW - (int64_t)s * kChunk);
    const float nt = na + nb, delta = rec[2 * s] - mean;
    mean = mean + delta * (nb / nt);
    m2 = (m2 + rec[2 * s + 1]) + delta * delta * (na * (nb / nt));
    na = nt;
  }
  a.mean[plane] = mean;
  a.rstd[plane] = 1.0f / sqrtf(m2 / (float)a.HW + a.eps);
}

template <int R, int T, bool VEC, int MODE>
__global__ __launch_bounds__(kBlock) void plane_norm_bwd_kernel(Args a) {
  __shared__ float sh[kWaves][2];
  int64_t plane;
  int chunk, t;
  if (!locate<T>(a, plane, chunk, t)) return;
  const int64_t bn = plane / a.C;
  const int c = (int)(plane - bn * a.C);
  const int64_t start = (int64_t)chunk * kChunk;
  const int n = (int)min64(T * R, a.HW - start);
  float xh[R], dz[R];
  load_slots<R, T, VEC>(a.x + bn * a.xs_n + c * a.xs_c + start, n, t, xh);
  load_slots<R, T, VEC>(a.go + bn * a.gs_n + c * a.gs_c + start, n, t, dz);
  const float mean = a.mean[plane], rstd = a.rstd[plane], g = a.gamma[c], b = a.beta[c];
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    // (a slot past n: xhat = 0 and dz = 0 * gelu'(beta) = 0, whatever the plane's mean and rstd)
    xh[k] = slot_index<T, VEC>(t, k) < n ? (xh[k] - mean) * rstd : 0.0f;
    dz[k] = dz[k] * gelu_grad(xh[k] * g + b);
    if constexpr (MODE != kApply) {
      s1 += dz[k];
      s2 += dz[k] * xh[k];
    }
  }
  if constexpr (MODE != kApply) {
    group_sum2<T>(s1, s2, sh);
    float* dst = MODE == kPartial ? a.ws + (plane * a.S + chunk) * 2 : a.sums + plane * 2;
    if (t == 0) {
      dst[0] = s1;
      dst[1] = s2;
    }
    if constexpr (MODE == kPartial) return;
  } else {
    s1 = a.sums[plane * 2];
    s2 = a.sums[plane * 2 + 1];
  }
  const float inv = 1.0f / (float)a.HW, m1 = s1 * inv, m2 = s2 * inv, rg = rstd * g;
#pragma unroll
  for (int k = 0; k < R; ++k) xh[k] = rg * ((dz[k] - m1) - xh[k] * m2);
  store_slots<R, T, VEC>(a.out + plane * a.HW + start, n, t, xh);
}

__global__ __launch_bounds__(kBlock) void plane_norm_bwd_finish_kernel(Args a) {
  const int64_t plane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (plane >= a.P) return;
  const float* rec = a.ws + plane * a.S * 2;
  float s1 = rec[0], s2 = rec[1];
  for (int s = 1; s < a.S; ++s) {
    s1 += rec[2 * s];
    s2 += rec[2 * s + 1];
  }
  a.sums[plane * 2] = s1;
  a.sums[plane * 2 + 1] = s2;
}

// out[n, C + cs] = skip[n, cs], bit for bit: one workgroup per chunk of a plane
template <bool VEC>
__global__ __launch_bounds__(kBlock) void plane_skip_copy_kernel(const float* __restrict__ skip, int64_t ss_n, int64_t ss_c,
                                                                 float* __restrict__ out, int64_t os_n, int C, int Cs, int S,
                                                                 int64_t HW) {
  const int64_t plane = (int64_t)blockIdx.x / S;
  const int chunk = (int)((int64_t)blockIdx.x - plane * S);
  const int64_t bn = plane / Cs;
  const int cs = (int)(plane - bn * Cs);
  const int64_t start = (int64_t)chunk * kChunk;
  const int n = (int)min64(kChunk, HW - start);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(skip + bn * ss_n + cs * ss_c + start);
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + bn * os_n + (int64_t)(C + cs) * HW + start);
  if constexpr (VEC) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (int i = threadIdx.x * 4; i < n; i += kBlock * 4)
      *reinterpret_cast<u32x4*>(dst + i) = *reinterpret_cast<const u32x4*>(src + i);
  } else {
    for (int i = threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
  }
}

bool aligned(const void* p, unsigned to) { return ((uintptr_t)p & (to - 1)) == 0; }

// shape checks shared by the entry points and the workspace query; S = chunks of a plane (1: resident)
bool shape_ok(const char* fn, int64_t N, int C, int Cs, int H, int W, int64_t& HW, int& S) {
  if (N < 0 || C < 1 || Cs < 0 || H < 1 || W < 1) {
    set_error("%s: bad shape N=%lld C=%d Cs=%d H=%d W=%d (N, Cs >= 0; C, H, W >= 1)", fn, (long long)N, C, Cs, H, W);
    return false;
  }
  HW = (int64_t)H * W;
  if (HW > kMaxHW) {
    set_error("%s: too large: H W = %lld (at most 2^30)", fn, (long long)HW);
    return false;
  }
  S = HW > kChunk ? (int)((HW + kChunk - 1) / kChunk) : 1;
  const int64_t cmax = C > Cs ? C : Cs;
  // every plane index, workgroup index and chunk record index stays below 2^31 (the strides are the caller's, 64-bit)
  if (N > INT32_MAX || N * cmax > INT32_MAX || N * cmax * S > INT32_MAX) {
    set_error("%s: too large: N=%lld C=%d Cs=%d with %d chunks per plane is more than 2^31 - 1 workgroups", fn,
              (long long)N, C, Cs, S);
    return false;
  }
  return true;
}

int64_t workspace_bytes_of(int64_t P, int S) { return S > 1 ? P * S * 2 * (int64_t)sizeof(float) : 0; }

template <int MODE, bool BWD>
void launch_regime(const Args& a, bool vec, hipStream_t st) {
#define WALDO_PN_LAUNCH(R, T, GRID)                                                                       \
  do {                                                                                                    \
    if constexpr (BWD) {                                                                                  \
      if (vec) plane_norm_bwd_kernel<R, T, true, MODE><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);  \
      else plane_norm_bwd_kernel<R, T, false, MODE><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);     \
    } else {                                                                                              \
      if (vec) plane_norm_fwd_kernel<R, T, true, MODE><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);  \
      else plane_norm_fwd_kernel<R, T, false, MODE><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);     \
    }                                                                                                     \
  } while (0)
  if constexpr (MODE == kResident) {
    if (a.HW <= kWaveMax) WALDO_PN_LAUNCH(kWaveR, kWave, (a.P + kWaves - 1) / kWaves);
    else if (a.HW <= kMidMax) WALDO_PN_LAUNCH(kMidR, kBlock, a.P);
    else WALDO_PN_LAUNCH(kBigR, kBlock, a.P);
  } else {
    WALDO_PN_LAUNCH(kBigR, kBlock, a.P * a.S);
  }
#undef WALDO_PN_LAUNCH
}

template <bool BWD>
int run(const char* fn, const Args& a, bool vec, hipStream_t st) {
  if (a.S == 1) {
    launch_regime<kResident, BWD>(a, vec, st);
    return launch_status(fn);
  }
  launch_regime<kPartial, BWD>(a, vec, st);
  int rc = launch_status(fn);
  if (rc != WALDO_OK) return rc;
  const unsigned grid = (unsigned)((a.P + kBlock - 1) / kBlock);
  if (BWD) plane_norm_bwd_finish_kernel<<<dim3(grid), dim3(kBlock), 0, st>>>(a);
  else plane_norm_fwd_finish_kernel<<<dim3(grid), dim3(kBlock), 0, st>>>(a);
  rc = launch_status(fn);
  if (rc != WALDO_OK) return rc;
  launch_regime<kApply, BWD>(a, vec, st);
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_plane_norm_limits(int* out, int n) {
  const int limits[3] = {kWaveMax, kMidMax, kChunk};
  for (int i = 0; i < 3 && i < n && out; ++i) out[i] = limits[i];
  return 3;
}

extern "C" int64_t waldo_plane_norm_workspace_bytes(int64_t N, int C, int H, int W) {
  int64_t HW;
  int S;
  if (!shape_ok("waldo_plane_norm_workspace_bytes", N, C, 0, H, W, HW, S)) return -1;
  return workspace_bytes_of(N * C, S);
}

extern "C" int waldo_plane_norm_gelu_fwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                         float eps, const float* skip, int64_t ss_n, int64_t ss_c, float* out, int64_t os_n,
                                         float* mean, float* rstd, void* workspace, int64_t workspace_bytes, int64_t N, int C,
                                         int Cs, int H, int W, waldo_stream_t stream) {
  const char* fn = "waldo_plane_norm_gelu_fwd";
  int64_t HW;
  int S;
  if (!shape_ok(fn, N, C, Cs, H, W, HW, S)) return WALDO_EINVAL;
  if (xs_n < 0 || xs_c < 0 || ss_n < 0 || ss_c < 0 || os_n < 0) {
    set_error("%s: negative stride", fn);
    return WALDO_EINVAL;
  }
  if (!(eps >= 0.0f) || !(eps < INFINITY)) {
    set_error("%s: bad eps %g (finite, >= 0)", fn, (double)eps);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!x || !gamma || !beta || !out || !mean || !rstd || (Cs > 0 && !skip)) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!aligned(x, 4) || !aligned(gamma, 4) || !aligned(beta, 4) || !aligned(out, 4) || !aligned(mean, 4) ||
      !aligned(rstd, 4) || !aligned(skip, 4) || !aligned(workspace, 4)) {
    set_error("%s: pointer not aligned to 4 bytes", fn);
    return WALDO_EINVAL;
  }
  if (os_n < (int64_t)(C + Cs) * HW) {
    set_error("%s: bad stride: out's batch stride %lld is below (C + Cs) H W = %lld", fn, (long long)os_n,
              (long long)((int64_t)(C + Cs) * HW));
    return WALDO_EINVAL;
  }
  const int64_t P = N * C, need = workspace_bytes_of(P, S);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace too small: %lld bytes, %lld needed (waldo_plane_norm_workspace_bytes)", fn,
              (long long)(workspace ? workspace_bytes : 0), (long long)need);
    return WALDO_EINVAL;
  }
  Args a{};
  a.x = x, a.xs_n = xs_n, a.xs_c = xs_c, a.gamma = gamma, a.beta = beta, a.eps = eps;
  a.out = out, a.os_n = os_n, a.mean = mean, a.rstd = rstd, a.ws = static_cast<float*>(workspace);
  a.P = P, a.C = C, a.S = S, a.HW = HW;
  const bool dst_vec = HW % 4 == 0 && aligned(out, 16) && os_n % 4 == 0;
  const bool vec = dst_vec && aligned(x, 16) && xs_n % 4 == 0 && xs_c % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  int rc = run<false>(fn, a, vec, st);
  if (rc != WALDO_OK || Cs == 0) return rc;
  const unsigned grid = (unsigned)(N * Cs * S);
  if (dst_vec && aligned(skip, 16) && ss_n % 4 == 0 && ss_c % 4 == 0)
    plane_skip_copy_kernel<true><<<dim3(grid), dim3(kBlock), 0, st>>>(skip, ss_n, ss_c, out, os_n, C, Cs, S, HW);
  else
    plane_skip_copy_kernel<false><<<dim3(grid), dim3(kBlock), 0, st>>>(skip, ss_n, ss_c, out, os_n, C, Cs, S, HW);
  return launch_status(fn);
}

extern "C" int waldo_plane_norm_gelu_bwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                         const float* mean, const float* rstd, const float* grad_out, int64_t gs_n,
                                         int64_t gs_c, float* grad_x, float* sums, void* workspace, int64_t workspace_bytes,
                                         int64_t N, int C, int H, int W, waldo_stream_t stream) {
  const char* fn = "waldo_plane_norm_gelu_bwd";
  int64_t HW;
  int S;
  if (!shape_ok(fn, N, C, 0, H, W, HW, S)) return WALDO_EINVAL;
  if (xs_n < 0 || xs_c < 0 || gs_n < 0 || gs_c < 0) {
    set_error("%s: negative stride", fn);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!x || !gamma || !beta || !mean || !rstd || !grad_out || !grad_x || !sums) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!aligned(x, 4) || !aligned(gamma, 4) || !aligned(beta, 4) || !aligned(mean, 4) || !aligned(rstd, 4) ||
      !aligned(grad_out, 4) || !aligned(grad_x, 4) || !aligned(sums, 4) || !aligned(workspace, 4)) {
    set_error("%s: pointer not aligned to 4 bytes", fn);
    return WALDO_EINVAL;
  }
  const int64_t P = N * C, need = workspace_bytes_of(P, S);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace too small: %lld bytes, %lld needed (waldo_plane_norm_workspace_bytes)", fn,
              (long long)(workspace ? workspace_bytes : 0), (long long)need);
    return WALDO_EINVAL;
  }
  Args a{};
  a.x = x, a.xs_n = xs_n, a.xs_c = xs_c, a.gamma = gamma, a.beta = beta;
  a.out = grad_x, a.mean = const_cast<float*>(mean), a.rstd = const_cast<float*>(rstd);
  a.go = grad_out, a.gs_n = gs_n, a.gs_c = gs_c, a.sums = sums, a.ws = static_cast<float*>(workspace);
  a.P = P, a.C = C, a.S = S, a.HW = HW;
  const bool vec = HW % 4 == 0 && aligned(x, 16) && xs_n % 4 == 0 && xs_c % 4 == 0 && aligned(grad_out, 16) &&
                   gs_n % 4 == 0 && gs_c % 4 == 0 && aligned(grad_x, 16);
  return run<true>(fn, a, vec, (hipStream_t)stream);
}
