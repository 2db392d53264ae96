// Plane norm (include/waldo_hip.h "Plane norm"): the non-convolution work of one UNet level (the reference's
// models/modules/conv.py: conv -> CustomNorm("ln2d") = GroupNorm(C, C) -> GELU, then torch.cat with the skip) as one
// entry point each way.  Statistics are per (n, c) PLANE of H W values.  The kernel bodies, for an element type E of
// the tensor-sized buffers (float, __bf16, _Float16); the instances are compiled in plane_norm.hip (float),
// plane_norm_bf16.hip and plane_norm_f16.hip.
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
//
// A 16-bit E is STORAGE only: a value is widened to fp32 on load (exact), every register, sum and statistic is fp32 and
// the arithmetic is the float instance's line for line; a result is rounded to nearest-even on the store (a NaN stays
// a NaN).  The regime boundaries count values, so a thread keeps the same number of fp32 registers per value.  The
// 16-byte form then carries 8 consecutive values per lane (not the float layout's 4 in 8 bytes: 8-byte per-lane stores
// of 16-bit rows are bound by store issue on this part), so the in-lane slots hold other elements than the float
// instance's and the sums are taken in another -- equally fixed -- order.
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

constexpr int kPnWaveR = 8;                     // values of a lane, wavefront regime
constexpr int kPnWaveMax = kWave * kPnWaveR;    // 512
constexpr int kPnMidR = 8;                      // values of a thread, small workgroup regime
constexpr int kPnMidMax = kBlock * kPnMidR;     // 2048
constexpr int kPnBigR = 32;                     // values of a thread, large workgroup regime and chunks
constexpr int kPnChunk = kBlock * kPnBigR;      // 8192
constexpr int kPnWaves = kBlock / kWave;
constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;

enum PlaneNormMode { kResident = 0, kPartial = 1, kApply = 2 };

__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// E as 16-byte accesses hold it: kN consecutive values
template <typename E>
struct PlanePack;
template <>
struct PlanePack<float> {
  static constexpr int kN = 4;
  typedef float type __attribute__((ext_vector_type(4)));
  typedef uint32_t bits;
};
template <>
struct PlanePack<__bf16> {
  static constexpr int kN = 8;
  typedef __bf16 type __attribute__((ext_vector_type(8)));
  typedef uint16_t bits;
};
template <>
struct PlanePack<_Float16> {
  static constexpr int kN = 8;
  typedef _Float16 type __attribute__((ext_vector_type(8)));
  typedef uint16_t bits;
};

template <typename E>
struct PlaneNormArgs {
  const E* x;
  int64_t xs_n, xs_c;
  const float* gamma;
  const float* beta;
  float eps;
  E* out;            // forward: the concatenated output; backward: grad_x
  int64_t os_n;      // batch stride of out (its channels are H W apart)
  float* mean;
  float* rstd;
  const E* go;       // backward: grad_out
  int64_t gs_n, gs_c;
  float* sums;       // backward: (P, 2)
  float* ws;         // chunk records: (P, S, 2)
  int64_t P;         // planes = N C
  int C, S;
  int64_t HW;
};

// slot k of thread t among T: vector form = V consecutive elements per 16-byte access (4 floats, 8 16-bit values),
// consecutive threads adjacent
template <int T, bool VEC, int V>
__device__ __forceinline__ int slot_index(int t, int k) {
  return VEC ? (((k / V) * T + t) * V + (k % V)) : k * T + t;
}

// n % V == 0 and p 16-byte aligned with VEC (the host's decision): i < n implies i + V - 1 < n.  Slots past n read as 0.
template <int R, int T, bool VEC, typename E>
__device__ __forceinline__ void load_slots(const E* __restrict__ p, int n, int t, float (&v)[R]) {
  constexpr int V = PlanePack<E>::kN;
  if constexpr (VEC) {
    typedef float wide __attribute__((ext_vector_type(V)));
#pragma unroll
    for (int q = 0; q < R / V; ++q) {
      const int i = (q * T + t) * V;
      wide w = {};
      if (i < n) {
        if constexpr (std::is_same_v<E, float>) w = *reinterpret_cast<const wide*>(p + i);
        else w = __builtin_convertvector(*reinterpret_cast<const typename PlanePack<E>::type*>(p + i), wide);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) v[V * q + j] = w[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * T + t;
      v[k] = i < n ? (float)p[i] : 0.0f;
    }
  }
}

template <int R, int T, bool VEC, typename E>
__device__ __forceinline__ void store_slots(E* __restrict__ p, int n, int t, const float (&v)[R]) {
  constexpr int V = PlanePack<E>::kN;
  if constexpr (VEC) {
    typedef float wide __attribute__((ext_vector_type(V)));
#pragma unroll
    for (int q = 0; q < R / V; ++q) {
      const int i = (q * T + t) * V;
      wide w;
#pragma unroll
      for (int j = 0; j < V; ++j) w[j] = v[V * q + j];
      if (i < n) {
        if constexpr (std::is_same_v<E, float>) *reinterpret_cast<wide*>(p + i) = w;
        else *reinterpret_cast<typename PlanePack<E>::type*>(p + i) = __builtin_convertvector(w, typename PlanePack<E>::type);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int i = k * T + t;
      if (i < n) p[i] = (E)v[k];
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
template <int R, int T, bool VEC, int V>
__device__ __forceinline__ void resident_stat(const float (&v)[R], int n, int t, float (*sh)[2], float& mean, float& m2) {
  float s = 0.0f, unused = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) s += v[k];
  group_sum2<T>(s, unused, sh);
  const float m0 = s / (float)n;
  float c = 0.0f, q = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const float d = slot_index<T, VEC, V>(t, k) < n ? v[k] - m0 : 0.0f;
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
template <int T, typename E>
__device__ __forceinline__ bool locate(const PlaneNormArgs<E>& a, int64_t& plane, int& chunk, int& t) {
  if constexpr (T == kWave) {
    plane = (int64_t)blockIdx.x * kPnWaves + threadIdx.x / kWave;
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

template <int R, int T, bool VEC, int MODE, typename E>
__global__ __launch_bounds__(kBlock) void plane_norm_fwd_kernel(PlaneNormArgs<E> a) {
  __shared__ float sh[kPnWaves][2];
  int64_t plane;
  int chunk, t;
  if (!locate<T>(a, plane, chunk, t)) return;  // (wave-uniform; the wavefront regime has no barrier)
  const int64_t bn = plane / a.C;
  const int c = (int)(plane - bn * a.C);
  const int64_t start = (int64_t)chunk * kPnChunk;
  const int n = (int)min64(T * R, a.HW - start);
  float v[R];
  load_slots<R, T, VEC>(a.x + bn * a.xs_n + c * a.xs_c + start, n, t, v);
  float mean, rstd;
  if constexpr (MODE != kApply) {
    float m2;
    resident_stat<R, T, VEC, PlanePack<E>::kN>(v, n, t, sh, mean, m2);
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
template <typename E>
__global__ __launch_bounds__(kBlock) void plane_norm_fwd_finish_kernel(PlaneNormArgs<E> a) {
  const int64_t plane = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (plane >= a.P) return;
  const float* rec = a.ws + plane * a.S * 2;
  float na = (float)min64(kPnChunk, a.HW), mean = rec[0], m2 = rec[1];
  for (int s = 1; s < a.S; ++s) {
    const float nb = (float)min64(kPnChunk, a.HW - (int64_t)s * kPnChunk);
    const float nt = na + nb, delta = rec[2 * s] - mean;
    mean = mean + delta * (nb / nt);
    m2 = (m2 + rec[2 * s + 1]) + delta * delta * (na * (nb / nt));
    na = nt;
  }
  a.mean[plane] = mean;
  a.rstd[plane] = 1.0f / sqrtf(m2 / (float)a.HW + a.eps);
}

template <int R, int T, bool VEC, int MODE, typename E>
__global__ __launch_bounds__(kBlock) void plane_norm_bwd_kernel(PlaneNormArgs<E> a) {
  __shared__ float sh[kPnWaves][2];
  int64_t plane;
  int chunk, t;
  if (!locate<T>(a, plane, chunk, t)) return;
  const int64_t bn = plane / a.C;
  const int c = (int)(plane - bn * a.C);
  const int64_t start = (int64_t)chunk * kPnChunk;
  const int n = (int)min64(T * R, a.HW - start);
  float xh[R], dz[R];
  load_slots<R, T, VEC>(a.x + bn * a.xs_n + c * a.xs_c + start, n, t, xh);
  load_slots<R, T, VEC>(a.go + bn * a.gs_n + c * a.gs_c + start, n, t, dz);
  const float mean = a.mean[plane], rstd = a.rstd[plane], g = a.gamma[c], b = a.beta[c];
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    // (a slot past n: xhat = 0 and dz = 0 * gelu'(beta) = 0, whatever the plane's mean and rstd)
    xh[k] = slot_index<T, VEC, PlanePack<E>::kN>(t, k) < n ? (xh[k] - mean) * rstd : 0.0f;
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

template <typename E>
__global__ __launch_bounds__(kBlock) void plane_norm_bwd_finish_kernel(PlaneNormArgs<E> a) {
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
template <bool VEC, typename E>
__global__ __launch_bounds__(kBlock) void plane_skip_copy_kernel(const E* __restrict__ skip, int64_t ss_n, int64_t ss_c,
                                                                 E* __restrict__ out, int64_t os_n, int C, int Cs, int S,
                                                                 int64_t HW) {
  typedef typename PlanePack<E>::bits bits;
  constexpr int V = PlanePack<E>::kN;
  const int64_t plane = (int64_t)blockIdx.x / S;
  const int chunk = (int)((int64_t)blockIdx.x - plane * S);
  const int64_t bn = plane / Cs;
  const int cs = (int)(plane - bn * Cs);
  const int64_t start = (int64_t)chunk * kPnChunk;
  const int n = (int)min64(kPnChunk, HW - start);
  const bits* src = reinterpret_cast<const bits*>(skip + bn * ss_n + cs * ss_c + start);
  bits* dst = reinterpret_cast<bits*>(out + bn * os_n + (int64_t)(C + cs) * HW + start);
  if constexpr (VEC) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (int i = threadIdx.x * V; i < n; i += kBlock * V)
      *reinterpret_cast<u32x4*>(dst + i) = *reinterpret_cast<const u32x4*>(src + i);
  } else {
    for (int i = threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
  }
}

template <int MODE, bool BWD, typename E>
void plane_norm_launch_regime(const PlaneNormArgs<E>& a, bool vec, hipStream_t st) {
#define WALDO_PN_LAUNCH(R, T, GRID)                                                                          \
  do {                                                                                                       \
    if constexpr (BWD) {                                                                                     \
      if (vec) plane_norm_bwd_kernel<R, T, true, MODE, E><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);  \
      else plane_norm_bwd_kernel<R, T, false, MODE, E><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);     \
    } else {                                                                                                 \
      if (vec) plane_norm_fwd_kernel<R, T, true, MODE, E><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);  \
      else plane_norm_fwd_kernel<R, T, false, MODE, E><<<dim3((unsigned)(GRID)), dim3(kBlock), 0, st>>>(a);     \
    }                                                                                                        \
  } while (0)
  if constexpr (MODE == kResident) {
    if (a.HW <= kPnWaveMax) WALDO_PN_LAUNCH(kPnWaveR, kWave, (a.P + kPnWaves - 1) / kPnWaves);
    else if (a.HW <= kPnMidMax) WALDO_PN_LAUNCH(kPnMidR, kBlock, a.P);
    else WALDO_PN_LAUNCH(kPnBigR, kBlock, a.P);
  } else {
    WALDO_PN_LAUNCH(kPnBigR, kBlock, a.P * a.S);
  }
#undef WALDO_PN_LAUNCH
}

// the launches of one call, forward or backward (a.S chunks per plane: 1 = resident)
template <typename E, bool BWD>
int plane_norm_run(const char* fn, const PlaneNormArgs<E>& a, bool vec, hipStream_t st) {
  if (a.S == 1) {
    plane_norm_launch_regime<kResident, BWD>(a, vec, st);
    return launch_status(fn);
  }
  plane_norm_launch_regime<kPartial, BWD>(a, vec, st);
  int rc = launch_status(fn);
  if (rc != WALDO_OK) return rc;
  const unsigned grid = (unsigned)((a.P + kBlock - 1) / kBlock);
  if (BWD) plane_norm_bwd_finish_kernel<E><<<dim3(grid), dim3(kBlock), 0, st>>>(a);
  else plane_norm_fwd_finish_kernel<E><<<dim3(grid), dim3(kBlock), 0, st>>>(a);
  rc = launch_status(fn);
  if (rc != WALDO_OK) return rc;
  plane_norm_launch_regime<kApply, BWD>(a, vec, st);
  return launch_status(fn);
}

// the copy of the skip into out's channels C .. C + Cs, over N Cs planes of S chunks
template <typename E>
int plane_skip_copy(const char* fn, const E* skip, int64_t ss_n, int64_t ss_c, E* out, int64_t os_n, int64_t N, int C,
                    int Cs, int S, int64_t HW, bool vec, hipStream_t st) {
  const unsigned grid = (unsigned)(N * Cs * S);
  if (vec) plane_skip_copy_kernel<true, E><<<dim3(grid), dim3(kBlock), 0, st>>>(skip, ss_n, ss_c, out, os_n, C, Cs, S, HW);
  else plane_skip_copy_kernel<false, E><<<dim3(grid), dim3(kBlock), 0, st>>>(skip, ss_n, ss_c, out, os_n, C, Cs, S, HW);
  return launch_status(fn);
}

// one compile unit per element type (the float instances: plane_norm.hip)
#define WALDO_PLANE_NORM_INSTANCES(PREFIX, E)                                                    \
  PREFIX template decltype(plane_norm_run<E, false>) plane_norm_run<E, false>;                   \
  PREFIX template decltype(plane_norm_run<E, true>) plane_norm_run<E, true>;                     \
  PREFIX template decltype(plane_skip_copy<E>) plane_skip_copy<E>;
WALDO_PLANE_NORM_INSTANCES(extern, float)
WALDO_PLANE_NORM_INSTANCES(extern, __bf16)
WALDO_PLANE_NORM_INSTANCES(extern, _Float16)

}  // namespace waldo
