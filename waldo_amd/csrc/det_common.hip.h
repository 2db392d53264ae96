// Deterministic mode (include/waldo_hip.h "Reproducible gradients"): the two order-independent forms the *_det entry
// points are built from.
//
//   SLABS   small tables summed over all pixels (grad_occ, grad_dist, grad_mapping).  The pixel kernels already reduce
//           a workgroup's pixels to one partial table; their DET instances store that table to a row of a slab in the
//           workspace (plain stores, every row written exactly once: no zero fill) instead of issuing one float atomic
//           per entry, and slab_reduce_kernel sums the rows of one destination in an order that depends on the shapes
//           alone (the pattern of warp_composite_gmap_reduce_kernel).
//
//   SPLATS  bilinear scatters onto texels chosen by the data (grad_input of grid_sample2d, grad_a01 of flow_ctx_warp):
//           64-bit fixed point.  A first pass takes the largest contribution magnitude per destination plane
//           (atomicMax on the bit pattern of |x|: a maximum has no order; a NaN's pattern is above every number's, so
//           it survives), the splat adds llrint(contribution * 2^k) with integer atomics (integer sums have no order),
//           and a last pass converts the sums to fp32 with ONE rounding and overwrites the gradient.
//           k = 63 - ex - clog:  the plane's maximum is < 2^ex (frexp), a texel receives at most 2^clog contributions
//           (from the shapes, clog <= 32).  Every term is then an integer of magnitude < 2^(63 - clog), their sum stays
//           below 2^63 for ANY input, and one quantum 2^-k is at most 2^(clog - 62) <= 2^-30 of the plane's maximum.
//           The scale is a power of two that follows the maximum: doubling the incoming gradient doubles the result
//           exactly.  A plane whose maximum is infinite or NaN comes back all NaN (float -> integer is undefined there).
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

// ---- slabs -------------------------------------------------------------------------------------------------------
// out[dst(d) * E + e] = sum over the live parts of slab[row(d, part) * E + e].  A workgroup sums kSlabLanes entries of
// one destination: kSlabGroups thread groups take a contiguous share of the parts each (four running sums, combined in
// a fixed tree), then the group sums are added in group order.
constexpr int kSlabLanes = 32, kSlabGroups = kBlock / kSlabLanes;
// Pixel tiles a workgroup of a DET pixel kernel walks before it stores its row: a constant -- the default kernels pick
// theirs from the whole problem's size, which would make the slab (and the workspace query) shrink where a size grows.
constexpr int kDetTilesPerBlock = 4;

// rows d * nparts .. (d + 1) * nparts - 1 (those below `rows`); destination (d / dq) * dstride + d % dq
struct SlabPlain {
  int64_t rows, dq, dstride;
  __device__ __forceinline__ int64_t row(int64_t d, int part, int nparts) const {
    const int64_t r = d * nparts + part;
    return r < rows ? r : -1;
  }
  __device__ __forceinline__ int64_t dst(int64_t d) const { return (d / dq) * dstride + d % dq; }
};

// flow_ctx_warp_bwd: destination d = (b, t); part = (tc, tp, group) of unit (b, tc, tp), live when the unit's predicted
// frame pred_ts[tp] (clamped as the kernel clamps it) is t
struct SlabByPredFrame {
  const int64_t* pred_ts;
  int T, Tc, Tp, groups;
  __device__ __forceinline__ int64_t row(int64_t d, int part, int) const {
    const int g = part % groups, u = part / groups, tp = u % Tp, tc = u / Tp;
    const int64_t b = d / T;
    const int t = (int)(d % T);
    const int tpred = (int)min(max(pred_ts[tp], (int64_t)0), (int64_t)(T - 1));
    return tpred == t ? ((b * Tc + tc) * Tp + tp) * groups + g : -1;
  }
  __device__ __forceinline__ int64_t dst(int64_t d) const { return d; }
};

template <typename Map>
static __global__ __launch_bounds__(kBlock) void slab_reduce_kernel(const float* __restrict__ slab,
                                                                    float* __restrict__ out, int nparts, int E,
                                                                    int egroups, Map map) {
  const int64_t d = blockIdx.x / egroups;
  const int lane = threadIdx.x % kSlabLanes, grp = threadIdx.x / kSlabLanes;
  const int e = (int)(blockIdx.x % egroups) * kSlabLanes + lane;
  __shared__ float red[kSlabGroups][kSlabLanes];
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (e < E) {
    const int p0 = (int)((int64_t)nparts * grp / kSlabGroups), p1 = (int)((int64_t)nparts * (grp + 1) / kSlabGroups);
    for (int p = p0; p < p1; p += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = p + q < p1 ? map.row(d, p + q, nparts) : -1;
        if (r >= 0) s[q] += slab[r * E + e];
      }
    }
  }
  red[grp][lane] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (grp == 0 && e < E) {
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kSlabGroups; ++k) sum += red[k][lane];
    out[map.dst(d) * E + e] = sum;
  }
}

template <typename Map>
static void slab_reduce(const float* slab, float* out, int64_t D, int nparts, int E, Map map, hipStream_t st) {
  const int egroups = (E + kSlabLanes - 1) / kSlabLanes;
  hipLaunchKernelGGL(slab_reduce_kernel<Map>, dim3((unsigned)(D * egroups)), dim3(kBlock), 0, st, slab, out, nparts, E,
                     egroups, map);
}

// ---- splats ------------------------------------------------------------------------------------------------------
constexpr int kSplatMaxLog = 32;  // a texel may receive at most 2^32 contributions

inline int splat_count_log(int64_t count) {  // ceil(log2(count)), count >= 1
  int c = 0;
  while (c < 63 && ((int64_t)1 << c) < count) ++c;
  return c;
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
constexpr unsigned kInfBits = 0x7f800000u;

// k of the header comment from the bit pattern of the plane's maximum (finite, non-zero)
__device__ __forceinline__ int splat_shift(unsigned max_bits, int clog) {
  int ex;
  (void)frexpf(__uint_as_float(max_bits), &ex);  // maximum = f * 2^ex, 0.5 <= f < 1
  return 63 - ex - clog;
}

// contribution -> integer: the scaling is exact (a power of two; < 2^63 by the choice of k), one rounding to integer
__device__ __forceinline__ unsigned long long splat_term(float c, int k) {
  return (unsigned long long)(long long)rintf(ldexpf(c, k));
}

__device__ __forceinline__ void plane_max_update(unsigned* slot, unsigned bits) {
  // wave maximum first: one atomic per wave
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, d));
  if ((threadIdx.x & (kWave - 1)) == 0 && bits != 0u) atomicMax(slot, bits);
}

// the last pass: out[plane][i] = sum[plane][i] * 2^-k, one rounding (int64 -> fp32; the power of two is exact unless
// the result is denormal)
static __global__ __launch_bounds__(kBlock) void splat_convert_kernel(const unsigned long long* __restrict__ acc,
                                                                      const unsigned* __restrict__ plane_max,
                                                                      float* __restrict__ out, int64_t plane_elems,
                                                                      int64_t total, int clog) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const unsigned mb = plane_max[i / plane_elems];
  float v = 0.0f;
  if (mb >= kInfBits) v = __uint_as_float(0x7fc00000u);
  else if (mb != 0u) v = ldexpf((float)(long long)acc[i], -splat_shift(mb, clog));
  out[i] = v;
}

}  // namespace waldo
