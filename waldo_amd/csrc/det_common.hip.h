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
#include <cstdarg>
#include <cstdio>

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

// A workgroup's partial table of N entries in LDS, one row per wave, over `__shared__ float s[4][N]`
// of the kernel: every wave zeroes and adds into ITS OWN row (wave_transpose_reduce leaves one lane per entry: plain
// read-modify-write, no atomics, no barrier), and after a barrier the four rows are summed in a fixed order and leave
// the workgroup -- as ONE float atomic per entry into the table's home row of `dest`, or (DET) as a plain store into
// the workgroup's row of the slab `dest`.  occ_composite_bwd_kernel's table; the two flow_ctx backward kernels
// (flow_ctx_bwd.hip) keep the same steps written out (through this type their largest
// instances spill more).
template <int N>
struct WaveTable {
  static_assert(kBlock == 4 * kWave, "four waves, four rows");
  float (*rows)[N];
  __device__ __forceinline__ void zero(int wave, int lane) const {
    for (int e = lane; e < N; e += kWave) rows[wave][e] = 0.0f;
  }
  __device__ __forceinline__ float* row(int wave) const { return rows[wave]; }
  // E: entries of a row of dest; index(e, at): whether entry e of the table goes anywhere (not padding), and where inside
  // that row
  template <bool DET, typename Index>
  __device__ __forceinline__ void flush(float* __restrict__ dest, int E, int64_t home_row, Index&& index) const {
    for (int e = threadIdx.x; e < N; e += kBlock) {
      int at;
      if (index(e, at)) {
        const float sum = (rows[0][e] + rows[1][e]) + (rows[2][e] + rows[3][e]);
        float* out = dest + (DET ? (int64_t)blockIdx.x : home_row) * E;
        if constexpr (DET) out[at] = sum;
        else atomicAdd(out + at, sum);
      }
    }
  }
};

// index() of an L x L matrix kept as an LP x LP table: entry i * LP + j -> i * L + j
template <int LP>
struct PaddedSquare {
  int L;
  __device__ __forceinline__ bool operator()(int e, int& at) const {
    const int i = e / LP, j = e % LP;
    at = i * L + j;
    return i < L && j < L;
  }
};

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

// ---- workspaces (host) ---------------------------------------------------------------------------------------------
// Segments of a workspace in the order given, each rounded up to 256 bytes.  An op builds ONE of these from its shapes;
// its *_workspace_bytes query returns total() and its entry point takes its pointers from at().
template <int N>
struct Carved {
  int64_t off[N + 1];  // off[N]: the total
  int64_t total() const { return off[N]; }
  template <typename T>
  T* at(void* workspace, int i) const { return reinterpret_cast<T*>(static_cast<char*>(workspace) + off[i]); }
};

template <typename... S>
Carved<(int)sizeof...(S)> carve(S... bytes) {
  constexpr int N = (int)sizeof...(S);
  const int64_t size[N] = {(int64_t)bytes...};
  Carved<N> c;
  c.off[0] = 0;
  for (int i = 0; i < N; ++i) c.off[i + 1] = c.off[i] + round256(size[i]);
  return c;
}

// the refusal of a missing or short workspace (a null one counts as 0 bytes)
inline int check_workspace(const char* fn, const void* workspace, int64_t workspace_bytes, int64_t need,
                           const char* note = "") {
  if (workspace != nullptr && workspace_bytes >= need) return WALDO_OK;
  set_error("%s: workspace of %lld bytes given, %lld needed%s", fn, (long long)(workspace == nullptr ? 0 : workspace_bytes),
            (long long)need, note);
  return WALDO_EINVAL;
}

// ---- splats ------------------------------------------------------------------------------------------------------
constexpr int kSplatMaxLog = 32;  // a texel may receive at most 2^32 contributions

// clog of the header comment: ceil(log2(count)) for the largest number of contributions one texel can receive;
// -1: more than 2^32, no deterministic sum
inline int splat_clog(int64_t count) {
  int c = 0;
  while (c < 63 && ((int64_t)1 << c) < count) ++c;
  return c <= kSplatMaxLog ? c : -1;
}

// the refusal that goes with splat_clog() < 0; `grad`: the gradient's name, then the caller's sizes (printf style)
__attribute__((format(printf, 3, 4))) inline int splat_refuse(const char* fn, const char* grad, const char* sizes, ...) {
  char text[160];
  va_list ap;
  va_start(ap, sizes);
  vsnprintf(text, sizeof(text), sizes, ap);
  va_end(ap);
  set_error("%s: a texel of %s may receive more than 2^%d contributions (%s): no deterministic sum for this shape", fn,
            grad, kSplatMaxLog, text);
  return WALDO_EINVAL;
}

// grids of the maximum pass (the caller's workgroups) and of the conversion (one thread per texel of the gradient)
inline int check_splat_launches(const char* fn, int64_t max_blocks, int64_t texels) {
  if (max_blocks > 2147483647 || (texels + kBlock - 1) / kBlock > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
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

// The passes of one splat, in stream order: zero fill, the caller's maximum pass, the caller's splat pass, and the
// conversion that overwrites out (planes x plane_elems).  Segments i (the 64-bit sums, 8 bytes per texel) and i + 1 (the
// maxima, 4 bytes per plane) of the op's workspace are adjacent: one fill zeroes both.  `live` false: nothing
// contributes (no source maps), out = 0.  An op whose stream order puts launches of its own between these passes hands
// them over as `before_max` (after the fill) and `after_splat` (before the conversion); they run when `live`, too.
struct NoLaunch {
  void operator()() const {}
};
template <int N, typename MaxPass, typename SplatPass, typename Before = NoLaunch, typename After = NoLaunch>
void splat_passes(const Carved<N>& lo, void* workspace, int i, float* out, int64_t planes, int64_t plane_elems, int clog,
                  bool live, hipStream_t st, MaxPass&& max_pass, SplatPass&& splat_pass, Before&& before_max = Before{},
                  After&& after_splat = After{}) {
  unsigned long long* acc = lo.template at<unsigned long long>(workspace, i);
  unsigned* plane_max = lo.template at<unsigned>(workspace, i + 1);
  fill_words(acc, 0u, (size_t)(lo.off[i + 2] - lo.off[i]), st);
  if (live) {
    before_max();
    max_pass(plane_max);
    splat_pass(acc, plane_max);
    after_splat();
  }
  const int64_t total = planes * plane_elems;
  hipLaunchKernelGGL(splat_convert_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, acc,
                     plane_max, out, plane_elems, total, clog);
}

}  // namespace waldo
