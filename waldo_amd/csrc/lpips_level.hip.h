// LPIPS level distance (include/waldo_hip.h "LPIPS level distance"): the kernels and the host checks that the fp32 entry
// points (lpips_level.hip) and the 16-bit ones (lpips_level_16.hip) share.  The tail of LPIPS at one feature level --
// lpips.normalize_tensor of both maps (eps added AFTER the square root), the squared difference, the bias-free 1 x 1 "lin"
// convolution to one channel and spatial_average -- as one pass structure over the two maps of element type T (float,
// __bf16, _Float16); w, the partials, `saved`, grad_out and ALL ARITHMETIC are fp32 whatever T is:
//   lpips_level_fwd_kernel  a workgroup owns a tile of 64 pixels of ONE image.  Lanes run along pixels (unit stride, ONE
//                           ELEMENT each: no alignment of P or of a pointer beyond sizeof(T) matters), the four waves
//                           share the channels (wave k takes c = k, k + 4, ...; a channel step strides by P).  Walk 1
//                           sums the squares, the waves' sums meet in LDS, every lane has 1 / (n + eps) of its pixel;
//                           walk 2 sums w[c] e[c]^2 and the projection w[c] e[c] f0[c], e = f0 / m0 - f1 / m1 IN THIS
//                           FORM (the expanded A / m0^2 - 2 B / (m0 m1) + Cc / m1^2 cancels where the maps are close;
//                           this one gives exact zeros for equal maps).  The tile's partial goes to the workspace, three
//                           floats per pixel (1 / m0, 1 / m1 and S / (n0 m0^2)) to `saved` when the caller wants a
//                           backward; a finishing launch adds each image's partials in a fixed order and divides by P.
//                           NO ATOMICS: the same bits from run to run.
//   lpips_level_bwd_kernel  one launch, elementwise given `saved`: 2 g (w[c] e[c] / m0 - f0[c] q) in fp32, rounded ONCE to
//                           T (nearest-even; fp16 keeps its subnormals), EXACT 0 on every channel of a pixel whose n0 is 0
//                           (saved 1 / m0 = 0 marks it).
// A tile of 256 pixels (four per lane, 16-byte pieces where the alignment allowed) was built and measured too for fp32:
// never faster beyond the spread, twice as slow at the deep levels and 1.3 to 1.4 x as slow at 2 x 64 x 512 x 1024
// (DESIGN 4q).  The 16-bit maps keep the one-element-per-lane form alone: two pixels per lane as one dword would need
// (c P + p) even and a 4-byte-aligned base, which fails on every odd channel of an odd P (DESIGN 4q "16 bits").
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

namespace {

constexpr int kLpWaves = kBlock / kWave;
constexpr int kLpTile = kWave;                  // pixels of a tile: one per lane
constexpr int kLpBwdChunk = 64;                 // channels of one backward workgroup at a time
constexpr int kLpBwdGridY = 64;                 // at most this many chunks side by side: C > 4096 strides over the rest
constexpr int64_t kLpMaxElems = 2147483647;     // offsets inside an image are 32-bit

template <typename T>
struct LpipsArgs {
  const T* f0;
  const T* f1;
  const float* w;
  float* partial;         // fwd: one float per workgroup
  float* saved;           // (N, 3, P): 1 / m0 (0 where n0 == 0), 1 / m1, S / (n0 m0^2); fwd: NULL = not wanted
  const float* grad_out;  // bwd: (N,)
  T* grad_f0;
  uint32_t C, P, tiles;   // tiles per image
  float eps;
};

// the four waves' values of a lane's pixel, added in wave order (every wave reads the same sums)
__device__ __forceinline__ float lp_across_waves(const float (&red)[kLpWaves][2][kWave], int which, int lane) {
  return ((red[0][which][lane] + red[1][which][lane]) + red[2][which][lane]) + red[3][which][lane];
}

// A lane's element of channel c in the forward's walks, 0 for a lane past the end of the plane.  fp32: the lane loads
// nothing there.  16-bit: the load is UNCONDITIONAL at the clamped pixel pc = min(p, P - 1) (in bounds: c P + pc < C P)
// and the value dropped afterwards -- under the lane's branch the compiler keeps the widening beside its load and waits
// for every 2-byte load on its own, which measured 1.4 to 2.4 x the fp32 kernel's time on half its bytes.
template <typename T>
__device__ __forceinline__ float lp_ld(const T* __restrict__ f, uint32_t row, uint32_t p, uint32_t pc, bool inside) {
  if constexpr (sizeof(T) == sizeof(float)) {
    return inside ? (float)f[row + p] : 0.0f;
  } else {
    const float v = (float)f[row + pc];  // (widening is exact)
    return inside ? v : 0.0f;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void lpips_level_fwd_kernel(LpipsArgs<T> A) {
  __shared__ float red1[kLpWaves][2][kWave];  // the squares of f0, f1
  __shared__ float red2[kLpWaves][2][kWave];  // the distance, the projection
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint32_t n = blockIdx.x / A.tiles, tile = blockIdx.x - n * A.tiles;
  const uint32_t C = A.C, P = A.P;
  const uint32_t p = tile * (uint32_t)kLpTile + lane;
  const bool inside = p < P;  // (a lane past the end of the plane takes no part in any product)
  const uint32_t pc = inside ? p : P - 1;
  const int64_t image = (int64_t)n * ((int64_t)C * P);
  const T* __restrict__ f0 = A.f0 + image;
  const T* __restrict__ f1 = A.f1 + image;
  const float* __restrict__ w = A.w;

  float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 4
  for (uint32_t c = wave; c < C; c += kLpWaves) {
    const float a = lp_ld(f0, c * P, p, pc, inside);  // (c P + p < C P <= 2^31 - 1)
    const float b = lp_ld(f1, c * P, p, pc, inside);
    s0 += a * a;
    s1 += b * b;
  }
  red1[wave][0][lane] = s0;
  red1[wave][1][lane] = s1;
  __syncthreads();
  const float n0 = sqrtf(lp_across_waves(red1, 0, lane));
  const float m0 = n0 + A.eps;
  // (outside: with eps == 0 the lane's 0 * (1 / 0) would be NaN)
  const float r0 = inside ? 1.0f / m0 : 0.0f;
  const float r1 = inside ? 1.0f / (sqrtf(lp_across_waves(red1, 1, lane)) + A.eps) : 0.0f;

  float d = 0.0f, proj = 0.0f;
#pragma unroll 4
  for (uint32_t c = wave; c < C; c += kLpWaves) {
    const float a = lp_ld(f0, c * P, p, pc, inside);
    const float b = lp_ld(f1, c * P, p, pc, inside);
    const float e = a * r0 - b * r1;
    const float we = w[c] * e;
    d += we * e;
    proj += we * a;
  }
  red2[wave][0][lane] = d;
  red2[wave][1][lane] = proj;
  __syncthreads();
  if (wave != 0) return;
  d = lp_across_waves(red2, 0, lane);
  if (A.saved != nullptr && inside) {
    proj = lp_across_waves(red2, 1, lane);
    const bool zero = n0 == 0.0f;
    float* __restrict__ sv = A.saved + (int64_t)n * (3 * (int64_t)P) + p;
    sv[0] = zero ? 0.0f : r0;
    sv[P] = r1;
    sv[2 * (int64_t)P] = zero ? 0.0f : proj / (n0 * (m0 * m0));
  }
  d = wave_sum(d);
  if (lane == 0) A.partial[blockIdx.x] = d;
}

// out[n] = (the partials of image n, in a fixed order) / P
template <typename T>
__global__ __launch_bounds__(kBlock) void lpips_level_finish_kernel(LpipsArgs<T> A, float* __restrict__ out) {
  __shared__ float red[kLpWaves];
  const float* __restrict__ part = A.partial + (int64_t)blockIdx.x * A.tiles;
  float acc = 0.0f;
  for (uint32_t t = threadIdx.x; t < A.tiles; t += kBlock) acc += part[t];
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) / (float)A.P;
}

// blockIdx.x: (image, tile) as in the forward; blockIdx.y, striding by gridDim.y (at most kLpBwdGridY): chunks of kLpBwdChunk
// channels, each shared by the four waves
template <typename T>
__global__ __launch_bounds__(kBlock) void lpips_level_bwd_kernel(LpipsArgs<T> A) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint32_t n = blockIdx.x / A.tiles, tile = blockIdx.x - n * A.tiles;
  const uint32_t C = A.C, P = A.P;
  const uint32_t p = tile * (uint32_t)kLpTile + lane;
  if (p >= P) return;
  const int64_t image = (int64_t)n * ((int64_t)C * P);
  const T* __restrict__ f0 = A.f0 + image;
  const T* __restrict__ f1 = A.f1 + image;
  T* __restrict__ grad = A.grad_f0 + image;
  const float* __restrict__ w = A.w;
  const float* __restrict__ sv = A.saved + (int64_t)n * (3 * (int64_t)P) + p;
  const float r0 = sv[0], r1 = sv[P], q = sv[2 * (int64_t)P];
  const float g2 = 2.0f * (A.grad_out[n] / (float)P);
  for (uint32_t c0 = blockIdx.y * (uint32_t)kLpBwdChunk; c0 < C; c0 += gridDim.y * (uint32_t)kLpBwdChunk) {
    const uint32_t c1 = min(c0 + (uint32_t)kLpBwdChunk, C);  // (c0 < C <= 2^31 - 1 and a step of 2^12: no wrap)
#pragma unroll 4
    for (uint32_t c = c0 + wave; c < c1; c += kLpWaves) {
      const float a = (float)f0[c * P + p];
      const float e = a * r0 - (float)f1[c * P + p] * r1;
      // (n0 == 0: EXACT 0, whatever g2 is; the conversion to T is the only rounding to T: nearest-even, no flush)
      grad[c * P + p] = (T)(r0 == 0.0f ? 0.0f : g2 * ((w[c] * e) * r0 - a * q));
    }
  }
}

inline bool lp_shape_ok(int64_t N, int64_t C, int64_t P) { return N > 0 && C > 0 && P > 0; }

inline int64_t lp_tiles(int64_t P) { return (P + kLpTile - 1) / kLpTile; }

// (P <= 2^31 - 1 is implied by C P <= 2^31 - 1)
inline bool lp_size_ok(int64_t N, int64_t C, int64_t P) { return C <= kLpMaxElems / P && N <= kLpMaxElems / lp_tiles(P); }

inline int64_t lp_workspace_bytes(int64_t N, int64_t C, int64_t P) {
  if (!lp_shape_ok(N, C, P) || !lp_size_ok(N, C, P)) return 0;
  return (N * lp_tiles(P) * (int64_t)sizeof(float) + 255) / 256 * 256;
}

// the shape's checks; WALDO_EINVAL with the message set, or WALDO_OK with A's sizes filled in
template <typename T>
int lp_grid(const char* fn, int64_t N, int64_t C, int64_t P, LpipsArgs<T>& A) {
  if (!lp_shape_ok(N, C, P)) {
    set_error("%s: bad shape N=%lld C=%lld P=%lld (all > 0)", fn, (long long)N, (long long)C, (long long)P);
    return WALDO_EINVAL;
  }
  if (!lp_size_ok(N, C, P)) {
    set_error("%s: too large: C=%lld x P=%lld elements per image (at most 2^31 - 1), N=%lld x %lld tiles (at most 2^31 - 1)",
              fn, (long long)C, (long long)P, (long long)N, (long long)lp_tiles(P));
    return WALDO_EINVAL;
  }
  A.C = (uint32_t)C;
  A.P = (uint32_t)P;
  A.tiles = (uint32_t)lp_tiles(P);
  return WALDO_OK;
}

// The entry points' bodies after their dtype is known: the checks in the order null pointer, bad shape, too large,
// workspace, then the launches.
template <typename T>
int lp_fwd(const char* fn, const void* f0, const void* f1, const float* w, float* out, float* saved, void* workspace,
           int64_t workspace_bytes, int64_t N, int64_t C, int64_t P, float eps, waldo_stream_t stream) {
  if (!f0 || !f1 || !w || !out || !workspace) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  LpipsArgs<T> A{static_cast<const T*>(f0), static_cast<const T*>(f1), w, static_cast<float*>(workspace), saved, nullptr,
                 nullptr, 0, 0, 0, eps};
  const int rc = lp_grid(fn, N, C, P, A);
  if (rc != WALDO_OK) return rc;
  const int64_t need = lp_workspace_bytes(N, C, P);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)need);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  lpips_level_fwd_kernel<T><<<dim3((uint32_t)(N * A.tiles)), dim3(kBlock), 0, st>>>(A);
  lpips_level_finish_kernel<T><<<dim3((uint32_t)N), dim3(kBlock), 0, st>>>(A, out);
  return launch_status(fn);
}

template <typename T>
int lp_bwd(const char* fn, const void* f0, const void* f1, const float* w, const float* saved, const float* grad_out,
           void* grad_f0, int64_t N, int64_t C, int64_t P, waldo_stream_t stream) {
  if (!f0 || !f1 || !w || !saved || !grad_out || !grad_f0) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  LpipsArgs<T> A{static_cast<const T*>(f0), static_cast<const T*>(f1), w, nullptr, const_cast<float*>(saved), grad_out,
                 static_cast<T*>(grad_f0), 0, 0, 0, 0.0f};
  const int rc = lp_grid(fn, N, C, P, A);
  if (rc != WALDO_OK) return rc;
  int64_t chunks = (C + kLpBwdChunk - 1) / kLpBwdChunk;
  if (chunks > kLpBwdGridY) chunks = kLpBwdGridY;  // (the kernel strides over the rest: no limit on C of its own)
  lpips_level_bwd_kernel<T><<<dim3((uint32_t)(N * A.tiles), (uint32_t)chunks), dim3(kBlock), 0, (hipStream_t)stream>>>(A);
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo
