// Supervision targets (include/waldo_hip.h "Supervision targets"): the data-side target of LVD training and its
// control-point distance terms -- the reference's Synthesizer.extract_object (models/synthesizer.py:907-945, 965-979).
//   waldo_flow_edges_fwd      EdgeExtractor.forward (models/modules/edge.py:28-40): one launch; a 16 x 64 tile with its
//                             k/2 halo per channel in LDS (18.7 KB at k = 15, C = 2), the k x k weights in the kernel's
//                             arguments (uniform index: scalar loads).  A lane owns 4 pixels of a column and slides a
//                             4-row register window down the taps: one LDS read per 12 multiply-adds.
//   waldo_gaussian_blur_fwd   torchvision's GaussianBlur with a fixed sigma: one launch; the 32 x 64 tile with its halo in
//                             LDS, the row pass into a second LDS buffer, the column pass out of it -- no intermediate
//                             in HBM.
//   waldo_mov_props_fwd       the sums over layout channels, read once, and the blur's input;
//   waldo_mov_finish_fwd      thresholds, masks and the masked overwrites, one pass;
//   waldo_cell_distance_*     min over objects of the weighted cell distance from the objects' moments, its mean and the
//                             two gradients.  NO FLOAT ATOMICS anywhere: a partial per workgroup in the workspace, then one
//                             pass over the partials in a fixed order -- the same bits from run to run.
// Streaming kernels: one lane per pixel, coalesced rows.  No allocation, no synchronisation; the caller's stream.
#include <math.h>

#include "waldo_common.hip.h"

namespace waldo {

namespace {

__device__ __forceinline__ int reflect_clamped(int i, int n) {
  // reflection without the border pixel (ReflectionPad2d); the clamp only serves the rows / columns of a partial tile
  // beyond the image's halo, whose values no output reads
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// block sum in a fixed order: lanes by wave_sum's butterfly, then the four waves in order; valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red4) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red4[threadIdx.x / kWave] = v;
  __syncthreads();
  return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// flow edges
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kEdgeMaxK = 15, kEdgeTH = 16, kEdgeTW = 64, kEdgeMaxC = 2, kEdgePx = 4;
constexpr int kEdgeTile = (kEdgeTH + kEdgeMaxK - 1) * (kEdgeTW + kEdgeMaxK - 1);
static_assert(kEdgeTW == kWave && kEdgeTH == kEdgePx * (kBlock / kWave), "a wave per 4 rows of the tile");

struct EdgeWeights {
  float wx[kEdgeMaxK * kEdgeMaxK];  // wx[d * k + j] = x_d / (x_d^2 + y_j^2); the other filter is its transpose
  float mean;                       // 1 / k^2
  float max_edge;                   // sqrt(32)
};

__global__ __launch_bounds__(kBlock) void flow_edges_kernel(const float* __restrict__ flow, float* __restrict__ edge,
                                                            float* __restrict__ dominant, int C, int H, int W, int k,
                                                            float eps, int tiles_x, int tiles_y, EdgeWeights wt) {
  __shared__ float tile[kEdgeMaxC][kEdgeTile];
  const int p = k >> 1;
  const int pitch = kEdgeTW + 2 * p, rows = kEdgeTH + 2 * p;
  const unsigned tx = blockIdx.x % (unsigned)tiles_x, rest = blockIdx.x / (unsigned)tiles_x;
  const unsigned ty = rest % (unsigned)tiles_y;
  const int64_t n = rest / (unsigned)tiles_y;
  const int x0 = (int)tx * kEdgeTW, y0 = (int)ty * kEdgeTH;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ src = flow + n * C * HW;
  for (int c = 0; c < C; ++c)
    for (int i = threadIdx.x; i < rows * pitch; i += kBlock) {
      const int ry = i / pitch, rx = i - ry * pitch;
      tile[c][i] = src[c * HW + (int64_t)reflect_clamped(y0 - p + ry, H) * W + reflect_clamped(x0 - p + rx, W)];
    }
  __syncthreads();
  const int lx = threadIdx.x & (kWave - 1), ly0 = (threadIdx.x / kWave) * kEdgePx;
  float keep[kEdgePx], flow_norm[kEdgePx], mean_norm[kEdgePx];
#pragma unroll
  for (int q = 0; q < kEdgePx; ++q) {
    keep[q] = 1.0f;
    flow_norm[q] = 0.0f;
    mean_norm[q] = 0.0f;
  }
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ t = tile[c] + ly0 * pitch + lx;
    float s[kEdgePx], gx[kEdgePx], gy[kEdgePx];
#pragma unroll
    for (int q = 0; q < kEdgePx; ++q) s[q] = gx[q] = gy[q] = 0.0f;
    for (int j = 0; j < k; ++j) {
      float v[kEdgePx];  // rows d .. d + 3 of column j: the tap (d, j) of the lane's four pixels
#pragma unroll
      for (int q = 0; q < kEdgePx - 1; ++q) v[q + 1] = t[q * pitch + j];
      for (int d = 0; d < k; ++d) {
#pragma unroll
        for (int q = 0; q < kEdgePx - 1; ++q) v[q] = v[q + 1];
        v[kEdgePx - 1] = t[(d + kEdgePx - 1) * pitch + j];
        const float wx = wt.wx[d * k + j], wy = wt.wx[j * k + d];
#pragma unroll
        for (int q = 0; q < kEdgePx; ++q) {
          s[q] += v[q];
          gx[q] = fmaf(wx, v[q], gx[q]);
          gy[q] = fmaf(wy, v[q], gy[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kEdgePx; ++q) {
      const float own = t[(q + p) * pitch + p], mean = s[q] * wt.mean;
      flow_norm[q] += own * own;
      mean_norm[q] += mean * mean;
      const float e = sqrtf(gx[q] * gx[q] + gy[q] * gy[q] + eps) / wt.max_edge;
      keep[q] *= 1.0f - e;
    }
  }
  const int x = x0 + lx;
#pragma unroll
  for (int q = 0; q < kEdgePx; ++q) {
    const int y = y0 + ly0 + q;
    if (x < W && y < H) {
      const int64_t o = n * HW + (int64_t)y * W + x;
      edge[o] = 1.0f - keep[q];
      dominant[o] = flow_norm[q] > mean_norm[q] ? 1.0f : 0.0f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian blur
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kBlurMaxK = 31, kBlurTH = 32, kBlurTW = 64;
constexpr int kBlurIn = (kBlurTH + kBlurMaxK - 1) * (kBlurTW + kBlurMaxK - 1);
constexpr int kBlurMid = (kBlurTH + kBlurMaxK - 1) * kBlurTW;

struct BlurWeights {
  float w[kBlurMaxK];
};

__global__ __launch_bounds__(kBlock) void gaussian_blur_kernel(const float* __restrict__ x, float* __restrict__ y, int H,
                                                               int W, int k, int tiles_x, int tiles_y, BlurWeights wt) {
  __shared__ float in[kBlurIn];
  __shared__ float mid[kBlurMid];
  const int p = k >> 1;
  const int pitch = kBlurTW + 2 * p, rows = kBlurTH + 2 * p;
  const unsigned tx = blockIdx.x % (unsigned)tiles_x, rest = blockIdx.x / (unsigned)tiles_x;
  const unsigned ty = rest % (unsigned)tiles_y;
  const int64_t plane = rest / (unsigned)tiles_y;
  const int x0 = (int)tx * kBlurTW, y0 = (int)ty * kBlurTH;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ src = x + plane * HW;
  for (int i = threadIdx.x; i < rows * pitch; i += kBlock) {
    const int ry = i / pitch, rx = i - ry * pitch;
    in[i] = src[(int64_t)reflect_clamped(y0 - p + ry, H) * W + reflect_clamped(x0 - p + rx, W)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * kBlurTW; i += kBlock) {  // rows
    const float* __restrict__ r = in + (i / kBlurTW) * pitch + (i % kBlurTW);
    float acc = 0.0f;
    for (int j = 0; j < k; ++j) acc = fmaf(wt.w[j], r[j], acc);
    mid[i] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBlurTH * kBlurTW; i += kBlock) {  // columns
    const int ly = i / kBlurTW, lx = i % kBlurTW;
    float acc = 0.0f;
    for (int d = 0; d < k; ++d) acc = fmaf(wt.w[d], mid[(ly + d) * kBlurTW + lx], acc);
    if (x0 + lx < W && y0 + ly < H) y[plane * HW + (int64_t)(y0 + ly) * W + x0 + lx] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// moving-object target
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mov_props_kernel(const float* __restrict__ lyt, const float* __restrict__ flow,
                                                           unsigned fg_bits, unsigned bg_bits, unsigned other_bits,
                                                           float* __restrict__ fg_prop, float* __restrict__ nobg_prop,
                                                           float* __restrict__ other_prop, float* __restrict__ blur_in,
                                                           int Nl, int64_t HW, int chunks) {
  const int64_t n = blockIdx.x / (unsigned)chunks;
  const int64_t i = (int64_t)(blockIdx.x % (unsigned)chunks) * kBlock + threadIdx.x;
  if (i >= HW) return;
  const float* __restrict__ l = lyt + n * Nl * HW + i;
  const unsigned any = fg_bits | bg_bits | other_bits;
  float fg = 0.0f, bg = 0.0f, other = 0.0f;
  for (int c = 0; c < Nl; ++c) {
    const unsigned bit = 1u << c;
    if (!(any & bit)) continue;
    const float v = l[c * HW] / 10.0f + 0.5f;
    if (fg_bits & bit) fg += v;
    if (bg_bits & bit) bg += v;
    if (other_bits & bit) other += v;
  }
  const float nofg = 1.0f - fg;
  fg_prop[n * HW + i] = fg;
  nobg_prop[n * HW + i] = 1.0f - bg;
  other_prop[n * HW + i] = other;
  blur_in[(n * 3 + 0) * HW + i] = nofg;
  blur_in[(n * 3 + 1) * HW + i] = nofg * flow[(n * 2 + 0) * HW + i];
  blur_in[(n * 3 + 2) * HW + i] = nofg * flow[(n * 2 + 1) * HW + i];
}

struct FinishArgs {
  const float *flow, *blurred, *fg_prop, *nobg_prop, *other_prop, *edge_raw, *dominant;
  float *edge, *mean_bg_flow, *mask, *mov_obj;
  float flow_thresh, mov_obj_thresh, reg_bg_mul, nobg_edge_mul;
  int flags, chunks;
  int64_t HW;
};

__global__ __launch_bounds__(kBlock) void mov_finish_kernel(FinishArgs A) {
  const int64_t n = blockIdx.x / (unsigned)A.chunks, HW = A.HW;
  const int64_t i = (int64_t)(blockIdx.x % (unsigned)A.chunks) * kBlock + threadIdx.x;
  if (i >= HW) return;
  const int64_t o = n * HW + i;
  const float edge = A.edge_raw[o] > A.flow_thresh ? 1.0f : 0.0f;
  const float b0 = A.blurred[(n * 3 + 0) * HW + i];
  const float sum = b0 + (b0 == 0.0f ? 1.0f : 0.0f);
  const float m0 = A.blurred[(n * 3 + 1) * HW + i] / sum, m1 = A.blurred[(n * 3 + 2) * HW + i] / sum;
  const float fg = A.fg_prop[o], nobg = A.nobg_prop[o];
  const float delta = fg * (fabsf(A.flow[(n * 2 + 0) * HW + i] - m0) + fabsf(A.flow[(n * 2 + 1) * HW + i] - m1));
  float mask = delta > A.mov_obj_thresh ? 1.0f : 0.0f;
  if (A.flags & WALDO_MOV_DOMINANT_OTHER) {  // torch.max: a NaN on either side wins
    const float cand = A.other_prop[o] * A.dominant[o] * edge;
    mask = (cand > mask || cand != cand) ? cand : mask;
  }
  if ((A.flags & WALDO_MOV_FLOW_NOBG) && edge > 0.1f && nobg > 0.0f) mask = 1.0f;
  float mov = mask * 2.0f - 1.0f;
  if (mov < 0.0f) mov *= A.reg_bg_mul;
  if ((A.flags & WALDO_MOV_USE_FG) && mov < 0.0f && fg > 0.0f) mov = 0.0f;
  if ((A.flags & WALDO_MOV_USE_NOBG) && mov < 0.0f && nobg > 0.0f) mov = 0.0f;
  if ((A.flags & WALDO_MOV_USE_NOBG_EDGE) && mov < 0.0f && nobg > 0.0f && edge > 0.1f) mov = A.nobg_edge_mul;
  A.edge[o] = edge;
  A.mean_bg_flow[(n * 2 + 0) * HW + i] = m0;
  A.mean_bg_flow[(n * 2 + 1) * HW + i] = m1;
  A.mask[o] = mask;
  A.mov_obj[o] = mov;
}

// ---------------------------------------------------------------------------------------------------------------------
// cell distance
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kCellMaxObj = 31, kCellPx = 8, kCellChunk = kCellPx * kBlock;  // pixels of a workgroup

inline int64_t cell_chunks(int64_t HW) { return (HW + kCellChunk - 1) / kCellChunk; }

// sum_k |g - c_k|^2 from the moments, the ONE definition the forward and the backward share (the same bits)
__device__ __forceinline__ float cell_dis(float px, float py, float kg2, const float* mom) {
  return (kg2 - 2.0f * (px * mom[0] + py * mom[1])) + mom[2];
}

struct CellArgs {
  const float *moments, *mov_mask, *fg_mask, *gx, *gy, *grad_out;
  float* partial;
  uint8_t* chosen;
  float* grad_fg;
  int No, H, W, chunks;
  float K, eps, count;
};

struct CellPixel {
  float w, px, py, kg2;
  bool in;
};

template <bool HAS_FG>
__device__ __forceinline__ CellPixel cell_pixel(const CellArgs& A, int64_t f, int64_t i, int64_t HW) {
  CellPixel P;
  P.in = i < HW;
  P.w = P.px = P.py = P.kg2 = 0.0f;
  if (P.in) {
    const int y = (int)(i / A.W), x = (int)(i - (int64_t)y * A.W);
    P.px = A.gx[x];
    P.py = A.gy[y];
    P.kg2 = A.K * (P.px * P.px + P.py * P.py);
    const float m = A.mov_mask[f * HW + i];
    P.w = HAS_FG ? (m + A.eps) * (1.0f - A.fg_mask[f * HW + i]) : m;
  }
  return P;
}

template <bool HAS_FG>
__global__ __launch_bounds__(kBlock) void cell_distance_fwd_kernel(CellArgs A) {
  __shared__ float mom[kCellMaxObj * 3];
  __shared__ float red[kBlock / kWave];
  const int64_t f = blockIdx.x / (unsigned)A.chunks, HW = (int64_t)A.H * A.W;
  const int64_t base = (int64_t)(blockIdx.x % (unsigned)A.chunks) * kCellChunk;
  if ((int)threadIdx.x < A.No * 3) mom[threadIdx.x] = A.moments[f * A.No * 3 + threadIdx.x];
  __syncthreads();
  float acc = 0.0f;
#pragma unroll
  for (int it = 0; it < kCellPx; ++it) {
    const int64_t i = base + it * kBlock + threadIdx.x;
    const CellPixel P = cell_pixel<HAS_FG>(A, f, i, HW);
    if (!P.in) continue;
    float best = P.w * cell_dis(P.px, P.py, P.kg2, mom);
    int id = 0;
    for (int n = 1; n < A.No; ++n) {  // torch.min's index on the CPU: the lowest n among the minima, the first NaN kept
      const float v = P.w * cell_dis(P.px, P.py, P.kg2, mom + 3 * n);
      if (v < best || (v != v && best == best)) {
        best = v;
        id = n;
      }
    }
    A.chosen[f * HW + i] = (uint8_t)id;
    acc += best;
  }
  const float total = block_sum(acc, red);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = total;
}

// out[0] = (sum of n partials, in a fixed order) / count
__global__ __launch_bounds__(kBlock) void cell_mean_kernel(const float* __restrict__ partial, int64_t n, float count,
                                                           float* __restrict__ out) {
  __shared__ float red[kBlock / kWave];
  float acc = 0.0f;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) acc += partial[i];
  const float total = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = total / count;
}

// per workgroup and object: the sums of (-2 w gx, -2 w gy, w) over its pixels that chose the object -> partial; grad_fg
template <bool HAS_FG>
__global__ __launch_bounds__(kBlock) void cell_distance_bwd_kernel(CellArgs A) {
  __shared__ float mom[kCellMaxObj * 3];
  __shared__ float red[kCellMaxObj * 3][kBlock / kWave];
  const int64_t f = blockIdx.x / (unsigned)A.chunks, HW = (int64_t)A.H * A.W;
  const int64_t base = (int64_t)(blockIdx.x % (unsigned)A.chunks) * kCellChunk;
  if ((int)threadIdx.x < A.No * 3) mom[threadIdx.x] = A.moments[f * A.No * 3 + threadIdx.x];
  __syncthreads();
  const float scale = A.grad_out[0] / A.count;
  float w[kCellPx], px[kCellPx], py[kCellPx];
  int id[kCellPx];
#pragma unroll
  for (int it = 0; it < kCellPx; ++it) {
    const int64_t i = base + it * kBlock + threadIdx.x;
    const CellPixel P = cell_pixel<HAS_FG>(A, f, i, HW);
    w[it] = P.w;
    px[it] = P.px;
    py[it] = P.py;
    id[it] = P.in ? (int)A.chosen[f * HW + i] : 255;
    if (HAS_FG && P.in && A.grad_fg != nullptr) {
      const int n = min(id[it], A.No - 1);  // (a byte the forward did not write cannot index beyond the moments)
      const float m_eps = A.mov_mask[f * HW + i] + A.eps;
      A.grad_fg[f * HW + i] = -(scale * (m_eps * cell_dis(P.px, P.py, P.kg2, mom + 3 * n)));
    }
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int n = 0; n < A.No; ++n) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int it = 0; it < kCellPx; ++it)
      if (id[it] == n) {
        s0 += -2.0f * (w[it] * px[it]);
        s1 += -2.0f * (w[it] * py[it]);
        s2 += w[it];
      }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
      red[3 * n + 0][wave] = s0;
      red[3 * n + 1][wave] = s1;
      red[3 * n + 2][wave] = s2;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < A.No * 3) {
    const float* r = red[threadIdx.x];
    A.partial[(int64_t)blockIdx.x * A.No * 3 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// grad_moments[f][j] = scale * (the chunks' partials of (f, j), in order); j over No * 3
__global__ __launch_bounds__(kBlock) void cell_moments_grad_kernel(const float* __restrict__ partial,
                                                                   const float* __restrict__ grad_out, float count,
                                                                   float* __restrict__ grad_moments, int64_t total,
                                                                   int per_frame, int chunks) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t f = i / per_frame;
  const int j = (int)(i - f * per_frame);
  float acc = 0.0f;
  for (int c = 0; c < chunks; ++c) acc += partial[(f * chunks + c) * per_frame + j];
  grad_moments[i] = (grad_out[0] / count) * acc;
}

bool finite(float v) { return v >= -3.4028234664e38f && v <= 3.4028234664e38f; }

bool odd_kernel(const char* fn, int k, int max_k, int H, int W) {
  if (k < 3 || k > max_k || k % 2 == 0) {
    set_error("%s: kernel size %d (odd, 3 .. %d)", fn, k, max_k);
    return false;
  }
  if (H <= k / 2 || W <= k / 2 || H > 32768 || W > 32768) {
    set_error("%s: bad shape H=%d W=%d for kernel size %d (reflection padding: k/2 < H, W <= 32768)", fn, H, W, k);
    return false;
  }
  return true;
}

// tiles_x * tiles_y * N workgroups as one grid dimension
bool grid_of(const char* fn, int64_t a, int64_t b, int64_t c, unsigned& grid) {
  if (a <= 0 || b <= 0 || c <= 0 || a > 2147483647 / b || a * b > 2147483647 / c) {
    set_error("%s: problem too large for one launch", fn);
    return false;
  }
  grid = (unsigned)(a * b * c);
  return true;
}

int cell_check(const char* fn, const void* moments, const void* mov_mask, const void* gx, const void* gy,
               const void* workspace, int64_t workspace_bytes, int64_t F, int No, int H, int W, float K, float eps,
               unsigned& grid) {
  if (No < 1 || No > kCellMaxObj) {
    set_error("%s: No=%d objects (1 .. %d: the chosen object is a byte, 255 marks no pixel)", fn, No, kCellMaxObj);
    return WALDO_EINVAL;
  }
  if (F < 0 || H < 1 || W < 1 || H > 32768 || W > 32768) {
    set_error("%s: bad shape F=%lld H=%d W=%d", fn, (long long)F, H, W);
    return WALDO_EINVAL;
  }
  if (!finite(K) || !(K > 0.0f) || !finite(eps)) {
    set_error("%s: bad K=%g (points per object, > 0) or eps=%g", fn, (double)K, (double)eps);
    return WALDO_EINVAL;
  }
  if (F == 0) return 1;
  if (!moments || !mov_mask || !gx || !gy || !workspace) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!grid_of(fn, F, cell_chunks((int64_t)H * W), 1, grid)) return WALDO_EINVAL;
  const int64_t need = waldo_cell_distance_workspace_bytes(F, No, (int64_t)H * W);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)need);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_flow_edges_fwd(const float* flow, float* flow_edge, float* dominant, int64_t N, int C, int H, int W,
                                    int k, float eps, waldo_stream_t stream) {
  const char* fn = "waldo_flow_edges_fwd";
  if (!odd_kernel(fn, k, kEdgeMaxK, H, W)) return WALDO_EINVAL;
  if (N < 0 || C < 1 || C > kEdgeMaxC || !finite(eps) || eps < 0.0f) {
    set_error("%s: bad arguments N=%lld C=%d (1 .. %d channels) eps=%g (>= 0)", fn, (long long)N, C, kEdgeMaxC,
              (double)eps);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!flow || !flow_edge || !dominant) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const int tiles_x = (W + kEdgeTW - 1) / kEdgeTW, tiles_y = (H + kEdgeTH - 1) / kEdgeTH;
  unsigned grid;
  if (!grid_of(fn, tiles_x, tiles_y, N, grid)) return WALDO_EINVAL;
  EdgeWeights wt{};
  for (int d = 0; d < k; ++d)  // edge.py:20-24: integer coordinates and their integer sum, then ONE fp32 division
    for (int j = 0; j < k; ++j) {
      const int xd = d - k / 2, yj = j - k / 2, sum = xd * xd + yj * yj;
      wt.wx[d * k + j] = (float)xd / (float)(sum == 0 ? 1 : sum);
    }
  wt.mean = 1.0f / (float)(k * k);
  wt.max_edge = (float)sqrt(32.0);
  flow_edges_kernel<<<dim3(grid), dim3(kBlock), 0, (hipStream_t)stream>>>(flow, flow_edge, dominant, C, H, W, k, eps,
                                                                         tiles_x, tiles_y, wt);
  return launch_status(fn);
}

extern "C" int waldo_gaussian_blur_fwd(const float* x, float* y, int64_t P, int H, int W, int k, float sigma,
                                       waldo_stream_t stream) {
  const char* fn = "waldo_gaussian_blur_fwd";
  if (!odd_kernel(fn, k, kBlurMaxK, H, W)) return WALDO_EINVAL;
  if (P < 0 || !finite(sigma) || !(sigma > 0.0f)) {
    set_error("%s: bad arguments P=%lld sigma=%g (> 0)", fn, (long long)P, (double)sigma);
    return WALDO_EINVAL;
  }
  if (P == 0) return WALDO_OK;
  if (!x || !y) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const int tiles_x = (W + kBlurTW - 1) / kBlurTW, tiles_y = (H + kBlurTH - 1) / kBlurTH;
  unsigned grid;
  if (!grid_of(fn, tiles_x, tiles_y, P, grid)) return WALDO_EINVAL;
  BlurWeights wt{};
  float sum = 0.0f;
  for (int i = 0; i < k; ++i) {  // exp(-0.5 (t / sigma)^2) at t = linspace(-(k-1)/2, (k-1)/2, k): integers for an odd k
    const float q = (float)(i - k / 2) / sigma;
    wt.w[i] = expf(-0.5f * (q * q));
    sum += wt.w[i];
  }
  for (int i = 0; i < k; ++i) wt.w[i] /= sum;
  gaussian_blur_kernel<<<dim3(grid), dim3(kBlock), 0, (hipStream_t)stream>>>(x, y, H, W, k, tiles_x, tiles_y, wt);
  return launch_status(fn);
}

static bool pixel_grid(const char* fn, int64_t N, int64_t HW, unsigned& grid, int& chunks) {
  if (N < 0 || HW < 1 || HW > (int64_t)32768 * 32768) {
    set_error("%s: bad shape N=%lld HW=%lld", fn, (long long)N, (long long)HW);
    return false;
  }
  const int64_t c = (HW + kBlock - 1) / kBlock;
  chunks = (int)c;
  return N == 0 || grid_of(fn, c, 1, N, grid);
}

extern "C" int waldo_mov_props_fwd(const float* lyt, const float* flow, uint32_t fg_bits, uint32_t bg_bits,
                                   uint32_t other_bits, float* fg_prop, float* nobg_prop, float* other_prop,
                                   float* blur_in, int64_t N, int Nl, int64_t HW, waldo_stream_t stream) {
  const char* fn = "waldo_mov_props_fwd";
  if (Nl < 1 || Nl > 32) {
    set_error("%s: Nl=%d layout channels (1 .. 32: the channel lists are bit masks)", fn, Nl);
    return WALDO_EINVAL;
  }
  if (Nl < 32 && ((fg_bits | bg_bits | other_bits) >> Nl) != 0) {
    set_error("%s: a channel list names a channel at or above Nl=%d", fn, Nl);
    return WALDO_EINVAL;
  }
  unsigned grid = 0;
  int chunks = 0;
  if (!pixel_grid(fn, N, HW, grid, chunks)) return WALDO_EINVAL;
  if (N == 0) return WALDO_OK;
  if (!lyt || !flow || !fg_prop || !nobg_prop || !other_prop || !blur_in) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  mov_props_kernel<<<dim3(grid), dim3(kBlock), 0, (hipStream_t)stream>>>(lyt, flow, fg_bits, bg_bits, other_bits, fg_prop,
                                                                        nobg_prop, other_prop, blur_in, Nl, HW, chunks);
  return launch_status(fn);
}

extern "C" int waldo_mov_finish_fwd(const float* flow, const float* blurred, const float* fg_prop,
                                    const float* nobg_prop, const float* other_prop, const float* edge_raw,
                                    const float* dominant, float flow_thresh, float mov_obj_thresh, float reg_bg_mul,
                                    float nobg_edge_mul, int flags, float* edge, float* mean_bg_flow, float* mask,
                                    float* mov_obj, int64_t N, int64_t HW, waldo_stream_t stream) {
  const char* fn = "waldo_mov_finish_fwd";
  const int all = WALDO_MOV_USE_FG | WALDO_MOV_USE_NOBG | WALDO_MOV_USE_NOBG_EDGE | WALDO_MOV_FLOW_NOBG |
                  WALDO_MOV_DOMINANT_OTHER;
  if ((flags & ~all) != 0 || ((flags & WALDO_MOV_FLOW_NOBG) && (flags & WALDO_MOV_DOMINANT_OTHER))) {
    set_error("%s: bad flags %d (unknown bits, or WALDO_MOV_FLOW_NOBG with WALDO_MOV_DOMINANT_OTHER)", fn, flags);
    return WALDO_EINVAL;
  }
  if (!finite(flow_thresh) || !finite(mov_obj_thresh) || !finite(reg_bg_mul) || !finite(nobg_edge_mul)) {
    set_error("%s: a threshold or multiplier is not finite", fn);
    return WALDO_EINVAL;
  }
  unsigned grid = 0;
  int chunks = 0;
  if (!pixel_grid(fn, N, HW, grid, chunks)) return WALDO_EINVAL;
  if (N == 0) return WALDO_OK;
  if (!flow || !blurred || !fg_prop || !nobg_prop || !other_prop || !edge_raw || !dominant || !edge || !mean_bg_flow ||
      !mask || !mov_obj) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  FinishArgs A{flow,  blurred,      fg_prop, nobg_prop, other_prop,  edge_raw,       dominant,   edge,          mean_bg_flow,
               mask,  mov_obj,      flow_thresh,        mov_obj_thresh, reg_bg_mul, nobg_edge_mul, flags,
               chunks, HW};
  mov_finish_kernel<<<dim3(grid), dim3(kBlock), 0, (hipStream_t)stream>>>(A);
  return launch_status(fn);
}

extern "C" int64_t waldo_cell_distance_workspace_bytes(int64_t F, int No, int64_t HW) {
  if (F < 0 || No < 1 || No > kCellMaxObj || HW < 1) return 0;
  const int64_t bytes = F * cell_chunks(HW) * No * 3 * (int64_t)sizeof(float);
  return (bytes + 255) / 256 * 256;
}

extern "C" int waldo_cell_distance_fwd(const float* moments, const float* mov_mask, const float* fg_mask,
                                       const float* gx, const float* gy, float* out, uint8_t* chosen, void* workspace,
                                       int64_t workspace_bytes, int64_t F, int No, int H, int W, float K, float eps,
                                       waldo_stream_t stream) {
  const char* fn = "waldo_cell_distance_fwd";
  unsigned grid = 0;
  const int rc = cell_check(fn, moments, mov_mask, gx, gy, workspace, workspace_bytes, F, No, H, W, K, eps, grid);
  if (rc != WALDO_OK) return rc > 0 ? WALDO_OK : rc;
  if (!out || !chosen) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const float count = (float)((double)F * H * W);
  CellArgs A{moments, mov_mask, fg_mask, gx, gy, nullptr, static_cast<float*>(workspace), chosen, nullptr, No, H, W,
             (int)cell_chunks((int64_t)H * W), K, eps, count};
  hipStream_t st = (hipStream_t)stream;
  if (fg_mask) cell_distance_fwd_kernel<true><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  else cell_distance_fwd_kernel<false><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  cell_mean_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(A.partial, (int64_t)grid, count, out);
  return launch_status(fn);
}

extern "C" int waldo_cell_distance_bwd(const float* moments, const float* mov_mask, const float* fg_mask,
                                       const float* gx, const float* gy, const uint8_t* chosen, const float* grad_out,
                                       float* grad_moments, float* grad_fg, void* workspace, int64_t workspace_bytes,
                                       int64_t F, int No, int H, int W, float K, float eps, waldo_stream_t stream) {
  const char* fn = "waldo_cell_distance_bwd";
  unsigned grid = 0;
  const int rc = cell_check(fn, moments, mov_mask, gx, gy, workspace, workspace_bytes, F, No, H, W, K, eps, grid);
  if (rc != WALDO_OK) return rc > 0 ? WALDO_OK : rc;
  if (!chosen || !grad_out || !grad_moments || (grad_fg && !fg_mask)) {
    set_error("%s: null pointer (chosen, grad_out, grad_moments; grad_fg without fg_mask)", fn);
    return WALDO_EINVAL;
  }
  const float count = (float)((double)F * H * W);
  const int chunks = (int)cell_chunks((int64_t)H * W);
  CellArgs A{moments, mov_mask, fg_mask, gx, gy, grad_out, static_cast<float*>(workspace),
             const_cast<uint8_t*>(chosen), grad_fg, No, H, W, chunks, K, eps, count};
  hipStream_t st = (hipStream_t)stream;
  if (fg_mask) cell_distance_bwd_kernel<true><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  else cell_distance_bwd_kernel<false><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  const int64_t total = F * No * 3;
  cell_moments_grad_kernel<<<dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(
      A.partial, grad_out, count, grad_moments, total, No * 3, chunks);
  return launch_status(fn);
}
