// Frame metrics (include/waldo_hip.h "Frame metrics"): PSNR, SSIM and MS-SSIM per frame, TensorFlow's definitions
// (tf.image.psnr / ssim / ssim_multiscale, max_val = 1) as the reference's scorer calls them (tools/eval/metrics.py:67-74).
//
// One pass kernel per scale: a workgroup owns a 32 x 64 pixel tile of one (frame, channel) and the SSIM outputs at the
// same positions (an output's 11 x 11 window starts at its pixel).  It stages the tile and its 10-pixel apron of both
// operands in LDS as fp32 values in [0, 1], runs the separable 11-tap correlation (rows into LDS, then columns in
// registers), and writes one partial sum of lum * cs and of cs (fp64) -- and, at scale 0, of the squared error over its
// pixels (PSNR).  With MS-SSIM the pass also writes the 2 x 2 average of its pixels (the next scale, symmetric padding
// at an odd end) into the caller's scratch: each scale's source is read from HBM once.
//
// The window statistics are TF's _ssim_helper on SHIFTED operands.  TF forms the variance term as E[x^2 + y^2] -
// (mx^2 + my^2), a difference of two sums of about 2 mu^2: in fp32 a bright, nearly flat window (mu^2 2000 times the
// variance + c2) loses the bits the term needs, 4e-5 on the frame's SSIM.  Variance and covariance do not change when
// a constant is subtracted from an operand, so the workgroup subtracts from each operand the mean of its staged
// in-frame values (cx, cy), filters x' = x - cx, y' = y - cy, x'^2 + y'^2 and x'y', and takes
//   cs  = (2 E[x'y'] - 2 dx dy + c2) / (E[x'^2 + y'^2] - (dx^2 + dy^2) + c2),   dx = E[x'], dy = E[y'],
//   lum = (2 mx my + c1) / (mx^2 + my^2 + c1),   mx = dx + cx, my = dy + cy
// -- TF's operation order otherwise, commutative in (x, y), and cs = lum = 1 exactly for equal operands.  PSNR and the
// pooled next scale use the staged values as they are.
// The combine kernel sums the partials of a frame in a fixed order in fp64: no atomics, the same bits on every call.
#include "packed_clip.hip.h"
#include "quantize.hip.h"

namespace waldo {

namespace {

constexpr int kTaps = 11;
constexpr int kMetTileH = 32, kMetTileW = 64;                   // owned pixels = SSIM outputs of a workgroup
constexpr int kStageH = kMetTileH + kTaps - 1;               // 42 staged rows
constexpr int kStageW = kMetTileW + kTaps - 1;               // 74 staged columns that feed an output
constexpr int kStagePitch = (kStageW + 3) / 4 * 4;           // 76 staged: rows of whole float4s
constexpr int kRowQuads = kMetTileW / 4;                     // a row thread filters 4 adjacent outputs
constexpr int kRowsPerThread = kMetTileH / (kBlock / kMetTileW);  // 8 output rows per thread (4 waves x 8 rows)
constexpr int kScales = 5;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;  // (k1 max_val)^2, (k2 max_val)^2
// the source of a pass: a caller's operand (waldo_metrics_enc) or, past scale 0, the pooled fp32 [0, 1] scratch
constexpr int kEncUnit = 3;

struct Operand {
  const void* p;
  int64_t sb, st, sc, sh;
  int enc;
};

struct Window {
  float g[kTaps];
};

struct PassArgs {
  Operand a, b;
  Window win;
  const float* rgb_table;
  float* pool_a;  // next scale of each operand, (B*T, 3, Hn, Wn); null when there is no next scale
  float* pool_b;
  double* partials;  // (B*T, 3, tiles, 3): sum lum*cs, sum cs, sum (x - y)^2
  int T, H, W, Hn, Wn, tiles_x, tiles, quant;
  float lo, range;
};

__device__ __forceinline__ float quantize(float x, float lo, float range, int quant) {
  const float u = quant_unit(x, lo, range);  // (quantize.hip.h: the formula of every byte the library writes)
  if (quant == WALDO_METRICS_TRUNC) return quant_level_trunc(u) / 255.0f;
  if (quant == WALDO_METRICS_ROUND) return quant_level_round(u) / 255.0f;
  return u;
}

// the [0, 1] value of channel c of pixel (y, x) of frame (bi, ti); the 256-entry table in LDS serves the byte encodings
__device__ __forceinline__ float load_unit(const Operand& o, const float* tab, int64_t bi, int64_t ti, int c, int y,
                                           int x, float lo, float range, int quant) {
  const int64_t base = bi * o.sb + ti * o.st + (int64_t)y * o.sh + x;
  switch (o.enc) {
    case WALDO_METRICS_F32:
      return quantize(static_cast<const float*>(o.p)[base + c * o.sc], lo, range, quant);
    case WALDO_METRICS_U8:
      return tab[static_cast<const uint8_t*>(o.p)[base + c * o.sc]];
    case WALDO_METRICS_PACKED:
      return tab[(static_cast<const uint32_t*>(o.p)[base] >> (8 * c)) & 255u];
    default:  // kEncUnit: sb = the plane of a frame's 3 channels, sc = a channel's plane
      return static_cast<const float*>(o.p)[base + c * o.sc];
  }
}

__device__ __forceinline__ void fill_table(float* tab, const Operand& o, const float* rgb_table, float lo, float range,
                                           int quant) {
  static_assert(kBlock == kRgbTable, "one table entry per thread");
  const int i = threadIdx.x;
  if (o.enc == WALDO_METRICS_U8) tab[i] = (float)i / 255.0f;
  else if (o.enc == WALDO_METRICS_PACKED) tab[i] = quantize(rgb_table[i], lo, range, quant);
}

// fixed-order sum over the 64 lanes of a wave (every lane gets it)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void frame_metrics_pass_kernel(PassArgs P, int scale0) {
  __shared__ __attribute__((aligned(16))) float sx[kStageH][kStagePitch], sy[kStageH][kStagePitch];
  __shared__ __attribute__((aligned(16))) float hq[4][kStageH][kMetTileW];  // row-filtered x', y', x'^2 + y'^2, x'y'
  __shared__ float tab_a[kRgbTable], tab_b[kRgbTable];
  __shared__ float stage_sum[2][kBlock / 64];
  __shared__ double red[3][kBlock / 64];

  const unsigned fc = blockIdx.x / (unsigned)P.tiles;  // frame * 3 + channel
  const int tile = (int)(blockIdx.x - fc * (unsigned)P.tiles);
  const int f = (int)(fc / 3u), c = (int)(fc - 3u * (unsigned)f);
  const int64_t bi = f / P.T, ti = f % P.T;
  const int y0 = (tile / P.tiles_x) * kMetTileH, x0 = (tile % P.tiles_x) * kMetTileW;
  const int H = P.H, W = P.W;

  if (scale0) {
    fill_table(tab_a, P.a, P.rgb_table, P.lo, P.range, P.quant);
    fill_table(tab_b, P.b, P.rgb_table, P.lo, P.range, P.quant);
    __syncthreads();
  }
  // stage: pixels outside the frame are 0 (they feed no VALID output); columns 74 and 75 only fill the last float4.
  // On the way: the sum of the in-frame values of each operand in the 74 columns (the shift), and at scale 0 the
  // squared error over the owned pixels (PSNR)
  double se = 0.0;
  float sum_a = 0.0f, sum_b = 0.0f;
  for (int i = threadIdx.x; i < kStageH * kStagePitch; i += kBlock) {
    const int r = i / kStagePitch, q = i - r * kStagePitch;
    const int y = y0 + r, x = x0 + q;
    float va = 0.0f, vb = 0.0f;
    if (y < H && x < W) {
      va = load_unit(P.a, tab_a, bi, ti, c, y, x, P.lo, P.range, P.quant);
      vb = load_unit(P.b, tab_b, bi, ti, c, y, x, P.lo, P.range, P.quant);
      if (q < kStageW) {
        sum_a += va;
        sum_b += vb;
      }
      if (scale0 && r < kMetTileH && q < kMetTileW) {
        const float d = va - vb;
        se += (double)(d * d);
      }
    }
    sx[r][q] = va;
    sy[r][q] = vb;
  }
  sum_a = wave_sum(sum_a);
  sum_b = wave_sum(sum_b);
  if ((threadIdx.x & 63) == 0) {
    stage_sum[0][threadIdx.x / 64] = sum_a;
    stage_sum[1][threadIdx.x / 64] = sum_b;
  }
  __syncthreads();
  // the shift of each operand: the mean of its staged in-frame values, the same bits in every thread
  const float staged = (float)((min(H - y0, kStageH)) * (min(W - x0, kStageW)));
  const float cx = ((stage_sum[0][0] + stage_sum[0][1]) + (stage_sum[0][2] + stage_sum[0][3])) / staged;
  const float cy = ((stage_sum[1][0] + stage_sum[1][1]) + (stage_sum[1][2] + stage_sum[1][3])) / staged;

  // rows: the 11-tap correlation along x of the four quantities, for every staged row; a thread filters 4 adjacent
  // outputs from the 14 staged values under their windows (16 read, as float4s)
  for (int i = threadIdx.x; i < kStageH * kRowQuads; i += kBlock) {
    const int r = i / kRowQuads, q = (i - r * kRowQuads) * 4;
    float xs[16], ys[16], ss[16], xy[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 a = *reinterpret_cast<const float4*>(&sx[r][q + 4 * v]);
      const float4 b = *reinterpret_cast<const float4*>(&sy[r][q + 4 * v]);
      xs[4 * v] = a.x - cx, xs[4 * v + 1] = a.y - cx, xs[4 * v + 2] = a.z - cx, xs[4 * v + 3] = a.w - cx;
      ys[4 * v] = b.x - cy, ys[4 * v + 1] = b.y - cy, ys[4 * v + 2] = b.z - cy, ys[4 * v + 3] = b.w - cy;
    }
#pragma unroll
    for (int k = 0; k < 4 + kTaps - 1; ++k) {
      ss[k] = xs[k] * xs[k] + ys[k] * ys[k];
      xy[k] = xs[k] * ys[k];
    }
    float e[4][4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float ex = 0.0f, ey = 0.0f, ess = 0.0f, exy = 0.0f;
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
        const float g = P.win.g[j];
        ex += g * xs[o + j];
        ey += g * ys[o + j];
        ess += g * ss[o + j];
        exy += g * xy[o + j];
      }
      e[0][o] = ex, e[1][o] = ey, e[2][o] = ess, e[3][o] = exy;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      *reinterpret_cast<float4*>(&hq[k][r][q]) = make_float4(e[k][0], e[k][1], e[k][2], e[k][3]);
  }

  // the next scale's 2 x 2 averages of the owned pixels
  if (P.pool_a) {
    constexpr int PH = kMetTileH / 2, PW = kMetTileW / 2;
    const int64_t plane = (int64_t)P.Hn * P.Wn, fbase = ((int64_t)f * 3 + c) * plane;
    for (int i = threadIdx.x; i < PH * PW; i += kBlock) {
      const int r = i / PW, q = i - r * PW;
      const int py = y0 / 2 + r, px = x0 / 2 + q;
      if (py < P.Hn && px < P.Wn) {
        // rows 2py, 2py + 1 (the last row again at an odd end: SYMMETRIC padding), the same for columns
        const int r0 = 2 * py - y0, r1 = min(2 * py + 1, H - 1) - y0;
        const int q0 = 2 * px - x0, q1 = min(2 * px + 1, W - 1) - x0;
        const int64_t o = fbase + (int64_t)py * P.Wn + px;
        P.pool_a[o] = ((sx[r0][q0] + sx[r0][q1]) + (sx[r1][q0] + sx[r1][q1])) * 0.25f;
        P.pool_b[o] = ((sy[r0][q0] + sy[r0][q1]) + (sy[r1][q0] + sy[r1][q1])) * 0.25f;
      }
    }
  }
  __syncthreads();

  // columns: each thread 8 outputs of one column from 18 row-filtered rows held in registers
  const int q = threadIdx.x & (kMetTileW - 1), rg = (threadIdx.x / kMetTileW) * kRowsPerThread;
  const int Hv = H - (kTaps - 1), Wv = W - (kTaps - 1);  // the VALID map
  float sum_ssim = 0.0f, sum_cs = 0.0f;
  if (x0 + q < Wv) {
    float h[4][kRowsPerThread + kTaps - 1];
#pragma unroll
    for (int r = 0; r < kRowsPerThread + kTaps - 1; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) h[k][r] = hq[k][rg + r][q];
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
      float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < kTaps; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] += P.win.g[j] * h[k][o + j];
      // TF's _ssim_helper in its operation order, on the shifted operands; the means get the shift back
      const float mx = e[0] + cx, my = e[1] + cy;
      const float lum = (mx * my * 2.0f + kC1) / (mx * mx + my * my + kC1);
      const float num0 = e[0] * e[1] * 2.0f;
      const float den0 = e[0] * e[0] + e[1] * e[1];
      const float num1 = e[3] * 2.0f;
      const float cs = (num1 - num0 + kC2) / (e[2] - den0 + kC2);
      if (y0 + rg + o < Hv) {
        sum_ssim += lum * cs;
        sum_cs += cs;
      }
    }
  }

  // the workgroup's partials: waves in order
  const double s0 = wave_sum((double)sum_ssim), s1 = wave_sum((double)sum_cs), s2 = wave_sum(se);
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = s0;
    red[1][wave] = s1;
    red[2][wave] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
    P.partials[((int64_t)fc * P.tiles + tile) * 3 + threadIdx.x] = s;
  }
}

struct CombineArgs {
  const double* partials;   // scales one after the other, each (B*T, 3, tiles_k, 3)
  int64_t part_off[kScales];  // in entries of 3 doubles
  int tiles[kScales];
  double valid[kScales];    // VALID outputs of a channel at each scale
  int nscales;
  double npix;              // 3 H W
  float* psnr;
  float* ssim;
  float* msssim;
};

// one wave per frame: lane l sums the tiles l, l + 64, ... of each (channel, scale), then the wave sums the lanes
__global__ __launch_bounds__(64) void frame_metrics_combine_kernel(CombineArgs A) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const double w[kScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};  // TF's _MSSSIM_WEIGHTS
  double se = 0.0, ssim = 0.0, ms = 0.0;
  for (int c = 0; c < 3; ++c) {
    double prod = 1.0;
    for (int k = 0; k < A.nscales; ++k) {
      const double* p = A.partials + (A.part_off[k] + ((int64_t)f * 3 + c) * A.tiles[k]) * 3;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      for (int t = lane; t < A.tiles[k]; t += 64) {
        s0 += p[(int64_t)t * 3];
        s1 += p[(int64_t)t * 3 + 1];
        s2 += p[(int64_t)t * 3 + 2];
      }
      s0 = wave_sum(s0) / A.valid[k];
      s1 = wave_sum(s1) / A.valid[k];
      s2 = wave_sum(s2);
      if (k == 0) {
        se += s2;
        ssim += s0;
      }
      // relu(cs)^w below the last scale, relu(ssim)^w at it (pow(0, w) = 0)
      const double v = k + 1 < kScales ? s1 : s0;
      prod *= pow(fmax(v, 0.0), w[k]);
    }
    ms += prod;
  }
  if (lane == 0) {
    if (A.psnr) {
      const double mse = se / A.npix;
      A.psnr[f] = mse == 0.0 ? __builtin_inff() : (float)(-10.0 * log10(mse));
    }
    if (A.ssim) A.ssim[f] = (float)(ssim / 3.0);
    if (A.msssim) A.msssim[f] = (float)(ms / 3.0);
  }
}

}  // namespace waldo

using namespace waldo;

namespace {

struct Scales {
  int n;
  int H[kScales], W[kScales], tiles_x[kScales], tiles[kScales];
  int64_t part_off[kScales], part_entries, pool_off[kScales], pool_floats;  // pool_off[k]: scale k's planes (k >= 1)
};

Scales plan(int B, int T, int H, int W, int mask) {
  Scales s{};
  const int64_t frames = (int64_t)B * T;
  s.n = (mask & WALDO_METRIC_MSSSIM) ? kScales : 1;
  for (int k = 0; k < s.n; ++k) {
    s.H[k] = k ? (s.H[k - 1] + 1) / 2 : H;
    s.W[k] = k ? (s.W[k - 1] + 1) / 2 : W;
    s.tiles_x[k] = (s.W[k] + kMetTileW - 1) / kMetTileW;
    s.tiles[k] = ((s.H[k] + kMetTileH - 1) / kMetTileH) * s.tiles_x[k];
    s.part_off[k] = s.part_entries;
    s.part_entries += frames * 3 * s.tiles[k];
    if (k) {
      s.pool_off[k] = s.pool_floats;
      s.pool_floats += 2 * frames * 3 * (int64_t)s.H[k] * s.W[k];  // both operands
    }
  }
  return s;
}

bool shape_ok(int B, int T, int H, int W, int mask) {
  return B >= 0 && T >= 0 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && mask > 0 && mask < 8;
}

}  // namespace

extern "C" int64_t waldo_frame_metrics_partial_bytes(int B, int T, int H, int W, int mask) {
  if (!shape_ok(B, T, H, W, mask)) return -1;
  return plan(B, T, H, W, mask).part_entries * 3 * (int64_t)sizeof(double);
}

extern "C" int64_t waldo_frame_metrics_scratch_bytes(int B, int T, int H, int W, int mask) {
  if (!shape_ok(B, T, H, W, mask)) return -1;
  return plan(B, T, H, W, mask).pool_floats * (int64_t)sizeof(float);
}

extern "C" int waldo_frame_metrics_fwd(const void* a, int enc_a, int64_t sa_b, int64_t sa_t, int64_t sa_c,
                                       int64_t sa_h, const void* b, int enc_b, int64_t sb_b, int64_t sb_t,
                                       int64_t sb_c, int64_t sb_h, const float* rgb_table, int B, int T, int H, int W,
                                       float lo, float range, int quant, int mask, double* partials, float* scratch,
                                       float* psnr, float* ssim, float* msssim, waldo_stream_t stream) {
  const char* fn = "waldo_frame_metrics_fwd";
  if (!shape_ok(B, T, H, W, mask)) {
    set_error("%s: bad shape B=%d T=%d H=%d W=%d mask=%d (1 <= H, W <= 32768; mask: WALDO_METRIC_* bits)", fn, B, T,
              H, W, mask);
    return WALDO_EINVAL;
  }
  const bool want_ssim = mask & (WALDO_METRIC_SSIM | WALDO_METRIC_MSSSIM);
  const Scales s = plan(B, T, H, W, mask);
  if (want_ssim && (s.H[s.n - 1] < kTaps || s.W[s.n - 1] < kTaps)) {
    set_error("%s: %dx%d is too small: every scale must be at least 11x11 (SSIM: H, W >= 11; MS-SSIM: H, W >= 161)",
              fn, H, W);
    return WALDO_EINVAL;
  }
  for (int e : {enc_a, enc_b})
    if (e < WALDO_METRICS_F32 || e > WALDO_METRICS_PACKED) {
      set_error("%s: unknown operand encoding %d", fn, e);
      return WALDO_EINVAL;
    }
  if (quant < WALDO_METRICS_TRUNC || quant > WALDO_METRICS_NONE || !(range > 0.0f)) {
    set_error("%s: bad quantisation %d or range %g (> 0)", fn, quant, (double)range);
    return WALDO_EINVAL;
  }
  const int64_t frames = (int64_t)B * T;
  if (frames == 0) return WALDO_OK;
  if (!a || !b || !partials || (s.n > 1 && !scratch) ||
      ((enc_a == WALDO_METRICS_PACKED || enc_b == WALDO_METRICS_PACKED) && !rgb_table) ||
      ((mask & WALDO_METRIC_PSNR) && !psnr) || ((mask & WALDO_METRIC_SSIM) && !ssim) ||
      ((mask & WALDO_METRIC_MSSSIM) && !msssim)) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (frames * 3 * s.tiles[0] > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  // TF's _fspecial_gauss: softmax of -0.5 (i - 5)^2 / 1.5^2, separable
  Window win;
  double g[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) sum += g[i] = std::exp(-0.5 * (i - 5) * (i - 5) / (1.5 * 1.5));
  for (int i = 0; i < kTaps; ++i) win.g[i] = (float)(g[i] / sum);

  PassArgs P{};
  P.win = win;
  P.rgb_table = rgb_table;
  P.partials = partials;
  P.T = T;
  P.quant = quant;
  P.lo = lo;
  P.range = range;
  for (int k = 0; k < s.n; ++k) {
    P.H = s.H[k];
    P.W = s.W[k];
    P.tiles_x = s.tiles_x[k];
    P.tiles = s.tiles[k];
    P.partials = partials + s.part_off[k] * 3;
    if (k == 0) {
      P.a = Operand{a, sa_b, sa_t, sa_c, sa_h, enc_a};
      P.b = Operand{b, sb_b, sb_t, sb_c, sb_h, enc_b};
    } else {
      // the previous pass's pooled planes (B*T, 3, Hk, Wk): frame stride 3 Hk Wk, T-major
      const int64_t plane = (int64_t)s.H[k] * s.W[k];
      const float* pa = scratch + s.pool_off[k];
      P.a = Operand{pa, (int64_t)T * 3 * plane, 3 * plane, plane, s.W[k], kEncUnit};
      P.b = Operand{pa + frames * 3 * plane, (int64_t)T * 3 * plane, 3 * plane, plane, s.W[k], kEncUnit};
    }
    if (k + 1 < s.n) {
      P.Hn = s.H[k + 1];
      P.Wn = s.W[k + 1];
      P.pool_a = scratch + s.pool_off[k + 1];
      P.pool_b = P.pool_a + frames * 3 * (int64_t)P.Hn * P.Wn;
    } else {
      P.Hn = P.Wn = 0;
      P.pool_a = P.pool_b = nullptr;
    }
    frame_metrics_pass_kernel<<<dim3((unsigned)(frames * 3 * s.tiles[k])), dim3(kBlock), 0, (hipStream_t)stream>>>(
        P, k == 0);
    const int rc = launch_status(fn);
    if (rc != WALDO_OK) return rc;
  }
  CombineArgs A{};
  A.partials = partials;
  for (int k = 0; k < s.n; ++k) {
    A.part_off[k] = s.part_off[k];
    A.tiles[k] = s.tiles[k];
    A.valid[k] = (double)(s.H[k] - (kTaps - 1)) * (s.W[k] - (kTaps - 1));
  }
  A.nscales = s.n;
  A.npix = 3.0 * H * W;
  A.psnr = (mask & WALDO_METRIC_PSNR) ? psnr : nullptr;
  A.ssim = (mask & WALDO_METRIC_SSIM) ? ssim : nullptr;
  A.msssim = (mask & WALDO_METRIC_MSSSIM) ? msssim : nullptr;
  if (frames > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  frame_metrics_combine_kernel<<<dim3((unsigned)frames), dim3(64), 0, (hipStream_t)stream>>>(A);
  return launch_status(fn);
}
