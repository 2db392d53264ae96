// Renders (include/waldo_hip.h "Renders"): the views of the layered decomposition as bytes, made on the device.
//   waldo_render_argmax_fwd   N frames of C planes -> the class id of every pixel (torch.max's index on the CPU) as a
//                             byte, and / or palette[id] as RGB bytes: the reference's Logger.get_lyt
//                             (tools/logger.py:169-179 -> tools/utils.py:202-214) without its trip through the host;
//   waldo_render_flow_fwd     N flows (2, H, W) -> the colour-wheel picture of Logger.get_flow_rgb (tools/logger.py:310-318),
//                             quantised with the library's one quantisation (quantize.hip.h), span (0, 1).
//
// Both are streaming passes over the rows of byte_rows.hip.h (H merged into the row where the source rows are dense): a
// lane keeps its 16 pixels' running maxima and ids in registers while it walks the C planes -- kAhead planes' 16-byte
// loads in flight -- and writes 16 ids as one 16-byte store, an interleaved group as three.  The head reaches the first
// 16-byte boundary of the row's PRIMARY destination: the id map where there is one, else the RGB bytes.  The body's loads
// are 16-byte ones where every plane's row is 16-byte aligned at the head's end.
// With two destinations (ids AND rgb) or a planar one whose planes are not a multiple of 16 bytes apart, the others may
// sit at another alignment than the primary: every store checks its own address (store_words: 16-byte, else dword, else
// byte stores -- uniform over a row), so any alignment is correct and the aligned case pays one compare.
// The palette lives in LDS as one packed word per class (0x00BBGGRR), filled by the workgroup at entry; the flow wheel
// too while it has at most kWheelLds rows.  No atomics, no workspace, no allocation; the caller's stream.
#include "byte_rows.hip.h"

namespace waldo {

namespace {

constexpr int kMaxClasses = 256; // an id fits a byte
constexpr int kWheelLds = 256;   // rows of a flow wheel kept in LDS (a larger one is read from global memory)
constexpr int kMaxWheel = 4096;

struct Dest {
  uint8_t* ids;   // this row of the id map, or null
  uint8_t* rgb;   // planar: this row of plane 0; interleaved: the row's first byte; or null
  int64_t plane;  // bytes between the planes of a planar frame
  bool nhwc;
};

struct RenderArgs {
  const void* src;
  int64_t ss_n, ss_c, ss_h;  // in elements
  const uint8_t* palette;    // argmax: C rows of 3 bytes
  const float* wheel;        // flow: K rows of 3 fp32
  uint8_t* ids;
  int64_t di_n;
  uint8_t* rgb;
  int64_t dr_n;
  Rows R;  // (rows of a frame: Hr)
  int C, K, quant;
  float mul;
  bool nhwc;
};

// NP consecutive pixels from pixel x of the row on: ids id[] and colours col[] (0x00BBGGRR) to whatever the row writes.
// NP = 16 (a lane's group), 4 or 1 (the tail and the head).
template <int NP>
__device__ __forceinline__ void emit(const Dest& d, int64_t x, const uint32_t (&id)[NP], const uint32_t (&col)[NP]) {
  if constexpr (NP == 1) {
    if (d.ids) d.ids[x] = (uint8_t)id[0];
    if (d.rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) (d.nhwc ? d.rgb + 3 * x + c : d.rgb + c * d.plane + x)[0] = (uint8_t)(col[0] >> (8 * c));
    }
  } else {
    if (d.ids) {
      uint32_t w[NP / 4];
      pack_planar<NP>(w, [&](int k) { return id[k]; });
      store_words(d.ids + x, w);
    }
    if (d.rgb && d.nhwc) {
      uint32_t w[3 * NP / 4];
      pack_interleaved<NP>(w, [&](int c, int k) { return (col[k] >> (8 * c)) & 255u; });
      store_words(d.rgb + 3 * x, w);
    } else if (d.rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t w[NP / 4];
        pack_planar<NP>(w, [&](int k) { return (col[k] >> (8 * c)) & 255u; });
        store_words(d.rgb + c * d.plane + x, w);
      }
    }
  }
}

// the destinations of row r of frame n, and the row's head
__device__ __forceinline__ Dest row_dest(const RenderArgs& A, int64_t n, int r, int& head) {
  Dest d;
  d.nhwc = A.nhwc;
  d.plane = (int64_t)A.R.Hr * A.R.Wr;
  d.ids = A.ids ? A.ids + n * A.di_n + (int64_t)r * A.R.Wr : nullptr;
  d.rgb = A.rgb ? A.rgb + n * A.dr_n + (int64_t)r * A.R.Wr * (A.nhwc ? 3 : 1) : nullptr;
  head = row_head(d.ids ? d.ids : d.rgb, !d.ids && d.nhwc, A.R.Wr);
  return d;
}

// torch.max's index on the CPU: the lowest c among the maxima, NaN above everything and the first NaN kept
__device__ __forceinline__ void take(float v, uint32_t c, float& best, uint32_t& id) {
  if (v > best || (v != v && best == best)) {
    best = v;
    id = c;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void render_argmax_kernel(RenderArgs A) {
  __shared__ uint32_t pal[kMaxClasses];
  static_assert(kBlock >= kMaxClasses, "one palette row per thread");
  const bool want_rgb = A.rgb != nullptr;
  if (want_rgb) {
    if ((int)threadIdx.x < A.C) {
      const uint8_t* q = A.palette + 3 * threadIdx.x;
      pal[threadIdx.x] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
    __syncthreads();
  }
  int64_t n;
  int r, chunk, head;
  decode_row(A.R, n, r, chunk);
  const Dest d = row_dest(A, n, r, head);
  const T* __restrict__ s0 = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const int64_t sc = A.ss_c;
  const int C = A.C;
  // every plane's row is 16-byte aligned at the head's end (then at every group: 16 elements are 32 or 64 bytes)
  const bool vec = aligned16(s0 + head) && (C == 1 || ((uint64_t)sc * sizeof(T)) % 16 == 0);
  walk_row(head, chunk, A.R.Wr, [&](auto np, int64_t x) {
    constexpr int NP = decltype(np)::value;
    constexpr int kAhead = NP != kPx ? 1 : sizeof(T) == 4 ? 2 : 4;  // planes in flight: 8 16-byte loads of a lane
    const T* __restrict__ p = s0 + x;
    float best[NP];
    uint32_t id[NP];
    {
      T v[NP];
      load_px(p, vec, v);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        best[k] = widen(v[k]);
        id[k] = 0;
      }
    }
    int c = 1;
    for (; c + kAhead <= C; c += kAhead) {
      T v[kAhead][NP];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) load_px(p + (c + u) * sc, vec, v[u]);
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
#pragma unroll
        for (int k = 0; k < NP; ++k) take(widen(v[u][k]), (uint32_t)(c + u), best[k], id[k]);
    }
    for (; c < C; ++c) {
      T v[NP];
      load_px(p + c * sc, vec, v);
#pragma unroll
      for (int k = 0; k < NP; ++k) take(widen(v[k]), (uint32_t)c, best[k], id[k]);
    }
    uint32_t col[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) col[k] = want_rgb ? pal[id[k]] : 0u;
    emit<NP>(d, x, id, col);
  });
}

constexpr float kSqrt2 = 1.41421356237309504880f, kPi = 3.14159265358979323846f;

// Logger.get_flow_rgb of one pixel, then the quantisation: 0x00BBGGRR.  `wheel`: K rows of 3 fp32 (LDS or global).
// r keeps a NaN (the reference's r[r > 1] = 1 does) and a NaN angle takes bin 0: NaN anywhere -> r * wheel is NaN -> 0.
__device__ __forceinline__ uint32_t flow_colour(float u, float v, const float* wheel, int K, float mul, int quant) {
  const float m = sqrtf(u * u + v * v);
  const float s = m / kSqrt2 * mul;
  const float r = s > 1.0f ? 1.0f : s;
  const float theta = (1.0f + atan2f(v, u) / kPi) / 2.0f;
  const float tk = theta * (float)K;
  const int k = tk >= 0.0f ? min((int)fminf(tk, (float)K), K - 1) : 0;
  const float* w = wheel + 3 * k;
  return quant_byte(r * w[0], 0.0f, 1.0f, quant) | (quant_byte(r * w[1], 0.0f, 1.0f, quant) << 8) |
         (quant_byte(r * w[2], 0.0f, 1.0f, quant) << 16);
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kBlock) void render_flow_kernel(RenderArgs A) {
  __shared__ float wheel_s[LDS ? 3 * kWheelLds : 1];
  const float* wheel = A.wheel;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < 3 * A.K; i += kBlock) wheel_s[i] = A.wheel[i];
    __syncthreads();
    wheel = wheel_s;
  }
  int64_t n;
  int r, chunk, head;
  decode_row(A.R, n, r, chunk);
  const Dest d = row_dest(A, n, r, head);
  const T* __restrict__ su = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const T* __restrict__ sv = su + A.ss_c;
  const int K = A.K, quant = A.quant;
  const float mul = A.mul;
  const bool vec = aligned16(su + head) && aligned16(sv + head);
  walk_row(head, chunk, A.R.Wr, [&](auto np, int64_t x) {
    constexpr int NP = decltype(np)::value;
    T u[NP], v[NP];
    load_px(su + x, vec, u);
    load_px(sv + x, vec, v);
    uint32_t id[NP], col[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      id[k] = 0;
      col[k] = flow_colour(widen(u[k]), widen(v[k]), wheel, K, mul, quant);
    }
    emit<NP>(d, x, id, col);
  });
}

// the source and the row geometry, which the two entry points take alike.  false: refused (the message is set)
bool render_rows(const char* fn, RenderArgs& A, const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                 int64_t N, int H, int W, unsigned& grid) {
  A.src = src;
  A.ss_n = ss_n;
  A.ss_c = ss_c;
  A.ss_h = ss_h;
  return check_aligned(fn, src, elem_bytes(src_code), "the source") && row_geometry(fn, N, H, W, ss_h, 1, false, A.R, grid);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_render_argmax_fwd(const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                                       const uint8_t* palette, uint8_t* ids, int64_t di_n, uint8_t* rgb, int64_t dr_n,
                                       int layout, int64_t N, int C, int H, int W, waldo_stream_t stream) {
  const char* fn = "waldo_render_argmax_fwd";
  if (!check_dtype(fn, src_code, false, "the source", "; a packed clip holds its ids") || !check_layout(fn, layout) ||
      !check_shape(fn, N, "C", C, kMaxClasses, H, W))
    return WALDO_EINVAL;
  if (ss_n < 0 || ss_c < 0 || ss_h < 0 || di_n < 0 || dr_n < 0) {
    set_error("%s: negative stride (source n=%lld c=%lld h=%lld, ids n=%lld, rgb n=%lld)", fn, (long long)ss_n,
              (long long)ss_c, (long long)ss_h, (long long)di_n, (long long)dr_n);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!src || (!ids && !rgb) || (rgb && !palette)) {
    set_error("%s: null pointer (src; ids and rgb both; rgb without a palette)", fn);
    return WALDO_EINVAL;
  }
  RenderArgs A{};
  unsigned grid;
  if (!render_rows(fn, A, src, src_code, ss_n, ss_c, ss_h, N, H, W, grid)) return WALDO_EINVAL;
  A.palette = palette;
  A.ids = ids;
  A.di_n = di_n;
  A.rgb = rgb;
  A.dr_n = dr_n;
  A.C = C;
  A.nhwc = layout == WALDO_BYTES_NHWC;
  hipStream_t st = (hipStream_t)stream;
  switch (src_code) {
    case WALDO_DTYPE_F16: render_argmax_kernel<_Float16><<<dim3(grid), dim3(kBlock), 0, st>>>(A); break;
    case WALDO_DTYPE_BF16: render_argmax_kernel<__bf16><<<dim3(grid), dim3(kBlock), 0, st>>>(A); break;
    default: render_argmax_kernel<float><<<dim3(grid), dim3(kBlock), 0, st>>>(A); break;
  }
  return launch_status(fn);
}

template <typename T>
static int launch_flow(const char* fn, const RenderArgs& A, unsigned grid, hipStream_t st) {
  if (A.K <= kWheelLds) render_flow_kernel<T, true><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  else render_flow_kernel<T, false><<<dim3(grid), dim3(kBlock), 0, st>>>(A);
  return launch_status(fn);
}

extern "C" int waldo_render_flow_fwd(const void* flow, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                                     const float* wheel, int K, float mul, uint8_t* rgb, int64_t dr_n, int layout,
                                     int quant, int64_t N, int H, int W, waldo_stream_t stream) {
  const char* fn = "waldo_render_flow_fwd";
  if (!check_dtype(fn, src_code, false, "the flow", "") || !check_layout(fn, layout) || !check_quant(fn, quant))
    return WALDO_EINVAL;
  if (!(mul >= -3.4028234664e38f && mul <= 3.4028234664e38f)) {
    set_error("%s: bad multiplier mul=%g (must be finite)", fn, (double)mul);
    return WALDO_EINVAL;
  }
  if (!check_shape(fn, N, "K", K, kMaxWheel, H, W)) return WALDO_EINVAL;
  if (ss_n < 0 || ss_c < 0 || ss_h < 0 || dr_n < 0) {
    set_error("%s: negative stride (flow n=%lld c=%lld h=%lld, rgb n=%lld)", fn, (long long)ss_n, (long long)ss_c,
              (long long)ss_h, (long long)dr_n);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!flow || !wheel || !rgb) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  RenderArgs A{};
  unsigned grid;
  if (!render_rows(fn, A, flow, src_code, ss_n, ss_c, ss_h, N, H, W, grid)) return WALDO_EINVAL;
  A.wheel = wheel;
  A.K = K;
  A.mul = mul;
  A.quant = quant;
  A.rgb = rgb;
  A.dr_n = dr_n;
  A.nhwc = layout == WALDO_BYTES_NHWC;
  hipStream_t st = (hipStream_t)stream;
  switch (src_code) {
    case WALDO_DTYPE_F16: return launch_flow<_Float16>(fn, A, grid, st);
    case WALDO_DTYPE_BF16: return launch_flow<__bf16>(fn, A, grid, st);
    default: return launch_flow<float>(fn, A, grid, st);
  }
}
