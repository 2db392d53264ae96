// Renders (include/waldo_hip.h "Renders"): the views of the layered decomposition as bytes, made on the device.
//   waldo_render_argmax_fwd   N frames of C planes -> the class id of every pixel (torch.max's index on the CPU) as a
//                             byte, and / or palette[id] as RGB bytes: the reference's Logger.get_lyt
//                             (tools/logger.py:169-179 -> tools/utils.py:202-214) without its trip through the host;
//   waldo_render_flow_fwd     N flows (2, H, W) -> the colour-wheel picture of Logger.get_flow_rgb (tools/logger.py:310-318),
//                             quantised with the library's one quantisation (quantize.hip.h), span (0, 1).
//
// Both are streaming passes laid out as frames_to_bytes.hip (sub-dword stores cost ~12 x a 16-byte store per byte on this
// part): a lane owns 16 consecutive pixels of a ROW (H merged into the row where the source rows are dense), keeps their
// running maxima and ids in registers while it walks the C planes -- kAhead planes' 16-byte loads in flight -- and writes
// 16 ids as one 16-byte store, an interleaved group as three.  Per row:
//   head   the pixels up to the first 16-byte boundary of the row's PRIMARY destination (the id map where there is one,
//          else the RGB bytes; at most 15; any base alignment is accepted): single bytes, one lane each;
//   body   groups of 16 pixels: 16-byte loads where every plane's row is 16-byte aligned at the head's end, element loads
//          otherwise;
//   tail   the last, partial group: 4 pixels per dword store (three dwords interleaved), then single bytes.
// With two destinations (ids AND rgb) or a planar one whose planes are not a multiple of 16 bytes apart, the others may
// sit at another alignment than the primary: every store checks its own address (store_words: 16-byte, else dword, else
// byte stores -- uniform over a row), so any alignment is correct and the aligned case pays one compare.
// The palette lives in LDS as one packed word per class (0x00BBGGRR), filled by the workgroup at entry; the flow wheel
// too while it has at most kWheelLds rows.  No atomics, no workspace, no allocation; the caller's stream.
#include "quantize.hip.h"

namespace waldo {

namespace {

constexpr int kPx = 16;          // pixels of a lane
constexpr int kMaxClasses = 256; // an id fits a byte
constexpr int kWheelLds = 256;   // rows of a flow wheel kept in LDS (a larger one is read from global memory)
constexpr int kMaxWheel = 4096;
typedef uint32_t bytes_u32x4 __attribute__((ext_vector_type(4)));

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
  int64_t Wr;  // pixels of a row (after merging)
  int Hr;      // rows of a frame
  int chunks;  // workgroups of a row
  int C, K, quant;
  float mul;
  bool nhwc;
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// 16 consecutive elements at p; vec: p is 16-byte aligned
template <typename T>
__device__ __forceinline__ void load16(const T* __restrict__ p, bool vec, T (&v)[kPx]) {
  if (vec) {
    constexpr int kQ = (int)sizeof(T) * kPx / 16;
    bytes_u32x4 q[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) q[k] = reinterpret_cast<const bytes_u32x4*>(p)[k];
    __builtin_memcpy(v, q, sizeof(v));
  } else {
#pragma unroll
    for (int k = 0; k < kPx; ++k) v[k] = p[k];
  }
}

// NW words at p, whatever its alignment, with the widest store that alignment allows
template <int NW>
__device__ __forceinline__ void store_words(uint8_t* p, const uint32_t (&w)[NW]) {
  const unsigned a = (unsigned)((uintptr_t)p & 15u);
  if (NW % 4 == 0 && a == 0) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q)
      reinterpret_cast<bytes_u32x4*>(p)[q] = (bytes_u32x4){w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
  } else if ((a & 3u) == 0) {
#pragma unroll
    for (int j = 0; j < NW; ++j) reinterpret_cast<uint32_t*>(p)[j] = w[j];
  } else {
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i) p[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
  }
}

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
#pragma unroll
      for (int j = 0; j < NP / 4; ++j) w[j] = id[4 * j] | (id[4 * j + 1] << 8) | (id[4 * j + 2] << 16) | (id[4 * j + 3] << 24);
      store_words(d.ids + x, w);
    }
    if (d.rgb && d.nhwc) {  // byte i of the group's 3 NP: channel i % 3 of pixel i / 3
      uint32_t w[3 * NP / 4];
#pragma unroll
      for (int j = 0; j < 3 * NP / 4; ++j) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = 4 * j + b;
          word |= ((col[i / 3] >> (8 * (i % 3))) & 255u) << (8 * b);
        }
        w[j] = word;
      }
      store_words(d.rgb + 3 * x, w);
    } else if (d.rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t w[NP / 4];
#pragma unroll
        for (int j = 0; j < NP / 4; ++j) {
          uint32_t word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) word |= ((col[4 * j + b] >> (8 * c)) & 255u) << (8 * b);
          w[j] = word;
        }
        store_words(d.rgb + c * d.plane + x, w);
      }
    }
  }
}

// workgroup -> (frame, row of the frame, chunk of the row); the row's destinations and its head
__device__ __forceinline__ void decode_row(const RenderArgs& A, int64_t& n, int& r, int& chunk, Dest& d, int& head) {
  const unsigned row_id = blockIdx.x / (unsigned)A.chunks;
  chunk = (int)(blockIdx.x - row_id * (unsigned)A.chunks);
  n = row_id / (unsigned)A.Hr;
  r = (int)(row_id - (unsigned)n * (unsigned)A.Hr);
  d.nhwc = A.nhwc;
  d.plane = (int64_t)A.Hr * A.Wr;
  d.ids = A.ids ? A.ids + n * A.di_n + (int64_t)r * A.Wr : nullptr;
  d.rgb = A.rgb ? A.rgb + n * A.dr_n + (int64_t)r * A.Wr * (A.nhwc ? 3 : 1) : nullptr;
  unsigned h;
  if (d.ids || !d.nhwc) h = (16u - (unsigned)((uintptr_t)(d.ids ? d.ids : d.rgb) & 15u)) & 15u;
  // the first pixel whose 3 bytes start a 16-byte line: 3 h = -address (mod 16), 3 * 11 = 1 (mod 16)
  else h = ((16u - (unsigned)((uintptr_t)d.rgb & 15u)) * 11u) & 15u;
  head = (int)min((int64_t)h, A.Wr);
}

// torch.max's index on the CPU: the lowest c among the maxima, NaN above everything and the first NaN kept
__device__ __forceinline__ void take(float v, uint32_t c, float& best, uint32_t& id) {
  if (v > best || (v != v && best == best)) {
    best = v;
    id = c;
  }
}

// one pixel: p at its plane 0
template <typename T>
__device__ __forceinline__ uint32_t argmax_px(const T* __restrict__ p, int64_t ss_c, int C) {
  float best = widen(p[0]);
  uint32_t id = 0;
  for (int c = 1; c < C; ++c) take(widen(p[c * ss_c]), (uint32_t)c, best, id);
  return id;
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
  Dest d;
  decode_row(A, n, r, chunk, d, head);
  const T* __restrict__ s0 = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const int64_t sc = A.ss_c, Wr = A.Wr;
  const int C = A.C;
  if (chunk == 0 && (int)threadIdx.x < head) {
    const uint32_t id[1] = {argmax_px(s0 + threadIdx.x, sc, C)};
    const uint32_t col[1] = {want_rgb ? pal[id[0]] : 0u};
    emit<1>(d, threadIdx.x, id, col);
  }
  const int64_t x = head + ((int64_t)chunk * kBlock + threadIdx.x) * kPx;
  if (x + kPx <= Wr) {
    // every plane's row is 16-byte aligned at the head's end (then at every group: 16 elements are 32 or 64 bytes)
    const bool vec = aligned16(s0 + head) && (C == 1 || ((uint64_t)sc * sizeof(T)) % 16 == 0);
    constexpr int kAhead = sizeof(T) == 4 ? 2 : 4;  // planes in flight: 8 16-byte loads of a lane
    const T* __restrict__ p = s0 + x;
    float best[kPx];
    uint32_t id[kPx];
    {
      T v[kPx];
      load16(p, vec, v);
#pragma unroll
      for (int k = 0; k < kPx; ++k) {
        best[k] = widen(v[k]);
        id[k] = 0;
      }
    }
    int c = 1;
    for (; c + kAhead <= C; c += kAhead) {
      T v[kAhead][kPx];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) load16(p + (c + u) * sc, vec, v[u]);
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
#pragma unroll
        for (int k = 0; k < kPx; ++k) take(widen(v[u][k]), (uint32_t)(c + u), best[k], id[k]);
    }
    for (; c < C; ++c) {
      T v[kPx];
      load16(p + c * sc, vec, v);
#pragma unroll
      for (int k = 0; k < kPx; ++k) take(widen(v[k]), (uint32_t)c, best[k], id[k]);
    }
    uint32_t col[kPx];
#pragma unroll
    for (int k = 0; k < kPx; ++k) col[k] = want_rgb ? pal[id[k]] : 0u;
    emit<kPx>(d, x, id, col);
  } else if (x < Wr) {
    for (int64_t xs = x; xs < Wr; xs += 4) {
      if (xs + 4 <= Wr) {
        uint32_t id[4], col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          id[k] = argmax_px(s0 + xs + k, sc, C);
          col[k] = want_rgb ? pal[id[k]] : 0u;
        }
        emit<4>(d, xs, id, col);
      } else {
        for (int64_t k = xs; k < Wr; ++k) {
          const uint32_t id[1] = {argmax_px(s0 + k, sc, C)};
          const uint32_t col[1] = {want_rgb ? pal[id[0]] : 0u};
          emit<1>(d, k, id, col);
        }
      }
    }
  }
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
  Dest d;
  decode_row(A, n, r, chunk, d, head);
  const T* __restrict__ su = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const T* __restrict__ sv = su + A.ss_c;
  const int64_t Wr = A.Wr;
  const int K = A.K, quant = A.quant;
  const float mul = A.mul;
  const uint32_t none[1] = {0u};
  if (chunk == 0 && (int)threadIdx.x < head) {
    const uint32_t col[1] = {flow_colour(widen(su[threadIdx.x]), widen(sv[threadIdx.x]), wheel, K, mul, quant)};
    emit<1>(d, threadIdx.x, none, col);
  }
  const int64_t x = head + ((int64_t)chunk * kBlock + threadIdx.x) * kPx;
  if (x + kPx <= Wr) {
    const bool vec = aligned16(su + head) && aligned16(sv + head);
    T u[kPx], v[kPx];
    load16(su + x, vec, u);
    load16(sv + x, vec, v);
    uint32_t id[kPx], col[kPx];
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      id[k] = 0;
      col[k] = flow_colour(widen(u[k]), widen(v[k]), wheel, K, mul, quant);
    }
    emit<kPx>(d, x, id, col);
  } else if (x < Wr) {
    for (int64_t xs = x; xs < Wr; xs += 4) {
      if (xs + 4 <= Wr) {
        uint32_t id[4], col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          id[k] = 0;
          col[k] = flow_colour(widen(su[xs + k]), widen(sv[xs + k]), wheel, K, mul, quant);
        }
        emit<4>(d, xs, id, col);
      } else {
        for (int64_t k = xs; k < Wr; ++k) {
          const uint32_t col[1] = {flow_colour(widen(su[k]), widen(sv[k]), wheel, K, mul, quant)};
          emit<1>(d, k, none, col);
        }
      }
    }
  }
}

// what the two entry points check alike; fills the row geometry of A.  false: refused (the message is set)
bool render_geometry(const char* fn, RenderArgs& A, const void* src, int src_code, int64_t ss_n, int64_t ss_c,
                     int64_t ss_h, int64_t N, int H, int W, unsigned& grid) {
  const unsigned elem = src_code == WALDO_DTYPE_F32 ? 4u : 2u;
  if ((uintptr_t)src % elem) {
    set_error("%s: the source is not aligned to its %u-byte elements", fn, elem);
    return false;
  }
  const bool dense_h = H == 1 || ss_h == W;  // (the destinations' frames are dense: H merges into the row)
  A.src = src;
  A.ss_n = ss_n;
  A.ss_c = ss_c;
  A.ss_h = ss_h;
  A.Hr = dense_h ? 1 : H;
  A.Wr = dense_h ? (int64_t)H * W : W;
  const int64_t chunks = (A.Wr + kBlock * kPx - 1) / (kBlock * kPx);
  if (N > 2147483647 / ((int64_t)A.Hr * chunks)) {
    set_error("%s: problem too large for one launch", fn);
    return false;
  }
  A.chunks = (int)chunks;
  grid = (unsigned)(N * A.Hr * chunks);
  return true;
}

bool known_dtype(int code) { return code == WALDO_DTYPE_F32 || code == WALDO_DTYPE_F16 || code == WALDO_DTYPE_BF16; }

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_render_argmax_fwd(const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                                       const uint8_t* palette, uint8_t* ids, int64_t di_n, uint8_t* rgb, int64_t dr_n,
                                       int layout, int64_t N, int C, int H, int W, waldo_stream_t stream) {
  const char* fn = "waldo_render_argmax_fwd";
  if (!known_dtype(src_code)) {
    set_error("%s: unknown dtype %d of the source (WALDO_DTYPE_F32 / _F16 / _BF16; a packed clip holds its ids)", fn,
              src_code);
    return WALDO_EINVAL;
  }
  if (layout != WALDO_BYTES_NCHW && layout != WALDO_BYTES_NHWC) {
    set_error("%s: unknown layout %d (WALDO_BYTES_NCHW / WALDO_BYTES_NHWC)", fn, layout);
    return WALDO_EINVAL;
  }
  if (N < 0 || C < 1 || C > kMaxClasses || H < 1 || W < 1 || H > 32768 || W > 32768) {
    set_error("%s: bad shape N=%lld C=%d H=%d W=%d (1 <= H, W <= 32768, 1 <= C <= 256)", fn, (long long)N, C, H, W);
    return WALDO_EINVAL;
  }
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
  if (!render_geometry(fn, A, src, src_code, ss_n, ss_c, ss_h, N, H, W, grid)) return WALDO_EINVAL;
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
  if (!known_dtype(src_code)) {
    set_error("%s: unknown dtype %d of the flow (WALDO_DTYPE_F32 / _F16 / _BF16)", fn, src_code);
    return WALDO_EINVAL;
  }
  if (layout != WALDO_BYTES_NCHW && layout != WALDO_BYTES_NHWC) {
    set_error("%s: unknown layout %d (WALDO_BYTES_NCHW / WALDO_BYTES_NHWC)", fn, layout);
    return WALDO_EINVAL;
  }
  if (quant != WALDO_METRICS_TRUNC && quant != WALDO_METRICS_ROUND) {
    set_error("%s: unknown quantisation %d (WALDO_METRICS_TRUNC / WALDO_METRICS_ROUND)", fn, quant);
    return WALDO_EINVAL;
  }
  if (!(mul >= -3.4028234664e38f && mul <= 3.4028234664e38f)) {
    set_error("%s: bad multiplier mul=%g (must be finite)", fn, (double)mul);
    return WALDO_EINVAL;
  }
  if (N < 0 || K < 1 || K > kMaxWheel || H < 1 || W < 1 || H > 32768 || W > 32768) {
    set_error("%s: bad shape N=%lld K=%d H=%d W=%d (1 <= H, W <= 32768, 1 <= K <= 4096)", fn, (long long)N, K, H, W);
    return WALDO_EINVAL;
  }
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
  if (!render_geometry(fn, A, flow, src_code, ss_n, ss_c, ss_h, N, H, W, grid)) return WALDO_EINVAL;
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
