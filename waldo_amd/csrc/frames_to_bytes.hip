// Byte output (include/waldo_hip.h "Byte output"): frames (N, C, H, W) of fp32 / fp16 / bf16 values, or the RGB bytes of
// a packed clip, quantised to uint8 (quantize.hip.h) in the planar (N, C, H, W) or the interleaved (N, H, W, 3) layout.
//
// Pure streaming: 4 (2, 4) bytes read and 1 written per value.  Sub-dword stores cost ~12 x a 16-byte store per byte on
// this part, so a lane owns 16 consecutive pixels of a ROW and writes them as one 16-byte store (three for an interleaved
// group of 48 bytes).  A row is whatever is contiguous in both the source and the destination: the launcher merges H
// into the row when the source rows are dense, and C too when its planes are (a frame is then ONE row).  Per row:
//   head   the pixels up to the first 16-byte boundary of the DESTINATION (at most 15; any base alignment is accepted):
//          single bytes, one lane each;
//   body   groups of 16 pixels: 16-byte loads where the source is 16-byte aligned at the head's end, element loads
//          otherwise -- the store is a 16-byte one either way;
//   tail   the last, partial group: 4 pixels per dword store (three dwords interleaved), then single bytes.
// A packed source's bytes go through a 256-entry table of quantise(rgb_table[byte]) in LDS (as the scorer's fill_table):
// the byte a pixel had before read_rgb's normalisation is NOT what comes back for 63 of the 256 values under "trunc".
#include "packed_clip.hip.h"
#include "quantize.hip.h"

namespace waldo {

namespace {

constexpr int kPx = 16;  // pixels of a lane
typedef uint32_t bytes_u32x4 __attribute__((ext_vector_type(4)));

struct BytesArgs {
  const void* src;
  int64_t ss_n, ss_c, ss_h;  // in elements (a packed clip: pixels; ss_c unused)
  const float* rgb_table;
  uint8_t* dst;
  int64_t ds_n;
  int64_t Wr;  // pixels of a row (after merging)
  int rows;    // rows of a frame: planar C * Hr, interleaved Hr
  int Hr;      // rows of a plane
  int chunks;  // workgroups of a row
  int quant;
  float lo, range;
};

template <typename T>
constexpr bool kPacked = std::is_same<T, uint32_t>::value;

template <typename T>
struct Convert {
  const uint8_t* lut;
  float lo, range;
  int quant;
  __device__ __forceinline__ uint32_t operator()(T v, int shift) const {
    if constexpr (kPacked<T>) return lut[(v >> shift) & 255u];
    else return quant_byte(widen(v), lo, range, quant);
  }
};

// the table of a packed source (every thread of the workgroup calls this)
template <typename T>
__device__ __forceinline__ Convert<T> make_convert(uint8_t* lut, const BytesArgs& A) {
  if constexpr (kPacked<T>) {
    static_assert(kBlock == kRgbTable, "one table entry per thread");
    lut[threadIdx.x] = (uint8_t)quant_byte(A.rgb_table[threadIdx.x], A.lo, A.range, A.quant);
    __syncthreads();
  }
  return Convert<T>{lut, A.lo, A.range, A.quant};
}

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

__device__ __forceinline__ uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// workgroup -> (frame, row of the frame, chunk of the row)
__device__ __forceinline__ void decode_row(const BytesArgs& A, int64_t& n, int& r, int& chunk) {
  const unsigned row_id = blockIdx.x / (unsigned)A.chunks;
  chunk = (int)(blockIdx.x - row_id * (unsigned)A.chunks);
  n = row_id / (unsigned)A.rows;
  r = (int)(row_id - (unsigned)n * (unsigned)A.rows);
}

// planar destination: row r = (c, y); dst row at ((c Hr + y) Wr) of the frame
template <typename T>
__global__ __launch_bounds__(kBlock) void frames_to_bytes_planar_kernel(BytesArgs A) {
  __shared__ uint8_t lut[kRgbTable];
  const Convert<T> conv = make_convert<T>(lut, A);
  int64_t n;
  int r, chunk;
  decode_row(A, n, r, chunk);
  const int c = r / A.Hr, y = r - c * A.Hr;
  const int shift = kPacked<T> ? 8 * c : 0;
  const T* __restrict__ srow =
      static_cast<const T*>(A.src) + n * A.ss_n + (kPacked<T> ? 0 : c * A.ss_c) + (int64_t)y * A.ss_h;
  uint8_t* __restrict__ drow = A.dst + n * A.ds_n + (int64_t)r * A.Wr;
  const int64_t Wr = A.Wr;
  const int head = (int)min((int64_t)((16u - ((uintptr_t)drow & 15u)) & 15u), Wr);
  if (chunk == 0 && (int)threadIdx.x < head) drow[threadIdx.x] = (uint8_t)conv(srow[threadIdx.x], shift);
  const int64_t x = head + ((int64_t)chunk * kBlock + threadIdx.x) * kPx;
  if (x + kPx <= Wr) {
    T v[kPx];
    load16(srow + x, aligned16(srow + head), v);
    bytes_u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = pack4(conv(v[4 * j], shift), conv(v[4 * j + 1], shift), conv(v[4 * j + 2], shift),
                   conv(v[4 * j + 3], shift));
    *reinterpret_cast<bytes_u32x4*>(drow + x) = w;
  } else if (x < Wr) {
    for (int64_t xs = x; xs < Wr; xs += 4) {
      if (xs + 4 <= Wr) {
        *reinterpret_cast<uint32_t*>(drow + xs) = pack4(conv(srow[xs], shift), conv(srow[xs + 1], shift),
                                                        conv(srow[xs + 2], shift), conv(srow[xs + 3], shift));
      } else {
        for (int64_t k = xs; k < Wr; ++k) drow[k] = (uint8_t)conv(srow[k], shift);
      }
    }
  }
}

// interleaved destination (C = 3): row r = y; pixel x of the row at byte 3 x of the destination row
template <typename T>
__global__ __launch_bounds__(kBlock) void frames_to_bytes_interleaved_kernel(BytesArgs A) {
  __shared__ uint8_t lut[kRgbTable];
  const Convert<T> conv = make_convert<T>(lut, A);
  int64_t n;
  int r, chunk;
  decode_row(A, n, r, chunk);
  const T* __restrict__ s0 = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const int64_t sc = kPacked<T> ? 0 : A.ss_c;  // (a packed pixel holds the three channels)
  uint8_t* __restrict__ drow = A.dst + n * A.ds_n + (int64_t)r * A.Wr * 3;
  const int64_t Wr = A.Wr;
  // the first pixel whose 3 bytes start a 16-byte line: 3 h = -address (mod 16), 3 * 11 = 1 (mod 16)
  const int head = (int)min((int64_t)(((16u - ((uintptr_t)drow & 15u)) * 11u) & 15u), Wr);
  if (chunk == 0 && (int)threadIdx.x < head) {
#pragma unroll
    for (int c = 0; c < 3; ++c) drow[3 * threadIdx.x + c] = (uint8_t)conv(s0[c * sc + threadIdx.x], 8 * c);
  }
  const int64_t x = head + ((int64_t)chunk * kBlock + threadIdx.x) * kPx;
  if (x + kPx <= Wr) {
    uint32_t b[3][kPx];
    if constexpr (kPacked<T>) {
      T v[kPx];
      load16(s0 + x, aligned16(s0 + head), v);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < kPx; ++k) b[c][k] = conv(v[k], 8 * c);
    } else {
      const bool vec = aligned16(s0 + head) && aligned16(s0 + sc + head) && aligned16(s0 + 2 * sc + head);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        T v[kPx];
        load16(s0 + c * sc + x, vec, v);
#pragma unroll
        for (int k = 0; k < kPx; ++k) b[c][k] = conv(v[k], 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {  // bytes 16 q .. 16 q + 15 of the group's 48: byte i is channel i % 3 of pixel i / 3
      bytes_u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 16 * q + 4 * j;
        w[j] = pack4(b[i % 3][i / 3], b[(i + 1) % 3][(i + 1) / 3], b[(i + 2) % 3][(i + 2) / 3],
                     b[(i + 3) % 3][(i + 3) / 3]);
      }
      *reinterpret_cast<bytes_u32x4*>(drow + 3 * x + 16 * q) = w;
    }
  } else if (x < Wr) {
    for (int64_t xs = x; xs < Wr; xs += 4) {
      if (xs + 4 <= Wr) {
        uint32_t p[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) p[3 * k + c] = conv(s0[c * sc + xs + k], 8 * c);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          reinterpret_cast<uint32_t*>(drow + 3 * xs)[j] = pack4(p[4 * j], p[4 * j + 1], p[4 * j + 2], p[4 * j + 3]);
      } else {
        for (int64_t k = xs; k < Wr; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) drow[3 * k + c] = (uint8_t)conv(s0[c * sc + k], 8 * c);
      }
    }
  }
}

template <typename T>
int launch_bytes(const char* fn, const BytesArgs& A, int64_t N, int layout, hipStream_t st) {
  const dim3 grid((unsigned)(N * A.rows * A.chunks));
  if (layout == WALDO_BYTES_NHWC) frames_to_bytes_interleaved_kernel<T><<<grid, dim3(kBlock), 0, st>>>(A);
  else frames_to_bytes_planar_kernel<T><<<grid, dim3(kBlock), 0, st>>>(A);
  return launch_status(fn);
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_frames_to_bytes_fwd(const void* src, int src_code, int64_t ss_n, int64_t ss_c, int64_t ss_h,
                                         const float* rgb_table, uint8_t* dst, int64_t ds_n, int layout, int64_t N,
                                         int C, int H, int W, float lo, float range, int quant,
                                         waldo_stream_t stream) {
  const char* fn = "waldo_frames_to_bytes_fwd";
  const bool packed = src_code == WALDO_BYTES_SRC_PACKED;
  if (src_code != WALDO_DTYPE_F32 && src_code != WALDO_DTYPE_F16 && src_code != WALDO_DTYPE_BF16 && !packed) {
    set_error("%s: unknown dtype %d of the source (WALDO_DTYPE_F32 / _F16 / _BF16, WALDO_BYTES_SRC_PACKED)", fn,
              src_code);
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
  if (!(range > 0.0f) || !(range <= 3.4028234664e38f) || !(lo >= -3.4028234664e38f && lo <= 3.4028234664e38f)) {
    set_error("%s: bad span lo=%g range=%g (range = hi - lo must be positive and finite)", fn, (double)lo,
              (double)range);
    return WALDO_EINVAL;
  }
  if (N < 0 || C < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || C > 4096) {
    set_error("%s: bad shape N=%lld C=%d H=%d W=%d (1 <= H, W <= 32768, 1 <= C <= 4096)", fn, (long long)N, C, H, W);
    return WALDO_EINVAL;
  }
  if (ss_n < 0 || ss_c < 0 || ss_h < 0 || ds_n < 0) {
    set_error("%s: negative stride (source n=%lld c=%lld h=%lld, destination n=%lld)", fn, (long long)ss_n,
              (long long)ss_c, (long long)ss_h, (long long)ds_n);
    return WALDO_EINVAL;
  }
  if ((layout == WALDO_BYTES_NHWC || packed) && C != 3) {
    set_error("%s: C=%d: the interleaved layout and a packed source have 3 channels", fn, C);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!src || !dst || (packed && !rgb_table)) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const unsigned elem = src_code == WALDO_DTYPE_F16 || src_code == WALDO_DTYPE_BF16 ? 2u : 4u;
  if ((uintptr_t)src % elem) {
    set_error("%s: the source is not aligned to its %u-byte elements", fn, elem);
    return WALDO_EINVAL;
  }
  // rows: what is contiguous in the source and in the destination
  const bool dense_h = H == 1 || ss_h == W;
  const bool dense_c = dense_h && !packed && layout == WALDO_BYTES_NCHW && (C == 1 || ss_c == (int64_t)H * W);
  BytesArgs A{};
  A.src = src;
  A.ss_n = ss_n;
  A.ss_c = ss_c;
  A.ss_h = ss_h;
  A.rgb_table = rgb_table;
  A.dst = dst;
  A.ds_n = ds_n;
  A.Hr = dense_h ? 1 : H;
  A.Wr = dense_h ? (int64_t)H * W : W;
  A.rows = layout == WALDO_BYTES_NHWC ? A.Hr : C * A.Hr;
  if (dense_c) {
    A.Wr *= C;
    A.rows = 1;
  }
  const int64_t chunks = (A.Wr + kBlock * kPx - 1) / (kBlock * kPx);
  if (chunks > 2147483647 || N > 2147483647 / ((int64_t)A.rows * chunks)) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  A.chunks = (int)chunks;
  A.quant = quant;
  A.lo = lo;
  A.range = range;
  hipStream_t st = (hipStream_t)stream;
  switch (src_code) {
    case WALDO_DTYPE_F16: return launch_bytes<_Float16>(fn, A, N, layout, st);
    case WALDO_DTYPE_BF16: return launch_bytes<__bf16>(fn, A, N, layout, st);
    case WALDO_BYTES_SRC_PACKED: return launch_bytes<uint32_t>(fn, A, N, layout, st);
    default: return launch_bytes<float>(fn, A, N, layout, st);
  }
}
