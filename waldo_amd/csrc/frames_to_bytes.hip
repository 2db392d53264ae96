// Byte output (include/waldo_hip.h "Byte output"): frames (N, C, H, W) of fp32 / fp16 / bf16 values, or the RGB bytes of
// a packed clip, quantised to uint8 (quantize.hip.h) in the planar (N, C, H, W) or the interleaved (N, H, W, 3) layout.
//
// Rows, head / body / tail and the stores: byte_rows.hip.h.  Pure streaming: 4 (2, 4) bytes read and 1 written per value.
// There is ONE destination and the head aligns it, so a group's store is a 16-byte one whatever the source's alignment.
// A packed source's bytes go through a 256-entry table of quantise(rgb_table[byte]) in LDS (as the scorer's fill_table):
// the byte a pixel had before read_rgb's normalisation is NOT what comes back for 63 of the 256 values under "trunc".
#include "byte_rows.hip.h"
#include "packed_clip.hip.h"
#include "quantize.hip.h"

namespace waldo {

namespace {

struct BytesArgs {
  const void* src;
  int64_t ss_n, ss_c, ss_h;  // in elements (a packed clip: pixels; ss_c unused)
  const float* rgb_table;
  uint8_t* dst;
  int64_t ds_n;
  Rows R;  // rows of a frame: planar C * Hr (1 with C merged), interleaved Hr
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

// planar destination: row r = (c, y); dst row at ((c Hr + y) Wr) of the frame
template <typename T>
__global__ __launch_bounds__(kBlock) void frames_to_bytes_planar_kernel(BytesArgs A) {
  __shared__ uint8_t lut[kRgbTable];
  const Convert<T> conv = make_convert<T>(lut, A);
  int64_t n;
  int r, chunk;
  decode_row(A.R, n, r, chunk);
  const int c = r / A.R.Hr, y = r - c * A.R.Hr;
  const int shift = kPacked<T> ? 8 * c : 0;
  const T* __restrict__ srow =
      static_cast<const T*>(A.src) + n * A.ss_n + (kPacked<T> ? 0 : c * A.ss_c) + (int64_t)y * A.ss_h;
  uint8_t* __restrict__ drow = A.dst + n * A.ds_n + (int64_t)r * A.R.Wr;
  const int head = row_head(drow, false, A.R.Wr);
  const bool vec = aligned16(srow + head);
  walk_row(head, chunk, A.R.Wr, [&](auto np, int64_t x) {
    constexpr int NP = decltype(np)::value;
    T v[NP];
    load_px(srow + x, vec, v);
    if constexpr (NP == 1) {
      drow[x] = (uint8_t)conv(v[0], shift);
    } else {
      uint32_t w[NP / 4];
      pack_planar<NP>(w, [&](int k) { return conv(v[k], shift); });
      store_aligned(drow + x, w);
    }
  });
}

// interleaved destination (C = 3): row r = y; pixel x of the row at byte 3 x of the destination row
template <typename T>
__global__ __launch_bounds__(kBlock) void frames_to_bytes_interleaved_kernel(BytesArgs A) {
  __shared__ uint8_t lut[kRgbTable];
  const Convert<T> conv = make_convert<T>(lut, A);
  int64_t n;
  int r, chunk;
  decode_row(A.R, n, r, chunk);
  const T* __restrict__ s0 = static_cast<const T*>(A.src) + n * A.ss_n + (int64_t)r * A.ss_h;
  const int64_t sc = kPacked<T> ? 0 : A.ss_c;  // (a packed pixel holds the three channels)
  uint8_t* __restrict__ drow = A.dst + n * A.ds_n + (int64_t)r * A.R.Wr * 3;
  const int head = row_head(drow, true, A.R.Wr);
  const bool vec = aligned16(s0 + head) && aligned16(s0 + sc + head) && aligned16(s0 + 2 * sc + head);
  walk_row(head, chunk, A.R.Wr, [&](auto np, int64_t x) {
    constexpr int NP = decltype(np)::value;
    uint32_t b[3][NP];
    if constexpr (kPacked<T>) {
      T v[NP];
      load_px(s0 + x, vec, v);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < NP; ++k) b[c][k] = conv(v[k], 8 * c);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        T v[NP];
        load_px(s0 + c * sc + x, vec, v);
#pragma unroll
        for (int k = 0; k < NP; ++k) b[c][k] = conv(v[k], 0);
      }
    }
    if constexpr (NP == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) drow[3 * x + c] = (uint8_t)b[c][0];
    } else {
      uint32_t w[3 * NP / 4];
      pack_interleaved<NP>(w, [&](int c, int k) { return b[c][k]; });
      store_aligned(drow + 3 * x, w);
    }
  });
}

template <typename T>
int launch_bytes(const char* fn, const BytesArgs& A, unsigned blocks, int layout, hipStream_t st) {
  const dim3 grid(blocks);
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
  if (!check_dtype(fn, src_code, true, "the source", ", WALDO_BYTES_SRC_PACKED") || !check_layout(fn, layout) ||
      !check_quant(fn, quant) || !check_span(fn, lo, range) || !check_shape(fn, N, "C", C, 4096, H, W))
    return WALDO_EINVAL;
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
  if (!check_aligned(fn, src, elem_bytes(src_code), "the source")) return WALDO_EINVAL;
  BytesArgs A{};
  unsigned grid;
  // (C merges into the row too where its planes are contiguous in the source and the destination)
  const bool merge_c = !packed && layout == WALDO_BYTES_NCHW && (C == 1 || ss_c == (int64_t)H * W);
  if (!row_geometry(fn, N, H, W, ss_h, layout == WALDO_BYTES_NHWC ? 1 : C, merge_c, A.R, grid)) return WALDO_EINVAL;
  A.src = src;
  A.ss_n = ss_n;
  A.ss_c = ss_c;
  A.ss_h = ss_h;
  A.rgb_table = rgb_table;
  A.dst = dst;
  A.ds_n = ds_n;
  A.quant = quant;
  A.lo = lo;
  A.range = range;
  hipStream_t st = (hipStream_t)stream;
  switch (src_code) {
    case WALDO_DTYPE_F16: return launch_bytes<_Float16>(fn, A, grid, layout, st);
    case WALDO_DTYPE_BF16: return launch_bytes<__bf16>(fn, A, grid, layout, st);
    case WALDO_BYTES_SRC_PACKED: return launch_bytes<uint32_t>(fn, A, grid, layout, st);
    default: return launch_bytes<float>(fn, A, grid, layout, st);
  }
}
