// The row scheme of the kernels that write uint8 results (frames_to_bytes.hip, render.hip; wif_fuse.hip takes the
// packers and the argument checks), written once.
//
// These are streaming passes, and sub-dword stores cost ~12 x a 16-byte store per byte on this part.  So a lane owns 16
// consecutive pixels of a ROW and writes them as one 16-byte store (three for an interleaved group of 48 bytes).  A row
// is whatever is contiguous in both the source and the destination: the launcher merges H into the row when the source
// rows are dense, and where the caller allows it C too when its planes are (a frame is then ONE row).  Per row:
//   head   the pixels up to the first 16-byte boundary of the row's DESTINATION (at most 15; any base alignment is
//          accepted): single bytes, one lane each;
//   body   groups of 16 pixels: 16-byte loads where the source is 16-byte aligned at the head's end, element loads
//          otherwise -- the store is as wide either way;
//   tail   the last, partial group: 4 pixels per dword store (three dwords interleaved), then single bytes.
// A kernel is its set-up (tables in LDS, the row's pointers, the head) and one callable handed to walk_row, which
// produces NP = 1, 4 or 16 pixels from pixel x of the row on and stores them.
#pragma once
#include <type_traits>

#include "quantize.hip.h"

namespace waldo {

constexpr int kPx = 16;  // pixels of a lane
typedef uint32_t bytes_u32x4 __attribute__((ext_vector_type(4)));

// ---- primitives -----------------------------------------------------------------------------------------------------
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

// NP consecutive elements at p: a lane's group through load16, the head's and the tail's pixels one by one
template <int NP, typename T>
__device__ __forceinline__ void load_px(const T* __restrict__ p, bool vec, T (&v)[NP]) {
  if constexpr (NP == kPx) {
    load16(p, vec, v);
  } else {
#pragma unroll
    for (int k = 0; k < NP; ++k) v[k] = p[k];
  }
}

__device__ __forceinline__ uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// NP bytes of one plane as NP / 4 words: byte(k) is pixel k's, 0 .. 255
template <int NP, typename B>
__device__ __forceinline__ void pack_planar(uint32_t (&w)[NP / 4], B&& byte) {
#pragma unroll
  for (int j = 0; j < NP / 4; ++j) w[j] = pack4(byte(4 * j), byte(4 * j + 1), byte(4 * j + 2), byte(4 * j + 3));
}

// three channels of NP pixels interleaved as 3 NP / 4 words: byte i of the 3 NP is byte(i % 3, i / 3), channel i % 3 of
// pixel i / 3
template <int NP, typename B>
__device__ __forceinline__ void pack_interleaved(uint32_t (&w)[3 * NP / 4], B&& byte) {
#pragma unroll
  for (int j = 0; j < 3 * NP / 4; ++j) {
    const int i = 4 * j;
    w[j] = pack4(byte(i % 3, i / 3), byte((i + 1) % 3, (i + 1) / 3), byte((i + 2) % 3, (i + 2) / 3),
                 byte((i + 3) % 3, (i + 3) / 3));
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

// NW words at the ONE destination the head aligned: 16-byte stores for a lane's group (NW % 4 == 0), dword stores for
// the tail's -- no test of the address
template <int NW>
__device__ __forceinline__ void store_aligned(uint8_t* p, const uint32_t (&w)[NW]) {
  if constexpr (NW % 4 == 0) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q)
      reinterpret_cast<bytes_u32x4*>(p)[q] = (bytes_u32x4){w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
  } else {
#pragma unroll
    for (int j = 0; j < NW; ++j) reinterpret_cast<uint32_t*>(p)[j] = w[j];
  }
}

// ---- rows -----------------------------------------------------------------------------------------------------------
struct Rows {
  int64_t Wr;  // pixels of a row (after merging)
  int Hr;      // rows of a plane
  int rows;    // rows of a frame: per_frame * Hr, or 1 with C merged
  int chunks;  // workgroups of a row
};

// (N, H, W, ss_h) -> the rows and the grid.  H merges into the row where the source rows are dense (the destinations'
// frames are); per_frame: rows of a frame per row of a plane (C for a planar destination written plane by plane, else
// 1); merge_c: the per_frame planes are dense in the source and the destination, and merge too where H does.
// false: refused (the message is set)
inline bool row_geometry(const char* fn, int64_t N, int H, int W, int64_t ss_h, int per_frame, bool merge_c, Rows& R,
                         unsigned& grid) {
  const bool dense_h = H == 1 || ss_h == W;
  R.Hr = dense_h ? 1 : H;
  R.Wr = dense_h ? (int64_t)H * W : W;
  R.rows = per_frame * R.Hr;
  if (dense_h && merge_c) {
    R.Wr *= per_frame;
    R.rows = 1;
  }
  const int64_t chunks = (R.Wr + kBlock * kPx - 1) / (kBlock * kPx);
  if (chunks > 2147483647 || N > 2147483647 / ((int64_t)R.rows * chunks)) {
    set_error("%s: problem too large for one launch", fn);
    return false;
  }
  R.chunks = (int)chunks;
  grid = (unsigned)(N * R.rows * chunks);
  return true;
}

// workgroup -> (frame, row of the frame, chunk of the row)
__device__ __forceinline__ void decode_row(const Rows& R, int64_t& n, int& r, int& chunk) {
  const unsigned row_id = blockIdx.x / (unsigned)R.chunks;
  chunk = (int)(blockIdx.x - row_id * (unsigned)R.chunks);
  n = row_id / (unsigned)R.rows;
  r = (int)(row_id - (unsigned)n * (unsigned)R.rows);
}

// the head of a row whose (primary) destination starts at d: one byte per pixel, or three interleaved
__device__ __forceinline__ int row_head(const uint8_t* d, bool interleaved, int64_t Wr) {
  unsigned h = 16u - (unsigned)((uintptr_t)d & 15u);
  // the first pixel whose 3 bytes start a 16-byte line: 3 h = -address (mod 16), 3 * 11 = 1 (mod 16)
  if (interleaved) h *= 11u;
  return (int)min((int64_t)(h & 15u), Wr);
}

// f(std::integral_constant<int, NP>{}, x): NP pixels from pixel x of the row on.  NP = 1 for the head's pixels (one lane
// each, in the row's first workgroup) and the tail's last odd ones, 16 for a lane's full group, 4 for the tail's dwords.
template <typename F>
__device__ __forceinline__ void walk_row(int head, int chunk, int64_t Wr, F&& f) {
  if (chunk == 0 && (int)threadIdx.x < head) f(std::integral_constant<int, 1>{}, (int64_t)threadIdx.x);
  const int64_t x = head + ((int64_t)chunk * kBlock + threadIdx.x) * kPx;
  if (x + kPx <= Wr) {
    f(std::integral_constant<int, kPx>{}, x);
  } else if (x < Wr) {
    for (int64_t xs = x; xs < Wr; xs += 4) {
      if (xs + 4 <= Wr) {
        f(std::integral_constant<int, 4>{}, xs);
      } else {
        for (int64_t k = xs; k < Wr; ++k) f(std::integral_constant<int, 1>{}, k);
      }
    }
  }
}

// ---- argument checks of the entry points: true, or false with the message set -------------------------------------------
inline bool known_dtype(int code) {
  return code == WALDO_DTYPE_F32 || code == WALDO_DTYPE_F16 || code == WALDO_DTYPE_BF16;
}

inline unsigned elem_bytes(int code) { return code == WALDO_DTYPE_F16 || code == WALDO_DTYPE_BF16 ? 2u : 4u; }

// what: "the source"; also: what else the entry point takes or says, appended inside the parentheses
inline bool check_dtype(const char* fn, int code, bool packed_ok, const char* what, const char* also) {
  if (known_dtype(code) || (packed_ok && code == WALDO_BYTES_SRC_PACKED)) return true;
  set_error("%s: unknown dtype %d of %s (WALDO_DTYPE_F32 / _F16 / _BF16%s)", fn, code, what, also);
  return false;
}

inline bool check_layout(const char* fn, int layout) {
  if (layout == WALDO_BYTES_NCHW || layout == WALDO_BYTES_NHWC) return true;
  set_error("%s: unknown layout %d (WALDO_BYTES_NCHW / WALDO_BYTES_NHWC)", fn, layout);
  return false;
}

inline bool check_quant(const char* fn, int quant) {
  if (quant == WALDO_METRICS_TRUNC || quant == WALDO_METRICS_ROUND) return true;
  set_error("%s: unknown quantisation %d (WALDO_METRICS_TRUNC / WALDO_METRICS_ROUND)", fn, quant);
  return false;
}

inline bool check_span(const char* fn, float lo, float range) {
  if (range > 0.0f && range <= 3.4028234664e38f && lo >= -3.4028234664e38f && lo <= 3.4028234664e38f) return true;
  set_error("%s: bad span lo=%g range=%g (range = hi - lo must be positive and finite)", fn, (double)lo, (double)range);
  return false;
}

// cname / c / cmax: the third extent, by its name ("C", "K")
inline bool check_shape(const char* fn, int64_t N, const char* cname, int c, int cmax, int H, int W) {
  if (N >= 0 && c >= 1 && c <= cmax && H >= 1 && W >= 1 && H <= 32768 && W <= 32768) return true;
  set_error("%s: bad shape N=%lld %s=%d H=%d W=%d (1 <= H, W <= 32768, 1 <= %s <= %d)", fn, (long long)N, cname, c, H,
            W, cname, cmax);
  return false;
}

inline bool check_aligned(const char* fn, const void* p, unsigned elem, const char* what) {
  if ((uintptr_t)p % elem == 0) return true;
  set_error("%s: %s is not aligned to its %u-byte elements", fn, what, elem);
  return false;
}

}  // namespace waldo
