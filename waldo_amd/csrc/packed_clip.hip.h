// The packed clip (waldo_amd.functional.PackedClip, include/waldo_hip.h "Packed clip"): (B, T, Hd, Wd) pixels of ONE
// 4-byte word each, bytes [R, G, B, class id] -- 4 bytes for what the clip's fp32 form spreads over 3 + Nl floats.
// Its UNPACKED form, which every packed kernel reproduces bit for bit:
//   channel c < 3:   rgb_table[byte c]   (256 fp32 values: read_rgb's (u8 / 255 - 0.5) / 0.5, built by the caller)
//   channel 3 + n:   +5 where the class id == n, -5 elsewhere (io.read_layout's 5 (2 onehot - 1); an id >= Nl: -5 in
//                    every layout channel)
// The kernels read the word and expand the channel they need; the arithmetic that follows is the fp32 kernels' own.
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

constexpr float kLytLogit = 5.0f;  // io.read_layout: 5 * (onehot * 2 - 1)
constexpr int kRgbTable = 256;
constexpr int kMaxPackedCls = 32;  // layout classes of a packed clip: the fused path's limit (flow_ctx_common.hip.h: kMaxCls)

__device__ __forceinline__ int packed_class(uint32_t w) { return (int)(w >> 24); }

// layout channel 3 + n of a pixel
__device__ __forceinline__ float packed_lyt(uint32_t w, int n) { return packed_class(w) == n ? kLytLogit : -kLytLogit; }

// channel c of the unpacked form of a pixel, the RGB table at `table` (global memory or LDS)
__device__ __forceinline__ float packed_channel(const float* table, uint32_t w, int c) {
  return c < 3 ? table[(w >> (8 * c)) & 255u] : packed_lyt(w, c - 3);
}

}  // namespace waldo
