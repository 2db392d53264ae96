// The library's ONE quantisation of a value to a byte (include/waldo_hip.h "Byte output"), shared by the scorer
// (frame_metrics.hip: the byte / 255 it scores) and the byte outputs (frames_to_bytes.hip, wif_fuse.hip):
//   u = clamp((x - lo) / range, 0, 1)                      fp32, IEEE division (-ffp-contract=off -fno-fast-math)
//   "trunc": level = truncf(u * 255)                       the reference's dump_video (tools/utils.py:246-264)
//   "round": level = truncf(u * 255 + 0.5)                 tools.io.dump_video / dump_image
// The clamp is fminf(fmaxf(u, 0), 1): fmaxf returns its other operand for a NaN, so NaN -> 0; -inf -> 0, +inf -> 255.
#pragma once
#include "waldo_common.hip.h"

namespace waldo {

__device__ __forceinline__ float quant_unit(float x, float lo, float range) {
  float u = (x - lo) / range;
  return fminf(fmaxf(u, 0.0f), 1.0f);
}

// the byte's value, 0 .. 255, still as a float
__device__ __forceinline__ float quant_level_trunc(float u) { return truncf(u * 255.0f); }
__device__ __forceinline__ float quant_level_round(float u) { return truncf(u * 255.0f + 0.5f); }

// quant: WALDO_METRICS_TRUNC or WALDO_METRICS_ROUND (the launchers refuse anything else)
__device__ __forceinline__ uint32_t quant_byte(float x, float lo, float range, int quant) {
  const float u = quant_unit(x, lo, range);
  return (uint32_t)(quant == WALDO_METRICS_ROUND ? quant_level_round(u) : quant_level_trunc(u));
}

// a 16-bit element widened exactly; a packed clip's word stays a word (its consumer looks the byte up)
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float widen(__bf16 v) { return (float)v; }

}  // namespace waldo
