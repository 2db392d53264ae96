// f3: the border objects of WIF.inpaint (models/nets/wif.py:134-157) for a batch of clips, chosen on the device.
// The reference handles ONE clip and steers with host reads -- `hit.sum() > 0`, `int(argmax)`, six `float()` of corner
// extrema per side, each of which stops the stream.  Here, per clip b and side s (0 = left, 1 = right border):
//
//     pred_px = to_px(pred_flow[b, -1, -1] + ident),  orig_px = to_px(ident),  to_px(g) = ((g.x W + W - 1) / 2, (g.y H + H - 1) / 2)
//     at      = pred_px.x < 3 | pred_px.x >= W - 3
//     obj[o]  = max_tc (alpha_ctx[b, tc, -1, 1 + o] + 1) / 2 > 0.9                       (torch.max: a NaN wins)
//     count[o] = #{at & obj[o]};  valid = any count > 0;  obj_id = first o of the largest count (torch.argmax)
//     by0, by1, ox0, ox1, oy0, oy1 = min / max of pred_px.y, orig_px.x, orig_px.y over at & obj[obj_id]
//
// in four small launches: init (the workspace), count, extrema (every workgroup re-derives obj_id from the finished
// counts), finalize (valid, obj_id and the corners, as float64).  The pixel arithmetic is taken in the order of the
// framework's elementwise kernels (the library is built with -ffp-contract=off): the `at` tests and the extrema have
// the bits of the torch expressions.  Counts are integer atomics; the extrema are integer atomic min / max on
// order-preserving keys of the fp32 values, a NaN is recorded in a flag word and propagates as in torch.min / torch.max:
// nothing depends on the order of arrival.  alpha_ctx is only read where a pixel is at a border.
#include "waldo_common.hip.h"

namespace waldo {

constexpr int kMaxObj = 32;        // object slots per (clip, side) in the workspace (L - 1 <= 31 are used)
constexpr int kExtWords = 8;       // by0 by1 ox0 ox1 oy0 oy1, the NaN flags, one spare
constexpr int kSideWords = kMaxObj + kExtWords;
constexpr float kBorder = 3.0f;    // `border = 3` pixels of wif.py:134
constexpr float kObjThresh = 0.9f; // wif.py:137, as the float32 scalar the comparison is made with

struct BorderCtx {
  int64_t b, tc, tp, l;  // element strides of alpha_ctx (B, Tc, Tp, L, H, W); the (H, W) planes are contiguous
};

// order-preserving key of a non-NaN float: a < b  <=>  key(a) < key(b) as unsigned (-0 sorts below +0)
__device__ __forceinline__ unsigned ordered_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float to_px(float g, float size) {  // (g * size + size - 1) / 2, left to right
  return (((g * size) + size) - 1.0f) / 2.0f;
}

// obj[o] of one pixel: the maximum over the contexts of (alpha + 1) / 2, a NaN winning, above 0.9
__device__ __forceinline__ bool object_here(const float* __restrict__ a, int Tc, int64_t stride_tc) {
  float m = 0.0f;
  for (int tc = 0; tc < Tc; ++tc) {
    const float h = (a[tc * stride_tc] + 1.0f) / 2.0f;
    m = (tc == 0 || h > m || h != h) ? h : m;
  }
  return m > kObjThresh;
}

// first index of the largest count (torch.argmax); valid = the largest count is not zero
__device__ __forceinline__ int pick_object(const unsigned* __restrict__ cnt, int No, bool& valid) {
  unsigned best = 0;
  int id = 0;
  for (int o = 0; o < No; ++o) {
    const unsigned c = cnt[o];
    if (c > best) {
      best = c;
      id = o;
    }
  }
  valid = best > 0;
  return id;
}

__global__ __launch_bounds__(kBlock) void border_init_kernel(unsigned* __restrict__ ws, int64_t sides) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= sides * kSideWords) return;
  const int w = (int)(i % kSideWords);
  // counts 0; minima start at the largest key, maxima at the smallest; flags 0
  const bool is_min = w >= kMaxObj && w < kMaxObj + 6 && ((w - kMaxObj) & 1) == 0;
  ws[i] = is_min ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(kBlock) void border_count_kernel(const float* __restrict__ flow, int64_t flow_stride_b,
                                                              const float* __restrict__ ident,
                                                              const float* __restrict__ actx, BorderCtx st,
                                                              unsigned* __restrict__ ws, int Tc, int Tp, int L, int H,
                                                              int W, int tiles) {
  __shared__ unsigned cnt[2][kMaxObj];
  const int64_t b = blockIdx.x / tiles;
  const int64_t HW = (int64_t)H * W;
  const int64_t p = (int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x;
  if (threadIdx.x < 2 * kMaxObj) cnt[threadIdx.x / kMaxObj][threadIdx.x % kMaxObj] = 0u;
  bool left = false, right = false;
  if (p < HW) {
    const float px = to_px(flow[b * flow_stride_b + p] + ident[2 * p], (float)W);
    left = px < kBorder;
    right = px >= (float)(W - 3);
  }
  if (!__syncthreads_or(left || right)) return;  // (uniform; also orders the zeroed counters)
  if (left || right) {
    const float* base = actx + b * st.b + (int64_t)(Tp - 1) * st.tp + p;
    for (int o = 0; o < L - 1; ++o) {
      if (object_here(base + (int64_t)(o + 1) * st.l, Tc, st.tc)) {
        if (left) atomicAdd(&cnt[0][o], 1u);
        if (right) atomicAdd(&cnt[1][o], 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * kMaxObj) {
    const int s = threadIdx.x / kMaxObj, o = threadIdx.x % kMaxObj;
    const unsigned c = cnt[s][o];
    if (c) atomicAdd(ws + (b * 2 + s) * kSideWords + o, c);
  }
}

__global__ __launch_bounds__(kBlock) void border_extrema_kernel(const float* __restrict__ flow, int64_t flow_stride_b,
                                                                int64_t flow_stride_c, const float* __restrict__ ident,
                                                                const float* __restrict__ actx, BorderCtx st,
                                                                unsigned* __restrict__ ws, int Tc, int Tp, int L, int H,
                                                                int W, int tiles) {
  __shared__ unsigned ext[2][kExtWords];
  __shared__ int pick[2];  // obj_id of the side, -1 where no object is at that border
  const int64_t b = blockIdx.x / tiles;
  const int64_t HW = (int64_t)H * W;
  const int64_t p = (int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x;
  if (threadIdx.x < 2 * kExtWords) {
    const int w = threadIdx.x % kExtWords;
    ext[threadIdx.x / kExtWords][w] = (w < 6 && (w & 1) == 0) ? 0xffffffffu : 0u;
  }
  if (threadIdx.x >= kWave && threadIdx.x < kWave + 2) {
    const int s = threadIdx.x - kWave;
    bool valid;
    const int id = pick_object(ws + (b * 2 + s) * kSideWords, L - 1, valid);
    pick[s] = valid ? id : -1;
  }
  bool left = false, right = false;
  float idx = 0.0f;
  if (p < HW) {
    idx = ident[2 * p];
    const float px = to_px(flow[b * flow_stride_b + p] + idx, (float)W);
    left = px < kBorder;
    right = px >= (float)(W - 3);
  }
  if (!__syncthreads_or(left || right)) return;  // (uniform; also orders `ext` and `pick`)
  bool any = false;
  if (left || right) {
    const float idy = ident[2 * p + 1];
    const float py = to_px(flow[b * flow_stride_b + flow_stride_c + p] + idy, (float)H);
    const float ox = to_px(idx, (float)W), oy = to_px(idy, (float)H);
    const float v[3] = {py, ox, oy};
    const float* base = actx + b * st.b + (int64_t)(Tp - 1) * st.tp + p;
    for (int s = 0; s < 2; ++s) {
      const int id = pick[s];
      if (!(s == 0 ? left : right) || id < 0) continue;
      if (!object_here(base + (int64_t)(id + 1) * st.l, Tc, st.tc)) continue;
      any = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (v[k] != v[k]) {
          atomicOr(&ext[s][6], 1u << k);
        } else {
          const unsigned key = ordered_key(v[k]);
          atomicMin(&ext[s][2 * k], key);
          atomicMax(&ext[s][2 * k + 1], key);
        }
      }
    }
  }
  if (!__syncthreads_or(any)) return;  // (a barrier: the LDS extrema are complete behind it)
  if (threadIdx.x < 2 * kExtWords) {
    const int s = threadIdx.x / kExtWords, w = threadIdx.x % kExtWords;
    unsigned* dst = ws + (b * 2 + s) * kSideWords + kMaxObj + w;
    const unsigned x = ext[s][w];
    if (w < 6) {
      if ((w & 1) == 0) {
        if (x != 0xffffffffu) atomicMin(dst, x);
      } else if (x != 0u) {
        atomicMax(dst, x);
      }
    } else if (w == 6 && x != 0u) {
      atomicOr(dst, x);
    }
  }
}

__global__ __launch_bounds__(kWave) void border_finalize_kernel(const unsigned* __restrict__ ws, int* __restrict__ valid,
                                                               int64_t* __restrict__ obj_id, double* __restrict__ corners,
                                                               int64_t sides, int L, int W) {
  const int64_t u = (int64_t)blockIdx.x * kWave + threadIdx.x;  // (b, s)
  if (u >= sides) return;
  const unsigned* w = ws + u * kSideWords;
  bool ok;
  const int id = pick_object(w, L - 1, ok);
  valid[u] = ok ? 1 : 0;
  obj_id[u] = ok ? id : 0;
  double* c = corners + u * 8;
  if (!ok) {
    for (int k = 0; k < 8; ++k) c[k] = 0.0;
    return;
  }
  const unsigned flags = w[kMaxObj + 6];
  double e[6];  // by0 by1 ox0 ox1 oy0 oy1: the exact widening of the fp32 extrema
  for (int k = 0; k < 6; ++k) {
    const float f = ((flags >> (k >> 1)) & 1u) ? __uint_as_float(0x7fc00000u) : ordered_value(w[kMaxObj + k]);
    e[k] = (double)f;
  }
  if ((u & 1) == 0) {  // left:  (0, by0) (0, by1) (ox1, oy1) (ox1, oy0)
    c[0] = 0.0;  c[1] = e[0];
    c[2] = 0.0;  c[3] = e[1];
    c[4] = e[3]; c[5] = e[5];
    c[6] = e[3]; c[7] = e[4];
  } else {             // right: (ox0, oy0) (ox0, oy1) (W - 1, by1) (W - 1, by0)
    c[0] = e[2]; c[1] = e[4];
    c[2] = e[2]; c[3] = e[5];
    c[4] = (double)(W - 1); c[5] = e[1];
    c[6] = (double)(W - 1); c[7] = e[0];
  }
}

}  // namespace waldo

using namespace waldo;

extern "C" int64_t waldo_border_objects_workspace_bytes(int64_t B) {
  if (B < 0) return 0;
  return B * 2 * kSideWords * (int64_t)sizeof(unsigned);
}

extern "C" int waldo_border_objects_fwd(const float* pred_flow, int64_t flow_stride_b, int64_t flow_stride_c,
                                        const float* ident, const float* alpha_ctx, int64_t stride_b, int64_t stride_tc,
                                        int64_t stride_tp, int64_t stride_l, int* valid, int64_t* obj_id, double* corners,
                                        void* workspace, int64_t B, int Tc, int Tp, int L, int H, int W,
                                        waldo_stream_t stream) {
  if (B < 0 || Tc < 1 || Tp < 1 || L < 2 || L > kMaxObj || H < 1 || W < 1 || H > 32767 || W > 32767 || flow_stride_b < 0 ||
      flow_stride_c < 0 || stride_b < 0 || stride_tc < 0 || stride_tp < 0 || stride_l < 0) {
    set_error("waldo_border_objects_fwd: bad arguments B=%lld Tc=%d Tp=%d L=%d H=%d W=%d (2 <= L <= %d layers, strides >= 0)",
              (long long)B, Tc, Tp, L, H, W, kMaxObj);
    return WALDO_EINVAL;
  }
  if (B == 0) return WALDO_OK;
  if (!pred_flow || !ident || !alpha_ctx || !valid || !obj_id || !corners || !workspace) {
    set_error("waldo_border_objects_fwd: null pointer");
    return WALDO_EINVAL;
  }
  const int64_t HW = (int64_t)H * W, tiles = (HW + kBlock - 1) / kBlock;
  if (B * tiles > 2147483647) {
    set_error("waldo_border_objects_fwd: problem too large for one launch");
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned* ws = static_cast<unsigned*>(workspace);
  const int64_t sides = B * 2, words = sides * kSideWords;
  const BorderCtx cs{stride_b, stride_tc, stride_tp, stride_l};
  border_init_kernel<<<dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(ws, sides);
  border_count_kernel<<<dim3((unsigned)(B * tiles)), dim3(kBlock), 0, st>>>(pred_flow, flow_stride_b, ident, alpha_ctx, cs,
                                                                           ws, Tc, Tp, L, H, W, (int)tiles);
  border_extrema_kernel<<<dim3((unsigned)(B * tiles)), dim3(kBlock), 0, st>>>(pred_flow, flow_stride_b, flow_stride_c, ident,
                                                                             alpha_ctx, cs, ws, Tc, Tp, L, H, W, (int)tiles);
  border_finalize_kernel<<<dim3((unsigned)((sides + kWave - 1) / kWave)), dim3(kWave), 0, st>>>(ws, valid, obj_id, corners,
                                                                                               sides, L, W);
  return launch_status("waldo_border_objects_fwd");
}
