// A12: fusion epilogue of WIF.forward with ii_score (models/nets/wif.py:49-54):
//   beta = net[:, :, :, 0:3];  w = softmax over Tc of net[:, :, :, 3];
//   a = sigmoid(vid[:, :, :, 4] + 5)   (INPUT channel 4, wif.py:53 -- not a network output; 0 if !ab)
//   out[b,t,c] = sum_tc (a * vid[b,t,tc,c] + beta[b,t,tc,c]) * w[b,t,tc]
// vid (B*T, Tc, C, HW) is the UNet input after the permute of wif.py:39, net (B*T, Tc, Co, HW) its
// output (Co >= 4).  The reference runs ~8 elementwise/softmax/reduce launches over (B,T,Tc,.,H,W)
// temporaries; here one thread owns one pixel of one (b,t), streams the Tc planes twice (max, then
// sum) and writes 3 values.  Pure HBM streaming: reads (5 + 4) * Tc floats, writes 3 per pixel.
// VT / NT: the element types of vid / net -- float, or _Float16 / __bf16 behind an autocast UNet (the *_dt entry
// points).  A 16-bit input is widened to fp32 on load and the arithmetic is the fp32 kernel's; a 16-bit gradient is
// the fp32 one rounded to nearest-even.
#include <type_traits>

#include "byte_rows.hip.h"
#include "quantize.hip.h"
#include "waldo_common.hip.h"

namespace waldo {

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + __expf(-x)); }

// a gradient in its input's type: the fp32 value, THEN rounded to nearest-even.  (Left alone, hipcc folds the last
// multiply and the fp16 cast into one v_fma_mixlo_f16 -- a single rounding of the exact product, which differs from the
// fp32 result's .to(float16) where the fp32 product lands on a tie.)
template <typename T>
__device__ __forceinline__ T round_to(float x) {
  if constexpr (!std::is_same<T, float>::value) asm volatile("" : "+v"(x));
  return (T)x;
}

template <typename VT, typename NT>
__global__ __launch_bounds__(kBlock) void wif_fuse_fwd_kernel(const VT* __restrict__ vid,
                                                              const NT* __restrict__ net,
                                                              float* __restrict__ out, int Tc, int C,
                                                              int Co, int64_t HW, int tiles, int ab) {
  const int64_t n = blockIdx.x / tiles;
  const int64_t p = (int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x;
  if (p >= HW) return;
  const VT* v = vid + n * Tc * C * HW + p;
  const NT* o = net + n * Tc * Co * HW + p;
  float m = -INFINITY;
  for (int t = 0; t < Tc; ++t) m = fmaxf(m, (float)o[((int64_t)t * Co + 3) * HW]);
  float den = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
  for (int t = 0; t < Tc; ++t) {
    const float e = expf((float)o[((int64_t)t * Co + 3) * HW] - m);
    const float a = ab ? sigmoidf((float)v[((int64_t)t * C + 4) * HW] + 5.0f) : 0.0f;
    den += e;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      acc[c] = fmaf(fmaf(a, (float)v[((int64_t)t * C + c) * HW], (float)o[((int64_t)t * Co + c) * HW]), e, acc[c]);
  }
  const float r = 1.0f / den;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(n * 3 + c) * HW + p] = acc[c] * r;
}

// grad_vid / grad_net are OVERWRITTEN on channels (0,1,2,4) / (0,1,2,3).  For an fp32 gradient the zero elsewhere
// must be provided by the caller (the launcher fills it first); a 16-bit gradient gets its zeros here (a word fill
// does not reach the last element of an odd count of 2-byte elements).
template <typename VT, typename NT>
__global__ __launch_bounds__(kBlock) void wif_fuse_bwd_kernel(
    const VT* __restrict__ vid, const NT* __restrict__ net, const float* __restrict__ out,
    const float* __restrict__ gout, VT* __restrict__ gvid, NT* __restrict__ gnet, int Tc, int C,
    int Co, int64_t HW, int tiles, int ab) {
  constexpr bool kZeroV = !std::is_same<VT, float>::value, kZeroN = !std::is_same<NT, float>::value;
  const int64_t n = blockIdx.x / tiles;
  const int64_t p = (int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x;
  if (p >= HW) return;
  const VT* v = vid + n * Tc * C * HW + p;
  const NT* o = net + n * Tc * Co * HW + p;
  VT* gv = gvid ? gvid + n * Tc * C * HW + p : nullptr;
  NT* go = gnet ? gnet + n * Tc * Co * HW + p : nullptr;
  float g[3], y[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g[c] = gout[(n * 3 + c) * HW + p];
    y[c] = out[(n * 3 + c) * HW + p];
  }
  float m = -INFINITY;
  for (int t = 0; t < Tc; ++t) m = fmaxf(m, (float)o[((int64_t)t * Co + 3) * HW]);
  float den = 0.0f;
  for (int t = 0; t < Tc; ++t) den += expf((float)o[((int64_t)t * Co + 3) * HW] - m);
  const float r = 1.0f / den;
  const float gy = g[0] * y[0] + g[1] * y[1] + g[2] * y[2];
  for (int t = 0; t < Tc; ++t) {
    const float w = expf((float)o[((int64_t)t * Co + 3) * HW] - m) * r;
    const float a = ab ? sigmoidf((float)v[((int64_t)t * C + 4) * HW] + 5.0f) : 0.0f;
    float gdot = 0.0f, ga = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = (float)v[((int64_t)t * C + c) * HW];
      const float u = fmaf(a, x, (float)o[((int64_t)t * Co + c) * HW]);  // a*x + beta
      gdot = fmaf(g[c], u, gdot);
      ga = fmaf(g[c] * w, x, ga);
      if (gv) gv[((int64_t)t * C + c) * HW] = round_to<VT>(g[c] * w * a);
      if (go) go[((int64_t)t * Co + c) * HW] = round_to<NT>(g[c] * w);
    }
    // softmax: d y / d s_t = w_t (u_t . g - y . g)
    if (go) go[((int64_t)t * Co + 3) * HW] = round_to<NT>(w * (gdot - gy));
    if (gv) gv[((int64_t)t * C + 4) * HW] = round_to<VT>(ab ? ga * a * (1.0f - a) : 0.0f);
    if (kZeroV && gv) {
      gv[((int64_t)t * C + 3) * HW] = (VT)0.0f;
      for (int c = 5; c < C; ++c) gv[((int64_t)t * C + c) * HW] = (VT)0.0f;
    }
    if (kZeroN && go)
      for (int c = 4; c < Co; ++c) go[((int64_t)t * Co + c) * HW] = (NT)0.0f;
  }
}

// ---- the epilogue with BYTES out (include/waldo_hip.h "Byte output"): the forward above, quantised (quantize.hip.h) and
// stored as uint8, planar (N, 3, HW) or interleaved (N, HW, 3): 3 bytes per pixel written in place of 12.  A lane owns
// 4 consecutive pixels, so that a plane's four bytes are one dword store (sub-dword stores: ~12 x the cost per byte).
// vec (HW % 4 == 0, 16-byte aligned fp32 / 8-byte aligned 16-bit bases): every plane is read with one 16- / 8-byte load
// per lane; otherwise element loads (an odd HW misaligns every second plane) and, where a group is cut by the end of
// the plane or its bytes do not start a dword, single-byte stores.
template <typename T>
__device__ __forceinline__ void load_px4(const T* __restrict__ p, bool vec, int valid, float (&v)[4]) {
  if (vec) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const t4 q = *reinterpret_cast<const t4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < valid ? (float)p[j] : 0.0f;
  }
}

template <typename VT, typename NT>
__global__ __launch_bounds__(kBlock) void wif_fuse_bytes_kernel(const VT* __restrict__ vid, const NT* __restrict__ net,
                                                                uint8_t* __restrict__ out, int Tc, int C, int Co,
                                                                int64_t HW, int tiles, int ab, int vec, int nhwc,
                                                                float lo, float range, int quant) {
  const int64_t n = blockIdx.x / tiles;
  const int64_t p = ((int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x) * 4;
  if (p >= HW) return;
  const int valid = (int)min((int64_t)4, HW - p);
  const VT* v = vid + n * Tc * C * HW + p;
  const NT* o = net + n * Tc * Co * HW + p;
  // (per pixel j: the text of wif_fuse_fwd_kernel, same order, same fmafs)
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int t = 0; t < Tc; ++t) {
    float s[4];
    load_px4(o + ((int64_t)t * Co + 3) * HW, vec, valid, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], s[j]);
  }
  float den[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[3][4] = {};
  for (int t = 0; t < Tc; ++t) {
    float s[4], g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, e[4], a[4];
    load_px4(o + ((int64_t)t * Co + 3) * HW, vec, valid, s);
    if (ab) load_px4(v + ((int64_t)t * C + 4) * HW, vec, valid, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = expf(s[j] - m[j]);
      a[j] = ab ? sigmoidf(g[j] + 5.0f) : 0.0f;
      den[j] += e[j];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x[4], b[4];
      load_px4(v + ((int64_t)t * C + c) * HW, vec, valid, x);
      load_px4(o + ((int64_t)t * Co + c) * HW, vec, valid, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c][j] = fmaf(fmaf(a[j], x[j], b[j]), e[j], acc[c][j]);
    }
  }
  uint32_t q[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float r = 1.0f / den[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c][j] = quant_byte(acc[c][j] * r, lo, range, quant);
  }
  if (nhwc) {
    uint8_t* d = out + (n * HW + p) * 3;
    if (valid == 4 && ((uintptr_t)d & 3u) == 0) {
      uint32_t w[3];
      pack_interleaved<4>(w, [&](int c, int j) { return q[c][j]; });
      store_aligned(d, w);
    } else {
      for (int j = 0; j < valid; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) d[3 * j + c] = (uint8_t)q[c][j];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint8_t* d = out + (n * 3 + c) * HW + p;
      if (valid == 4 && ((uintptr_t)d & 3u) == 0) {
        uint32_t w[1];
        pack_planar<4>(w, [&](int j) { return q[c][j]; });
        store_aligned(d, w);
      } else {
        for (int j = 0; j < valid; ++j) d[j] = (uint8_t)q[c][j];
      }
    }
  }
}

static int check_wif(const char* fn, int64_t N, int Tc, int C, int Co, int64_t HW) {
  if (N < 0 || Tc < 1 || C < 5 || Co < 4 || HW < 1 || N * ((HW + kBlock - 1) / kBlock) > 2147483647) {
    set_error("%s: bad shape N=%lld Tc=%d C=%d Co=%d HW=%lld (need C >= 5, Co >= 4)", fn,
              (long long)N, Tc, C, Co, (long long)HW);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

template <typename VT, typename NT>
static int wif_fwd_launch(const char* fn, const void* vid, const void* net, float* out, int64_t N, int Tc, int C,
                          int Co, int64_t HW, int ab, waldo_stream_t stream) {
  int rc = check_wif(fn, N, Tc, C, Co, HW);
  if (rc) return rc;
  if (N == 0) return WALDO_OK;
  if (!vid || !net || !out) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const int tiles = (int)((HW + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((wif_fuse_fwd_kernel<VT, NT>), dim3((unsigned)(N * tiles)), dim3(kBlock), 0,
                     (hipStream_t)stream, static_cast<const VT*>(vid), static_cast<const NT*>(net), out, Tc, C, Co,
                     HW, tiles, ab);
  return launch_status(fn);
}

template <typename VT, typename NT>
static int wif_bwd_launch(const char* fn, const void* vid, const void* net, const float* out, const float* grad_out,
                          void* grad_vid, void* grad_net, int64_t N, int Tc, int C, int Co, int64_t HW, int ab,
                          waldo_stream_t stream) {
  int rc = check_wif(fn, N, Tc, C, Co, HW);
  if (rc) return rc;
  if (N == 0) return WALDO_OK;
  if (!vid || !net || !out || !grad_out) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  // (a 16-bit gradient's zeros come from the kernel itself)
  if (grad_vid && std::is_same<VT, float>::value)
    fill_words(grad_vid, 0u, sizeof(float) * (size_t)(N * Tc * C * HW), st);
  if (grad_net && std::is_same<NT, float>::value)
    fill_words(grad_net, 0u, sizeof(float) * (size_t)(N * Tc * Co * HW), st);
  const int tiles = (int)((HW + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((wif_fuse_bwd_kernel<VT, NT>), dim3((unsigned)(N * tiles)), dim3(kBlock), 0, st,
                     static_cast<const VT*>(vid), static_cast<const NT*>(net), out, grad_out,
                     static_cast<VT*>(grad_vid), static_cast<NT*>(grad_net), Tc, C, Co, HW, tiles, ab);
  return launch_status(fn);
}

template <typename VT, typename NT>
static int wif_bytes_launch(const char* fn, const void* vid, const void* net, uint8_t* out, int64_t N, int Tc, int C,
                            int Co, int64_t HW, int ab, float lo, float range, int quant, int layout,
                            waldo_stream_t stream) {
  int rc = check_wif(fn, N, Tc, C, Co, HW);
  if (rc) return rc;
  if (!check_quant(fn, quant) || !check_layout(fn, layout) || !check_span(fn, lo, range)) return WALDO_EINVAL;
  if (N == 0) return WALDO_OK;
  if (!vid || !net || !out) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if ((uintptr_t)vid % sizeof(VT) || (uintptr_t)net % sizeof(NT)) {
    set_error("%s: vid / net not aligned to their elements", fn);
    return WALDO_EINVAL;
  }
  const int vec = HW % 4 == 0 && (uintptr_t)vid % (4 * sizeof(VT)) == 0 && (uintptr_t)net % (4 * sizeof(NT)) == 0;
  const int tiles = (int)(((HW + 3) / 4 + kBlock - 1) / kBlock);  // (<= check_wif's one-pixel tiles)
  hipLaunchKernelGGL((wif_fuse_bytes_kernel<VT, NT>), dim3((unsigned)(N * tiles)), dim3(kBlock), 0,
                     (hipStream_t)stream, static_cast<const VT*>(vid), static_cast<const NT*>(net), out, Tc, C, Co,
                     HW, tiles, ab, vec, (int)(layout == WALDO_BYTES_NHWC), lo, range, quant);
  return launch_status(fn);
}

// the 3 x 3 element types of (vid, net): f(VT{}, NT{}) for the pair the codes name; an unknown code is refused before
// anything is launched
template <typename VT, typename F>
static int wif_dispatch_net(int net_dtype, F&& f) {
  switch (net_dtype) {
    case WALDO_DTYPE_F16: return f(VT{}, _Float16{});
    case WALDO_DTYPE_BF16: return f(VT{}, __bf16{});
    default: return f(VT{}, float{});
  }
}

template <typename F>
static int wif_dispatch(const char* fn, int vid_dtype, int net_dtype, F&& f) {
  auto known = [](int d) { return d == WALDO_DTYPE_F32 || d == WALDO_DTYPE_F16 || d == WALDO_DTYPE_BF16; };
  if (!known(vid_dtype) || !known(net_dtype)) {
    set_error("%s: unknown dtype vid=%d net=%d (WALDO_DTYPE_F32 / _F16 / _BF16)", fn, vid_dtype, net_dtype);
    return WALDO_EINVAL;
  }
  switch (vid_dtype) {
    case WALDO_DTYPE_F16: return wif_dispatch_net<_Float16>(net_dtype, f);
    case WALDO_DTYPE_BF16: return wif_dispatch_net<__bf16>(net_dtype, f);
    default: return wif_dispatch_net<float>(net_dtype, f);
  }
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_wif_fuse_fwd(const float* vid, const float* net, float* out, int64_t N, int Tc,
                                  int C, int Co, int64_t HW, int ab, waldo_stream_t stream) {
  return wif_fwd_launch<float, float>("waldo_wif_fuse_fwd", vid, net, out, N, Tc, C, Co, HW, ab, stream);
}

extern "C" int waldo_wif_fuse_bwd(const float* vid, const float* net, const float* out,
                                  const float* grad_out, float* grad_vid, float* grad_net, int64_t N,
                                  int Tc, int C, int Co, int64_t HW, int ab, waldo_stream_t stream) {
  return wif_bwd_launch<float, float>("waldo_wif_fuse_bwd", vid, net, out, grad_out, grad_vid, grad_net, N, Tc, C, Co,
                                      HW, ab, stream);
}

extern "C" int waldo_wif_fuse_fwd_dt(const void* vid, const void* net, float* out, int64_t N, int Tc, int C, int Co,
                                     int64_t HW, int ab, int vid_dtype, int net_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_wif_fuse_fwd_dt";
  return wif_dispatch(fn, vid_dtype, net_dtype, [&](auto vt, auto nt) {
    return wif_fwd_launch<decltype(vt), decltype(nt)>(fn, vid, net, out, N, Tc, C, Co, HW, ab, stream);
  });
}

extern "C" int waldo_wif_fuse_bwd_dt(const void* vid, const void* net, const float* out, const float* grad_out,
                                     void* grad_vid, void* grad_net, int64_t N, int Tc, int C, int Co, int64_t HW,
                                     int ab, int vid_dtype, int net_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_wif_fuse_bwd_dt";
  return wif_dispatch(fn, vid_dtype, net_dtype, [&](auto vt, auto nt) {
    return wif_bwd_launch<decltype(vt), decltype(nt)>(fn, vid, net, out, grad_out, grad_vid, grad_net, N, Tc, C, Co,
                                                      HW, ab, stream);
  });
}

extern "C" int waldo_wif_fuse_bytes_fwd(const float* vid, const float* net, uint8_t* out, int64_t N, int Tc, int C,
                                        int Co, int64_t HW, int ab, float lo, float range, int quant, int layout,
                                        waldo_stream_t stream) {
  return wif_bytes_launch<float, float>("waldo_wif_fuse_bytes_fwd", vid, net, out, N, Tc, C, Co, HW, ab, lo, range,
                                        quant, layout, stream);
}

extern "C" int waldo_wif_fuse_bytes_fwd_dt(const void* vid, const void* net, uint8_t* out, int64_t N, int Tc, int C,
                                           int Co, int64_t HW, int ab, float lo, float range, int quant, int layout,
                                           int vid_dtype, int net_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_wif_fuse_bytes_fwd_dt";
  return wif_dispatch(fn, vid_dtype, net_dtype, [&](auto vt, auto nt) {
    return wif_bytes_launch<decltype(vt), decltype(nt)>(fn, vid, net, out, N, Tc, C, Co, HW, ab, lo, range, quant,
                                                        layout, stream);
  });
}
