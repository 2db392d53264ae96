// The C entry points of the fused full-resolution passes (flow_ctx_kernels.hip.h) and their fp32 instances.  The
// 16-bit and packed instances are compiled in units of their own (flow_ctx_raw_*.hip, flow_ctx_packed*.hip).
#include "flow_ctx_kernels.hip.h"

namespace waldo {

// f(T{}) for the element type T of a *_dt entry point's `raw` (WALDO_DTYPE_F32 / _F16 / _BF16)
template <typename F>
static int raw_dispatch(const char* fn, int raw_dtype, F&& f) {
  switch (raw_dtype) {
    case WALDO_DTYPE_F32: return f(float{});
    case WALDO_DTYPE_F16: return f(_Float16{});
    case WALDO_DTYPE_BF16: return f(__bf16{});
  }
  set_error("%s: unknown raw dtype %d (WALDO_DTYPE_F32 / _F16 / _BF16)", fn, raw_dtype);
  return WALDO_EINVAL;
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_flow_ctx_alpha_fwd(const float* alpha_lr, const float* input, const float* dist,
                                        const float* occ, float* a01, float* alpha_out, unsigned* layer_bits, int B,
                                        int T, int Tw, int L, int Nl, int C, int chan_off, int H, int W,
                                        int scale, waldo_stream_t stream) {
  return flow_ctx_alpha_launch("waldo_flow_ctx_alpha_fwd", alpha_lr, input, dist, occ, a01, alpha_out, layer_bits, B, T,
                               Tw, L, Nl, C, chan_off, H, W, scale, stream);
}

extern "C" int waldo_flow_ctx_alpha_packed_fwd(const float* alpha_lr, const uint8_t* clip, const float* dist,
                                               const float* occ, float* a01, float* alpha_out, unsigned* layer_bits,
                                               int B, int T, int Tw, int L, int Nl, int H, int W, int scale,
                                               waldo_stream_t stream) {
  const char* fn = "waldo_flow_ctx_alpha_packed_fwd";
  if (Nl < 1 || Nl > kMaxCls) {
    set_error("%s: %d classes (1 to %d)", fn, Nl, kMaxCls);
    return WALDO_EINVAL;
  }
  if ((int64_t)B * Tw > 0 && !clip) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  return flow_ctx_alpha_launch(fn, alpha_lr, reinterpret_cast<const uint32_t*>(clip), dist, occ, a01, alpha_out,
                               layer_bits, B, T, Tw, L, Nl, 3 + Nl, 3, H, W, scale, stream);
}

extern "C" int waldo_flow_ctx_warp_fwd(const float* flow_lr, const float* isobj_lr, const float* a01,
                                       const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ,
                                       float* flow, float* alpha_ctx, float* disocc, float* alpha_max,
                                       const unsigned* layer_bits, int* status, int B, int T, int Tw, int Tc, int Tp,
                                       int L, int H, int W, int scale, waldo_stream_t stream) {
  const int64_t plane = (int64_t)H * scale * W * scale;
  const ActxLayout lay = {(int64_t)Tc * Tp * L * plane, (int64_t)Tp * L * plane, (int64_t)L * plane};
  return flow_ctx_warp_launch("waldo_flow_ctx_warp_fwd", flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, flow,
                              alpha_ctx, lay, nullptr, disocc, alpha_max, layer_bits, status, B, T, Tw, Tc, Tp, L, H, W,
                              scale, stream);
}

extern "C" int waldo_flow_ctx_warp_raw_fwd(const float* flow_lr, const float* isobj_lr, const float* a01,
                                           const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ,
                                           float* flow, float* raw, float* score, float* disocc,
                                           float* alpha_max, const unsigned* layer_bits, int* status, int B, int T,
                                           int Tw, int Tc, int Tp, int L, int H, int W, int scale, int C, int Tcx,
                                           waldo_stream_t stream) {
  return flow_ctx_warp_raw("waldo_flow_ctx_warp_raw_fwd", flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, flow, raw, score,
                           disocc, alpha_max, layer_bits, status, B, T, Tw, Tc, Tp, L, H, W, scale, C, Tcx, stream);
}

extern "C" int waldo_flow_ctx_warp_raw_fwd_dt(const float* flow_lr, const float* isobj_lr, const float* a01,
                                              const int64_t* ctx_ts, const int64_t* pred_ts, const float* occ,
                                              float* flow, void* raw, float* score, float* disocc, float* alpha_max,
                                              const unsigned* layer_bits, int* status, int B, int T, int Tw, int Tc,
                                              int Tp, int L, int H, int W, int scale, int C, int Tcx, int raw_dtype,
                                              waldo_stream_t stream) {
  const char* fn = "waldo_flow_ctx_warp_raw_fwd_dt";
  return raw_dispatch(fn, raw_dtype, [&](auto rt) {
    return flow_ctx_warp_raw(fn, flow_lr, isobj_lr, a01, ctx_ts, pred_ts, occ, flow, static_cast<decltype(rt)*>(raw),
                             score, disocc, alpha_max, layer_bits, status, B, T, Tw, Tc, Tp, L, H, W, scale, C, Tcx,
                             stream);
  });
}

extern "C" int waldo_frame_warp_fuse_fwd(const float* input, const float* flow, const float* alpha,
                                         const int64_t* ctx_ts, float* out, float* raw, int* status, int B, int T,
                                         int Tc, int Tp, int C, int L, int Hd, int Wd, int include_self,
                                         float eps, waldo_stream_t stream) {
  if (B > 0 && !alpha) {
    set_error("waldo_frame_warp_fuse_fwd: null pointer");
    return WALDO_EINVAL;
  }
  return frame_warp_fuse_launch("waldo_frame_warp_fuse_fwd", input, flow, alpha, nullptr, ctx_ts, out, raw, status, B, T,
                                Tc, Tp, C, L, Hd, Wd, include_self, eps, stream);
}

extern "C" int waldo_frame_warp_fuse_raw_fwd(const float* input, const float* flow, const float* score,
                                             const int64_t* ctx_ts, float* out, float* raw, int* status, int B, int T,
                                             int Tc, int Tp, int C, int L, int Hd, int Wd, int include_self, float eps,
                                             waldo_stream_t stream) {
  return frame_warp_fuse_raw("waldo_frame_warp_fuse_raw_fwd", input, flow, score, ctx_ts, out, raw, status, B, T, Tc, Tp,
                             C, L, Hd, Wd, include_self, eps, stream);
}

extern "C" int waldo_frame_warp_fuse_raw_fwd_dt(const float* input, const float* flow, const float* score,
                                                const int64_t* ctx_ts, float* out, void* raw, int* status, int B, int T,
                                                int Tc, int Tp, int C, int L, int Hd, int Wd, int include_self,
                                                float eps, int raw_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_frame_warp_fuse_raw_fwd_dt";
  return raw_dispatch(fn, raw_dtype, [&](auto rt) {
    return frame_warp_fuse_raw(fn, input, flow, score, ctx_ts, out, static_cast<decltype(rt)*>(raw), status, B, T, Tc,
                               Tp, C, L, Hd, Wd, include_self, eps, stream);
  });
}

extern "C" int waldo_frame_warp_fuse_raw_packed_fwd(const uint8_t* clip, const float* rgb_table, const float* flow,
                                                    const float* score, const int64_t* ctx_ts, float* out, void* raw,
                                                    int* status, int B, int T, int Tc, int Tp, int Nl, int L, int Hd,
                                                    int Wd, int include_self, float eps, int raw_dtype,
                                                    waldo_stream_t stream) {
  const char* fn = "waldo_frame_warp_fuse_raw_packed_fwd";
  return raw_dispatch(fn, raw_dtype, [&](auto rt) {
    if (Nl < 0 || Nl > kMaxCls) {
      set_error("%s: %d classes (0 to %d)", fn, Nl, kMaxCls);
      return WALDO_EINVAL;
    }
    if (B > 0 && (!clip || !rgb_table)) {
      set_error("%s: null pointer", fn);
      return WALDO_EINVAL;
    }
    return frame_warp_fuse_raw(fn, reinterpret_cast<const uint32_t*>(clip), flow, score, ctx_ts, out,
                               static_cast<decltype(rt)*>(raw), status, B, T, Tc, Tp, 3 + Nl, L, Hd, Wd, include_self,
                               eps, stream, rgb_table);
  });
}
