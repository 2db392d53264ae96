// Fused WIF hot path -- C-ABI entry points and dispatch over the compiled (LP, K3P) variants.
// Kernels: warp_composite_kernels.hip.h; one translation unit per padded layer count and layer element type
// (warp_composite_lp*.hip, warp_composite_inst.hip.h) so that the variants compile in parallel.
#include "det_common.hip.h"

namespace waldo {

constexpr int kMaxLayers = 32;
constexpr int kMaxK3 = 32;

// explicit instances in warp_composite_lp<LP>[_bf16 | _f16].hip (16-bit backward: LP <= kBwd2MaxLayers)
template <int LP, typename T>
void wc_fwd(bool k19, const T* layers, const float* basis_t, const float* mapping, const float* inv_kernel,
            const float* src_pts, const float* occ, float* rgb, float* alpha, int F, int L, int H, int W, int K3,
            float delta, hipStream_t st);
template <int LP, typename T>
void wc_bwd(bool k19, const T* layers, const float* basis_t, const float* mapping, const float* occ,
            const float* grad_rgb, const float* grad_alpha, T* grad_layers, float* grad_mapping, float* grad_occ,
            void* workspace, int F, int L, int H, int W, int K3, float delta, hipStream_t st, float* occ_slab);

static int check_common(const char* fn, int64_t F, int L, int H, int W, int K3) {
  if (F < 0 || L < 1 || L > kMaxLayers || H < 1 || W < 1 || K3 < 3 || K3 > kMaxK3) {
    set_error("%s: unsupported shape F=%lld L=%d H=%d W=%d K3=%d (need 1<=L<=%d, 3<=K3<=%d)", fn,
              (long long)F, L, H, W, K3, kMaxLayers, kMaxK3);
    return WALDO_EINVAL;
  }
  if (F > 65535 || F * L > 65535 || (int64_t)H * W > (int64_t)2147483647 / 4 || H > 32767 ||
      W > 32767) {
    set_error("%s: F*L=%lld (max 65535 per launch) or H*W=%lld too large", fn, (long long)F * L,
              (long long)H * W);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

// f(T{}) for the element type of a layer stack (enum waldo_dtype)
template <typename F>
static int layers_dispatch(const char* fn, int layers_dtype, F&& f) {
  switch (layers_dtype) {
    case WALDO_DTYPE_F32: return f(float{});
    case WALDO_DTYPE_F16: return f(_Float16{});
    case WALDO_DTYPE_BF16: return f(__bf16{});
  }
  set_error("%s: unknown dtype %d for layers (WALDO_DTYPE_F32 / _F16 / _BF16)", fn, layers_dtype);
  return WALDO_EINVAL;
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_max_layers(void) { return kMaxLayers; }

extern "C" int64_t waldo_warp_composite_bwd_workspace_bytes(int64_t F, int L, int H, int W,
                                                            int K3) {
  if (F < 0 || L < 1 || H < 1 || W < 1 || debug_option(WALDO_DEBUG_BWD_GENERIC)) return 0;
  return bwd_workspace_bytes(F, L, H, W, K3);
}

extern "C" int waldo_warp_composite_pts_supported(int L, int H, int W, int N) {
  return N + 3 == kGmapK3 && L >= 1 && L <= kMaxLayers && H >= 1 && W >= 1 && staged_eligible(H, W) &&
         (int64_t)H * W * kGmapK3 * 4 < 4294967296ll && !debug_option(WALDO_DEBUG_FWD_PLAIN);
}

namespace {

// a 16-bit stack is served by the staged forward alone
template <typename T>
int check_fwd16(const char* fn, int L, int H, int W, int K3) {
  if (!std::is_same_v<T, float> && !waldo_warp_composite_pts_supported(L, H, W, K3 - 3)) {
    set_error("%s: a 16-bit layer stack needs the staged forward (K3 == 19, W %% 4 == 0, H, W >= 2, "
              "WALDO_DEBUG_FWD_PLAIN off); not served: L=%d H=%d W=%d K3=%d -- pass fp32 layers",
              fn, L, H, W, K3);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

template <typename T>
int warp_composite_fwd(const char* fn, const T* layers, const float* basis_t, const float* mapping, const float* occ,
                       float* rgb, float* alpha, int64_t F, int L, int H, int W, int K3, float delta,
                       waldo_stream_t stream) {
  int rc = check_common(fn, F, L, H, W, K3);
  if (rc) return rc;
  rc = check_fwd16<T>(fn, L, H, W, K3);
  if (rc) return rc;
  if (F == 0) return WALDO_OK;
  if (!layers || !basis_t || !mapping || !occ || !rgb) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  with_padded_layers(L, [&](auto lp) {
    wc_fwd<decltype(lp)::value>(K3 == 19, layers, basis_t, mapping, nullptr, nullptr, occ, rgb, alpha, (int)F, L, H,
                                W, K3, delta, st);
  });
  return launch_status(fn);
}

template <typename T>
int warp_composite_pts_fwd(const char* fn, const T* layers, const float* basis_t, const float* inverse_kernel,
                           const float* src_pts, const float* occ, float* rgb, float* alpha, int64_t F, int L, int H,
                           int W, int N, float delta, waldo_stream_t stream) {
  int rc = check_common(fn, F, L, H, W, N + 3);
  if (rc) return rc;
  if (!waldo_warp_composite_pts_supported(L, H, W, N)) {
    set_error("%s: shape not served (N=%d H=%d W=%d); use waldo_tps_mapping_fwd + "
              "waldo_warp_composite_fwd%s", fn, N, H, W, std::is_same_v<T, float> ? "" : " with fp32 layers");
    return WALDO_EINVAL;
  }
  if (F == 0) return WALDO_OK;
  if (!layers || !basis_t || !inverse_kernel || !src_pts || !occ || !rgb) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int K3 = N + 3;
  with_padded_layers(L, [&](auto lp) {
    wc_fwd<decltype(lp)::value>(true, layers, basis_t, nullptr, inverse_kernel, src_pts, occ, rgb, alpha, (int)F, L,
                                H, W, K3, delta, st);
  });
  return launch_status(fn);
}

// workspace of the deterministic backward: the two-kernel backward's own (a multiple of 256 bytes), then the slab of
// grad_occ: one L x L row per (frame, 16 x 16 tile, wave) of K1
Carved<2> det_workspace(int64_t F, int L, int H, int W, int K3) {
  return carve(bwd_workspace_bytes(F, L, H, W, K3), F * bwd2_layout(F, L, H, W).ntiles16 * 4 * L * L * 4);
}

// det: the *_det entry points -- two-kernel backward only, its workspace followed by the grad_occ slab; grad_mapping
// and grad_occ are overwritten
template <typename T>
int warp_composite_bwd(const char* fn, const T* layers, const float* basis_t, const float* mapping, const float* occ,
                       const float* grad_rgb, const float* grad_alpha, T* grad_layers, float* grad_mapping,
                       float* grad_occ, void* workspace, int64_t workspace_bytes, int64_t F, int L, int H, int W,
                       int K3, float delta, waldo_stream_t stream, bool det = false) {
  constexpr bool kF32 = std::is_same_v<T, float>;
  int rc = check_common(fn, F, L, H, W, K3);
  if (rc) return rc;
  if (det) {
    const int64_t need2 = bwd_workspace_bytes(F > 0 ? F : 1, L, H, W, K3);
    if (need2 == 0) {
      set_error("%s: no deterministic kernel for this shape: it needs the two-kernel backward (K3 == 19, L <= %d, "
                "W %% 4 == 0, H, W >= 2); the generic backward sums with float atomics: L=%d H=%d W=%d K3=%d", fn,
                kBwd2MaxLayers, L, H, W, K3);
      return WALDO_EINVAL;
    }
    if (F == 0) return WALDO_OK;
    const Carved<2> lo = det_workspace(F, L, H, W, K3);
    rc = check_workspace(fn, workspace, workspace_bytes, lo.total());
    if (rc) return rc;
    if (!layers || !basis_t || !mapping || !occ || !grad_rgb || !grad_layers) {
      set_error("%s: null pointer", fn);
      return WALDO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    // (the reduction of the control-point partials adds to grad_mapping)
    if (grad_mapping != nullptr) fill_words(grad_mapping, 0u, sizeof(float) * (size_t)F * L * K3 * 2, st);
    float* slab = lo.at<float>(workspace, 1);
    with_padded_layers(L, [&](auto lp) {
      constexpr int LP = decltype(lp)::value;
      if constexpr (LP <= kBwd2MaxLayers)
        wc_bwd<LP>(true, layers, basis_t, mapping, occ, grad_rgb, grad_alpha, grad_layers, grad_mapping, grad_occ,
                   workspace, (int)F, L, H, W, K3, delta, st, slab);
    });
    return launch_status(fn);
  }
  // a 16-bit stack is served by the two-kernel backward alone (whose size query does not depend on F being 0)
  if (!kF32 && waldo_warp_composite_bwd_workspace_bytes(F > 0 ? F : 1, L, H, W, K3) == 0) {
    set_error("%s: a 16-bit layer stack needs the two-kernel backward (K3 == 19, L <= %d, W %% 4 == 0, H, W >= 2, "
              "WALDO_DEBUG_BWD_GENERIC off); not served: L=%d H=%d W=%d K3=%d -- pass fp32 layers",
              fn, kBwd2MaxLayers, L, H, W, K3);
    return WALDO_EINVAL;
  }
  if (F == 0) return WALDO_OK;
  if (!layers || !basis_t || !mapping || !occ || !grad_rgb || !grad_layers) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t need = debug_option(WALDO_DEBUG_BWD_GENERIC) ? 0 : bwd_workspace_bytes(F, L, H, W, K3);
  if (!kF32) rc = check_workspace(fn, workspace, workspace_bytes, need, " (a 16-bit layer stack has no generic backward)");
  else if (workspace != nullptr && need != 0) rc = check_workspace(fn, workspace, workspace_bytes, need);
  if (rc) return rc;
  if (need == 0) workspace = nullptr;  // shape served by the generic kernel, which needs none
  with_padded_layers(L, [&](auto lp) {
    constexpr int LP = decltype(lp)::value;
    if constexpr (kF32 || LP <= kBwd2MaxLayers)
      wc_bwd<LP>(K3 == 19, layers, basis_t, mapping, occ, grad_rgb, grad_alpha, grad_layers, grad_mapping, grad_occ,
                 workspace, (int)F, L, H, W, K3, delta, st, nullptr);
  });
  return launch_status(fn);
}

}  // namespace

extern "C" int waldo_warp_composite_fwd(const float* layers, const float* basis_t,
                                        const float* mapping, const float* occ, float* rgb,
                                        float* alpha, int64_t F, int L, int H, int W, int K3,
                                        float delta, waldo_stream_t stream) {
  return warp_composite_fwd("waldo_warp_composite_fwd", layers, basis_t, mapping, occ, rgb, alpha, F, L, H, W, K3,
                            delta, stream);
}

extern "C" int waldo_warp_composite_fwd_dt(const void* layers, const float* basis_t, const float* mapping,
                                           const float* occ, float* rgb, float* alpha, int64_t F, int L, int H, int W,
                                           int K3, float delta, int layers_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_warp_composite_fwd_dt";
  return layers_dispatch(fn, layers_dtype, [&](auto lt) {
    using T = decltype(lt);
    return warp_composite_fwd(fn, static_cast<const T*>(layers), basis_t, mapping, occ, rgb, alpha, F, L, H, W, K3,
                              delta, stream);
  });
}

extern "C" int waldo_warp_composite_pts_fwd(const float* layers, const float* basis_t,
                                            const float* inverse_kernel, const float* src_pts,
                                            const float* occ, float* rgb, float* alpha, int64_t F,
                                            int L, int H, int W, int N, float delta,
                                            waldo_stream_t stream) {
  return warp_composite_pts_fwd("waldo_warp_composite_pts_fwd", layers, basis_t, inverse_kernel, src_pts, occ, rgb,
                                alpha, F, L, H, W, N, delta, stream);
}

extern "C" int waldo_warp_composite_pts_fwd_dt(const void* layers, const float* basis_t, const float* inverse_kernel,
                                               const float* src_pts, const float* occ, float* rgb, float* alpha,
                                               int64_t F, int L, int H, int W, int N, float delta, int layers_dtype,
                                               waldo_stream_t stream) {
  const char* fn = "waldo_warp_composite_pts_fwd_dt";
  return layers_dispatch(fn, layers_dtype, [&](auto lt) {
    using T = decltype(lt);
    return warp_composite_pts_fwd(fn, static_cast<const T*>(layers), basis_t, inverse_kernel, src_pts, occ, rgb,
                                  alpha, F, L, H, W, N, delta, stream);
  });
}

extern "C" int waldo_warp_composite_bwd(const float* layers, const float* basis_t,
                                        const float* mapping, const float* occ,
                                        const float* grad_rgb, const float* grad_alpha,
                                        float* grad_layers, float* grad_mapping, float* grad_occ,
                                        void* workspace, int64_t workspace_bytes, int64_t F,
                                        int L, int H, int W, int K3, float delta,
                                        waldo_stream_t stream) {
  return warp_composite_bwd("waldo_warp_composite_bwd", layers, basis_t, mapping, occ, grad_rgb, grad_alpha,
                            grad_layers, grad_mapping, grad_occ, workspace, workspace_bytes, F, L, H, W, K3, delta,
                            stream);
}

extern "C" int waldo_warp_composite_bwd_dt(const void* layers, const float* basis_t, const float* mapping,
                                           const float* occ, const float* grad_rgb, const float* grad_alpha,
                                           void* grad_layers, float* grad_mapping, float* grad_occ, void* workspace,
                                           int64_t workspace_bytes, int64_t F, int L, int H, int W, int K3,
                                           float delta, int layers_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_warp_composite_bwd_dt";
  return layers_dispatch(fn, layers_dtype, [&](auto lt) {
    using T = decltype(lt);
    return warp_composite_bwd(fn, static_cast<const T*>(layers), basis_t, mapping, occ, grad_rgb, grad_alpha,
                              static_cast<T*>(grad_layers), grad_mapping, grad_occ, workspace, workspace_bytes, F, L,
                              H, W, K3, delta, stream);
  });
}

// ---- deterministic mode: the two-kernel backward with grad_occ in slab form; grad_layers, grad_mapping and grad_occ
// are OVERWRITTEN.  0: no deterministic kernel for the shape (the generic backward would serve it)
extern "C" int64_t waldo_warp_composite_bwd_det_workspace_bytes(int64_t F, int L, int H, int W, int K3) {
  if (F < 0 || L < 1 || H < 1 || W < 1) return 0;
  return bwd_workspace_bytes(F, L, H, W, K3) == 0 ? 0 : det_workspace(F, L, H, W, K3).total();
}

extern "C" int waldo_warp_composite_bwd_det(const void* layers, const float* basis_t, const float* mapping,
                                            const float* occ, const float* grad_rgb, const float* grad_alpha,
                                            void* grad_layers, float* grad_mapping, float* grad_occ, void* workspace,
                                            int64_t workspace_bytes, int64_t F, int L, int H, int W, int K3,
                                            float delta, int layers_dtype, waldo_stream_t stream) {
  const char* fn = "waldo_warp_composite_bwd_det";
  return layers_dispatch(fn, layers_dtype, [&](auto lt) {
    using T = decltype(lt);
    return warp_composite_bwd(fn, static_cast<const T*>(layers), basis_t, mapping, occ, grad_rgb, grad_alpha,
                              static_cast<T*>(grad_layers), grad_mapping, grad_occ, workspace, workspace_bytes, F, L,
                              H, W, K3, delta, stream, true);
  });
}
