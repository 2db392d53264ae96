// Plane norm (include/waldo_hip.h "Plane norm"): the entry points, their argument checks and the float instances of
// the kernels (plane_norm_kernels.hip.h, where the regimes and the layouts are described; the 16-bit instances are
// compiled in plane_norm_bf16.hip and plane_norm_f16.hip).
#include "plane_norm_kernels.hip.h"

namespace waldo {

WALDO_PLANE_NORM_INSTANCES(, float)

namespace {

constexpr int64_t kMaxHW = (int64_t)1 << 30;

bool aligned(const void* p, unsigned to) { return ((uintptr_t)p & (to - 1)) == 0; }

// shape checks shared by the entry points and the workspace query; S = chunks of a plane (1: resident)
bool shape_ok(const char* fn, int64_t N, int C, int Cs, int H, int W, int64_t& HW, int& S) {
  if (N < 0 || C < 1 || Cs < 0 || H < 1 || W < 1) {
    set_error("%s: bad shape N=%lld C=%d Cs=%d H=%d W=%d (N, Cs >= 0; C, H, W >= 1)", fn, (long long)N, C, Cs, H, W);
    return false;
  }
  HW = (int64_t)H * W;
  if (HW > kMaxHW) {
    set_error("%s: too large: H W = %lld (at most 2^30)", fn, (long long)HW);
    return false;
  }
  S = HW > kPnChunk ? (int)((HW + kPnChunk - 1) / kPnChunk) : 1;
  const int64_t cmax = C > Cs ? C : Cs;
  // every plane index, workgroup index and chunk record index stays below 2^31 (the strides are the caller's, 64-bit)
  if (N > INT32_MAX || N * cmax > INT32_MAX || N * cmax * S > INT32_MAX) {
    set_error("%s: too large: N=%lld C=%d Cs=%d with %d chunks per plane is more than 2^31 - 1 workgroups", fn,
              (long long)N, C, Cs, S);
    return false;
  }
  return true;
}

int64_t workspace_bytes_of(int64_t P, int S) { return S > 1 ? P * S * 2 * (int64_t)sizeof(float) : 0; }

// "not aligned": the buffers of element type E to sizeof(E), every other one to 4 bytes
template <typename E>
bool alignment_ok(const char* fn, std::initializer_list<const void*> typed, std::initializer_list<const void*> f32) {
  bool ok = true;
  for (const void* p : typed) ok = ok && aligned(p, sizeof(E));
  for (const void* p : f32) ok = ok && aligned(p, 4);
  if (ok) return true;
  if (sizeof(E) == 4) set_error("%s: pointer not aligned to 4 bytes", fn);
  else set_error("%s: pointer not aligned (the 16-bit buffers to 2 bytes, every other one to 4)", fn);
  return false;
}

bool workspace_ok(const char* fn, const void* workspace, int64_t workspace_bytes, int64_t need) {
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace too small: %lld bytes, %lld needed (waldo_plane_norm_workspace_bytes)", fn,
              (long long)(workspace ? workspace_bytes : 0), (long long)need);
    return false;
  }
  return true;
}

// 16-byte accesses of a buffer of E: its base on a 16-byte boundary, its strides whole accesses
template <typename E>
bool vec_ok(const void* p, int64_t s0, int64_t s1 = 0) {
  constexpr int V = PlanePack<E>::kN;
  return aligned(p, 16) && s0 % V == 0 && s1 % V == 0;
}

template <typename E>
int fwd_body(const char* fn, const E* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta, float eps,
             const E* skip, int64_t ss_n, int64_t ss_c, E* out, int64_t os_n, float* mean, float* rstd, void* workspace,
             int64_t workspace_bytes, int64_t N, int C, int Cs, int H, int W, waldo_stream_t stream) {
  int64_t HW;
  int S;
  if (!shape_ok(fn, N, C, Cs, H, W, HW, S)) return WALDO_EINVAL;
  if (xs_n < 0 || xs_c < 0 || ss_n < 0 || ss_c < 0 || os_n < 0) {
    set_error("%s: negative stride", fn);
    return WALDO_EINVAL;
  }
  if (!(eps >= 0.0f) || !(eps < INFINITY)) {
    set_error("%s: bad eps %g (finite, >= 0)", fn, (double)eps);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!x || !gamma || !beta || !out || !mean || !rstd || (Cs > 0 && !skip)) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!alignment_ok<E>(fn, {x, out, skip}, {gamma, beta, mean, rstd, workspace})) return WALDO_EINVAL;
  if (os_n < (int64_t)(C + Cs) * HW) {
    set_error("%s: bad stride: out's batch stride %lld is below (C + Cs) H W = %lld", fn, (long long)os_n,
              (long long)((int64_t)(C + Cs) * HW));
    return WALDO_EINVAL;
  }
  const int64_t P = N * C;
  if (!workspace_ok(fn, workspace, workspace_bytes, workspace_bytes_of(P, S))) return WALDO_EINVAL;
  PlaneNormArgs<E> a{};
  a.x = x, a.xs_n = xs_n, a.xs_c = xs_c, a.gamma = gamma, a.beta = beta, a.eps = eps;
  a.out = out, a.os_n = os_n, a.mean = mean, a.rstd = rstd, a.ws = static_cast<float*>(workspace);
  a.P = P, a.C = C, a.S = S, a.HW = HW;
  const bool dst_vec = vec_ok<E>(out, os_n, HW);
  hipStream_t st = (hipStream_t)stream;
  int rc = plane_norm_run<E, false>(fn, a, dst_vec && vec_ok<E>(x, xs_n, xs_c), st);
  if (rc != WALDO_OK || Cs == 0) return rc;
  return plane_skip_copy<E>(fn, skip, ss_n, ss_c, out, os_n, N, C, Cs, S, HW, dst_vec && vec_ok<E>(skip, ss_n, ss_c), st);
}

template <typename E>
int bwd_body(const char* fn, const E* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
             const float* mean, const float* rstd, const E* grad_out, int64_t gs_n, int64_t gs_c, E* grad_x, float* sums,
             void* workspace, int64_t workspace_bytes, int64_t N, int C, int H, int W, waldo_stream_t stream) {
  int64_t HW;
  int S;
  if (!shape_ok(fn, N, C, 0, H, W, HW, S)) return WALDO_EINVAL;
  if (xs_n < 0 || xs_c < 0 || gs_n < 0 || gs_c < 0) {
    set_error("%s: negative stride", fn);
    return WALDO_EINVAL;
  }
  if (N == 0) return WALDO_OK;
  if (!x || !gamma || !beta || !mean || !rstd || !grad_out || !grad_x || !sums) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  if (!alignment_ok<E>(fn, {x, grad_out, grad_x}, {gamma, beta, mean, rstd, sums, workspace})) return WALDO_EINVAL;
  const int64_t P = N * C;
  if (!workspace_ok(fn, workspace, workspace_bytes, workspace_bytes_of(P, S))) return WALDO_EINVAL;
  PlaneNormArgs<E> a{};
  a.x = x, a.xs_n = xs_n, a.xs_c = xs_c, a.gamma = gamma, a.beta = beta;
  a.out = grad_x, a.mean = const_cast<float*>(mean), a.rstd = const_cast<float*>(rstd);
  a.go = grad_out, a.gs_n = gs_n, a.gs_c = gs_c, a.sums = sums, a.ws = static_cast<float*>(workspace);
  a.P = P, a.C = C, a.S = S, a.HW = HW;
  const bool vec = vec_ok<E>(x, xs_n, xs_c) && vec_ok<E>(grad_out, gs_n, gs_c) && vec_ok<E>(grad_x, HW);
  return plane_norm_run<E, true>(fn, a, vec, (hipStream_t)stream);
}

// f(E{}) for the element type of a dtype code; an unknown code is refused before any pointer is looked at
template <typename F>
int with_element_type(const char* fn, int dtype, F&& f) {
  switch (dtype) {
    case WALDO_DTYPE_F32: return f(float{});
    case WALDO_DTYPE_F16: return f(_Float16{});
    case WALDO_DTYPE_BF16: return f(__bf16{});
  }
  set_error("%s: unknown dtype %d (WALDO_DTYPE_F32 / _F16 / _BF16)", fn, dtype);
  return WALDO_EINVAL;
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_plane_norm_limits(int* out, int n) {
  const int limits[3] = {kPnWaveMax, kPnMidMax, kPnChunk};
  for (int i = 0; i < 3 && i < n && out; ++i) out[i] = limits[i];
  return 3;
}

extern "C" int64_t waldo_plane_norm_workspace_bytes(int64_t N, int C, int H, int W) {
  int64_t HW;
  int S;
  if (!shape_ok("waldo_plane_norm_workspace_bytes", N, C, 0, H, W, HW, S)) return -1;
  return workspace_bytes_of(N * C, S);
}

extern "C" int waldo_plane_norm_gelu_fwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                         float eps, const float* skip, int64_t ss_n, int64_t ss_c, float* out, int64_t os_n,
                                         float* mean, float* rstd, void* workspace, int64_t workspace_bytes, int64_t N, int C,
                                         int Cs, int H, int W, waldo_stream_t stream) {
  return fwd_body<float>("waldo_plane_norm_gelu_fwd", x, xs_n, xs_c, gamma, beta, eps, skip, ss_n, ss_c, out, os_n, mean,
                         rstd, workspace, workspace_bytes, N, C, Cs, H, W, stream);
}

extern "C" int waldo_plane_norm_gelu_bwd(const float* x, int64_t xs_n, int64_t xs_c, const float* gamma, const float* beta,
                                         const float* mean, const float* rstd, const float* grad_out, int64_t gs_n,
                                         int64_t gs_c, float* grad_x, float* sums, void* workspace, int64_t workspace_bytes,
                                         int64_t N, int C, int H, int W, waldo_stream_t stream) {
  return bwd_body<float>("waldo_plane_norm_gelu_bwd", x, xs_n, xs_c, gamma, beta, mean, rstd, grad_out, gs_n, gs_c, grad_x,
                         sums, workspace, workspace_bytes, N, C, H, W, stream);
}

extern "C" int waldo_plane_norm_gelu_fwd_dt(const void* x, int64_t xs_n, int64_t xs_c, const float* gamma,
                                            const float* beta, float eps, const void* skip, int64_t ss_n, int64_t ss_c,
                                            void* out, int64_t os_n, float* mean, float* rstd, void* workspace,
                                            int64_t workspace_bytes, int64_t N, int C, int Cs, int H, int W, int dtype,
                                            waldo_stream_t stream) {
  const char* fn = "waldo_plane_norm_gelu_fwd_dt";
  return with_element_type(fn, dtype, [&](auto e) {
    typedef decltype(e) E;
    return fwd_body<E>(std::is_same_v<E, float> ? "waldo_plane_norm_gelu_fwd" : fn, static_cast<const E*>(x), xs_n, xs_c,
                       gamma, beta, eps, static_cast<const E*>(skip), ss_n, ss_c, static_cast<E*>(out), os_n, mean, rstd,
                       workspace, workspace_bytes, N, C, Cs, H, W, stream);
  });
}

extern "C" int waldo_plane_norm_gelu_bwd_dt(const void* x, int64_t xs_n, int64_t xs_c, const float* gamma,
                                            const float* beta, const float* mean, const float* rstd, const void* grad_out,
                                            int64_t gs_n, int64_t gs_c, void* grad_x, float* sums, void* workspace,
                                            int64_t workspace_bytes, int64_t N, int C, int H, int W, int dtype,
                                            waldo_stream_t stream) {
  const char* fn = "waldo_plane_norm_gelu_bwd_dt";
  return with_element_type(fn, dtype, [&](auto e) {
    typedef decltype(e) E;
    return bwd_body<E>(std::is_same_v<E, float> ? "waldo_plane_norm_gelu_bwd" : fn, static_cast<const E*>(x), xs_n, xs_c,
                       gamma, beta, mean, rstd, static_cast<const E*>(grad_out), gs_n, gs_c, static_cast<E*>(grad_x), sums,
                       workspace, workspace_bytes, N, C, H, W, stream);
  });
}
