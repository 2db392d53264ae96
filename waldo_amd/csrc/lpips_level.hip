// LPIPS level distance on fp32 maps (include/waldo_hip.h "LPIPS level distance"): the size queries and the fp32 entry
// points over the kernels of lpips_level.hip.h.
#include "lpips_level.hip.h"

using namespace waldo;

extern "C" int64_t waldo_lpips_level_workspace_bytes(int64_t N, int64_t C, int64_t P) { return lp_workspace_bytes(N, C, P); }

extern "C" int64_t waldo_lpips_level_saved_bytes(int64_t N, int64_t C, int64_t P) {
  if (!lp_shape_ok(N, C, P) || !lp_size_ok(N, C, P) || N > (INT64_MAX / 16) / P) return 0;
  return (N * 3 * P * (int64_t)sizeof(float) + 255) / 256 * 256;
}

extern "C" int waldo_lpips_level_fwd(const float* f0, const float* f1, const float* w, float* out, float* saved,
                                     void* workspace, int64_t workspace_bytes, int64_t N, int64_t C, int64_t P, float eps,
                                     waldo_stream_t stream) {
  return lp_fwd<float>("waldo_lpips_level_fwd", f0, f1, w, out, saved, workspace, workspace_bytes, N, C, P, eps, stream);
}

extern "C" int waldo_lpips_level_bwd(const float* f0, const float* f1, const float* w, const float* saved,
                                     const float* grad_out, float* grad_f0, int64_t N, int64_t C, int64_t P,
                                     waldo_stream_t stream) {
  return lp_bwd<float>("waldo_lpips_level_bwd", f0, f1, w, saved, grad_out, grad_f0, N, C, P, stream);
}
