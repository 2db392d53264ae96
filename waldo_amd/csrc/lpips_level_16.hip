// LPIPS level distance on 16-bit maps (include/waldo_hip.h "LPIPS level distance in 16 bits"): the _dt entry points over
// the kernels of lpips_level.hip.h with T = __bf16 / _Float16.  f0, f1 and grad_f0 are T; w, out, saved, the partials and
// grad_out stay fp32 and so does all arithmetic.  A lane loads ONE 2-byte element per channel (128 bytes per wave and
// channel row): nothing assumes more than 2-byte alignment of a pointer, or an even P.  The tile is the fp32 kernels'
// (64 pixels), so the size queries are theirs.
#include "lpips_level.hip.h"

using namespace waldo;

namespace {

// The dtype's refusals, before anything else: the fp32 code names the fp32 entry point.
int lp16_check_dtype(const char* fn, const char* fp32_fn, int dtype) {
  if (dtype == WALDO_DTYPE_F32) {
    set_error("%s: dtype WALDO_DTYPE_F32 is served by %s", fn, fp32_fn);
    return WALDO_EINVAL;
  }
  if (dtype != WALDO_DTYPE_F16 && dtype != WALDO_DTYPE_BF16) {
    set_error("%s: unknown dtype %d", fn, dtype);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

}  // namespace

extern "C" int waldo_lpips_level_fwd_dt(const void* f0, const void* f1, const float* w, float* out, float* saved,
                                        void* workspace, int64_t workspace_bytes, int64_t N, int64_t C, int64_t P, float eps,
                                        int dtype, waldo_stream_t stream) {
  const char* fn = "waldo_lpips_level_fwd_dt";
  const int rc = lp16_check_dtype(fn, "waldo_lpips_level_fwd", dtype);
  if (rc != WALDO_OK) return rc;
  if (dtype == WALDO_DTYPE_BF16)
    return lp_fwd<__bf16>(fn, f0, f1, w, out, saved, workspace, workspace_bytes, N, C, P, eps, stream);
  return lp_fwd<_Float16>(fn, f0, f1, w, out, saved, workspace, workspace_bytes, N, C, P, eps, stream);
}

extern "C" int waldo_lpips_level_bwd_dt(const void* f0, const void* f1, const float* w, const float* saved,
                                        const float* grad_out, void* grad_f0, int64_t N, int64_t C, int64_t P, int dtype,
                                        waldo_stream_t stream) {
  const char* fn = "waldo_lpips_level_bwd_dt";
  const int rc = lp16_check_dtype(fn, "waldo_lpips_level_bwd", dtype);
  if (rc != WALDO_OK) return rc;
  if (dtype == WALDO_DTYPE_BF16) return lp_bwd<__bf16>(fn, f0, f1, w, saved, grad_out, grad_f0, N, C, P, stream);
  return lp_bwd<_Float16>(fn, f0, f1, w, saved, grad_out, grad_f0, N, C, P, stream);
}
