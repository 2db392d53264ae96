// Pose objective (include/waldo_hip.h "Pose objective"): the three L1 terms of the future layer predictor's training
// step -- the reference's (to_ctx(real, ~ctx_mask) - to_ctx(pred, ~ctx_mask)).abs().mean() for obj_pose, bg_pose and
// occ_score (models/synthesizer.py:752-754) -- as a masked mean: no gather, no host read.
//   waldo_pose_l1_fwd   one launch over the three tensor pairs (a workgroup owns 2048 flat elements of ONE term and stores
//                       its partial sum), then one workgroup that counts the kept frames and adds each term's partials in a
//                       fixed order.  NO ATOMICS: the same bits from run to run.
//   waldo_pose_l1_bwd   one launch, the same walk: sgn(pred - real) * grad / (kept E) on kept frames, exact 0 elsewhere.
// The tensors are addressed flat, a dword per lane (coalesced); the frame of an element is its flat index / E, so rows of
// 3, 5 or 17 floats need no alignment.  At the recipe's shape the three pairs are 351 KB: the op is bound by its launches.
#include "waldo_common.hip.h"

namespace waldo {

namespace {

constexpr int kPosePx = 8;                      // elements per lane
constexpr int kPoseChunk = kBlock * kPosePx;    // elements per workgroup
constexpr int64_t kPoseMaxElems = 2147483647;   // flat indices are 32-bit

struct PoseArgs {
  const float* real[3];
  const float* pred[3];
  float* grad_pred[3];
  float* grad_real[3];
  const float* grad_term[3];
  const uint8_t* mask;
  const float* kept;
  float* partial;
  uint32_t E[3], total[3];  // elements per frame, elements in all (F E)
  uint32_t first[3];        // the first workgroup of each term
};

// block sum in a fixed order: lanes by wave_sum's butterfly, then the four waves in order; every thread gets it, and
// red4 can be used again at once
__device__ __forceinline__ float block_sum(float v, float* red4) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red4[threadIdx.x / kWave] = v;
  __syncthreads();
  const float total = ((red4[0] + red4[1]) + red4[2]) + red4[3];
  __syncthreads();
  return total;
}

// the term a workgroup serves and the flat index of its first element
__device__ __forceinline__ int pose_term(const PoseArgs& A, uint32_t& base) {
  const int k = blockIdx.x >= A.first[2] ? 2 : blockIdx.x >= A.first[1] ? 1 : 0;
  base = (blockIdx.x - A.first[k]) * (uint32_t)kPoseChunk;
  return k;
}

__global__ __launch_bounds__(kBlock) void pose_l1_partial_kernel(PoseArgs A) {
  __shared__ float red[kBlock / kWave];
  uint32_t base;
  const int k = pose_term(A, base);
  const float* __restrict__ real = A.real[k];
  const float* __restrict__ pred = A.pred[k];
  const uint32_t E = A.E[k], total = A.total[k];
  float acc = 0.0f;
#pragma unroll
  for (int it = 0; it < kPosePx; ++it) {
    const uint32_t i = base + it * kBlock + threadIdx.x;  // (base + 2047 < 2^31 + 2047: no wrap)
    if (i < total && A.mask[i / E] == 0) acc += fabsf(real[i] - pred[i]);
  }
  const float sum = block_sum(acc, red);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = sum;
}

// kept = the number of zero bytes of mask (F); terms[k] = (the partials of term k, in a fixed order) / (kept E_k)
__global__ __launch_bounds__(kBlock) void pose_l1_finish_kernel(PoseArgs A, int64_t F, uint32_t blocks,
                                                                float* __restrict__ terms, float* __restrict__ kept_out) {
  __shared__ float red[kBlock / kWave];
  float n = 0.0f;  // (F <= 2^24 is checked: every count below is an integer that fp32 holds exactly)
  for (int64_t f = threadIdx.x; f < F; f += kBlock) n += A.mask[f] == 0 ? 1.0f : 0.0f;
  const float kept = block_sum(n, red);
  if (threadIdx.x == 0) kept_out[0] = kept;
  for (int k = 0; k < 3; ++k) {
    const uint32_t end = k < 2 ? A.first[k + 1] : blocks;
    float acc = 0.0f;
    for (uint32_t b = A.first[k] + threadIdx.x; b < end; b += kBlock) acc += A.partial[b];
    const float sum = block_sum(acc, red);
    if (threadIdx.x == 0) terms[k] = sum / (kept * (float)A.E[k]);
  }
}

__global__ __launch_bounds__(kBlock) void pose_l1_bwd_kernel(PoseArgs A) {
  uint32_t base;
  const int k = pose_term(A, base);
  const float* __restrict__ real = A.real[k];
  const float* __restrict__ pred = A.pred[k];
  float* __restrict__ grad_pred = A.grad_pred[k];
  float* __restrict__ grad_real = A.grad_real[k];
  const uint32_t E = A.E[k], total = A.total[k];
  // (without a kept frame the quotient is not finite and no element uses it)
  const float scale = A.grad_term[k] != nullptr ? A.grad_term[k][0] / (A.kept[0] * (float)E) : 0.0f;
#pragma unroll
  for (int it = 0; it < kPosePx; ++it) {
    const uint32_t i = base + it * kBlock + threadIdx.x;
    if (i >= total) continue;
    float g = 0.0f;
    if (A.mask[i / E] == 0) {
      const float d = pred[i] - real[i];
      g = d > 0.0f ? scale : d < 0.0f ? -scale : 0.0f;
    }
    grad_pred[i] = g;
    if (grad_real != nullptr) grad_real[i] = -g;
  }
}

int64_t pose_chunks(int64_t total) { return (total + kPoseChunk - 1) / kPoseChunk; }

// the shape's checks and the grid; WALDO_EINVAL with the message set, or WALDO_OK with A's sizes filled in
int pose_grid(const char* fn, int64_t F, const int64_t (&E)[3], PoseArgs& A, uint32_t& blocks) {
  if (F <= 0 || E[0] <= 0 || E[1] <= 0 || E[2] <= 0) {
    set_error("%s: bad shape F=%lld E=(%lld, %lld, %lld) (all > 0)", fn, (long long)F, (long long)E[0], (long long)E[1],
              (long long)E[2]);
    return WALDO_EINVAL;
  }
  blocks = 0;
  for (int k = 0; k < 3; ++k) {
    if (F > (1 << 24) || E[k] > kPoseMaxElems / F) {
      set_error("%s: too large: F=%lld (at most 2^24) x E=%lld elements (at most 2^31 - 1)", fn, (long long)F,
                (long long)E[k]);
      return WALDO_EINVAL;
    }
    A.E[k] = (uint32_t)E[k];
    A.total[k] = (uint32_t)(F * E[k]);
    A.first[k] = blocks;
    blocks += (uint32_t)pose_chunks(F * E[k]);  // (at most 3 * 2^20)
  }
  return WALDO_OK;
}

}  // namespace

}  // namespace waldo

using namespace waldo;

extern "C" int64_t waldo_pose_l1_workspace_bytes(int64_t F, int64_t E_obj, int64_t E_bg, int64_t E_occ) {
  const int64_t E[3] = {E_obj, E_bg, E_occ};
  if (F <= 0 || F > (1 << 24)) return 0;
  int64_t blocks = 0;
  for (int k = 0; k < 3; ++k) {
    if (E[k] <= 0 || E[k] > kPoseMaxElems / F) return 0;
    blocks += pose_chunks(F * E[k]);
  }
  return (blocks * (int64_t)sizeof(float) + 255) / 256 * 256;
}

extern "C" int waldo_pose_l1_fwd(const float* real_obj, const float* pred_obj, const float* real_bg,
                                 const float* pred_bg, const float* real_occ, const float* pred_occ,
                                 const uint8_t* ctx_mask, float* terms, float* kept_out, void* workspace,
                                 int64_t workspace_bytes, int64_t F, int64_t E_obj, int64_t E_bg, int64_t E_occ,
                                 waldo_stream_t stream) {
  const char* fn = "waldo_pose_l1_fwd";
  if (!real_obj || !pred_obj || !real_bg || !pred_bg || !real_occ || !pred_occ || !ctx_mask || !terms || !kept_out ||
      !workspace) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  PoseArgs A{{real_obj, real_bg, real_occ}, {pred_obj, pred_bg, pred_occ}, {}, {}, {}, ctx_mask, nullptr,
             static_cast<float*>(workspace), {}, {}, {}};
  uint32_t blocks = 0;
  const int64_t E[3] = {E_obj, E_bg, E_occ};
  const int rc = pose_grid(fn, F, E, A, blocks);
  if (rc != WALDO_OK) return rc;
  const int64_t need = waldo_pose_l1_workspace_bytes(F, E_obj, E_bg, E_occ);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)need);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  pose_l1_partial_kernel<<<dim3(blocks), dim3(kBlock), 0, st>>>(A);
  pose_l1_finish_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(A, F, blocks, terms, kept_out);
  return launch_status(fn);
}

extern "C" int waldo_pose_l1_bwd(const float* real_obj, const float* pred_obj, const float* real_bg,
                                 const float* pred_bg, const float* real_occ, const float* pred_occ,
                                 const uint8_t* ctx_mask, const float* kept, const float* grad_obj,
                                 const float* grad_bg, const float* grad_occ, float* grad_pred_obj, float* grad_pred_bg,
                                 float* grad_pred_occ, float* grad_real_obj, float* grad_real_bg, float* grad_real_occ,
                                 int64_t F, int64_t E_obj, int64_t E_bg, int64_t E_occ, waldo_stream_t stream) {
  const char* fn = "waldo_pose_l1_bwd";
  if (!real_obj || !pred_obj || !real_bg || !pred_bg || !real_occ || !pred_occ || !ctx_mask || !kept ||
      !grad_pred_obj || !grad_pred_bg || !grad_pred_occ) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  PoseArgs A{{real_obj, real_bg, real_occ},
             {pred_obj, pred_bg, pred_occ},
             {grad_pred_obj, grad_pred_bg, grad_pred_occ},
             {grad_real_obj, grad_real_bg, grad_real_occ},
             {grad_obj, grad_bg, grad_occ},
             ctx_mask, kept, nullptr, {}, {}, {}};
  uint32_t blocks = 0;
  const int64_t E[3] = {E_obj, E_bg, E_occ};
  const int rc = pose_grid(fn, F, E, A, blocks);
  if (rc != WALDO_OK) return rc;
  pose_l1_bwd_kernel<<<dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream>>>(A);
  return launch_status(fn);
}
