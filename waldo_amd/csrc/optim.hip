// Optimizer step (include/waldo_hip.h "Optimizer step"): multi-tensor Adam / AdamW with the gradient norm, the clip, the
// non-finite skip and the loss scale decided on the device.  Three phases on the caller's stream -- statistics (one pass
// over the gradients), finalize (one workgroup), update -- and nothing between them reads the host.  Bandwidth-bound:
// 4 bytes per parameter in the statistics phase, 28 in the update phase (p, m, v read and written, g read); one workgroup
// per chunk of 4096 elements, 16-byte loads and stores where the tensor's base allows them, no LDS beyond the reductions.
#include <math.h>

#include "waldo_common.hip.h"

namespace waldo {

constexpr int kAdamK = 64;         // tensors per launch: the pack below travels BY VALUE in the kernel arguments
constexpr int kAdamChunk = 4096;   // elements per workgroup: 4 x 16 bytes per lane and tensor
constexpr int kAdamVecIters = kAdamChunk / 4 / kBlock;
constexpr int64_t kAdamMaxChunks = 2147483647;

// state / hyper words (include/waldo_hip.h has the table)
enum { kStStep = 0, kStNorm, kStCoef, kStMult, kStFinite, kStBc1, kStSqrtBc2, kStStepSize, kStSkipRow, kStSkipped,
       kStGrowth };
enum { kHyLr = 0, kHyBeta1, kHyBeta2, kHyEps, kHyMaxNorm, kHyScale, kHyGrowthFactor, kHyBackoffFactor, kHyGrowthInterval };

// 64 x 48 bytes + 4: under the 4 KB the kernel arguments may take.  chunk_end: the pack's chunk prefix (tensor t owns the
// chunks [chunk_end[t - 1], chunk_end[t]) of the launch's grid).
struct AdamPack {
  float* p[kAdamK];
  const float* g[kAdamK];
  float* m[kAdamK];
  float* v[kAdamK];
  int64_t numel[kAdamK];
  float wd[kAdamK];
  int chunk_end[kAdamK];
  int n;
};
static_assert(sizeof(AdamPack) + 64 <= 4096, "the pack and the other arguments must fit the kernel argument limit");

// the chunk a workgroup owns: its tensor (binary search of the chunk prefix: wave-uniform scalar loads of the kernel
// arguments), the chunk's first element and its length
struct AdamChunk {
  int t;
  int64_t start;
  int len;
};

__device__ __forceinline__ AdamChunk adam_chunk(const AdamPack& pk, int c) {
  int lo = 0, hi = pk.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c < pk.chunk_end[mid]) hi = mid;
    else lo = mid + 1;
  }
  AdamChunk ch;
  ch.t = lo;
  ch.start = (int64_t)(c - (lo ? pk.chunk_end[lo - 1] : 0)) * kAdamChunk;
  const int64_t left = pk.numel[lo] - ch.start;
  ch.len = (int)(left < kAdamChunk ? left : kAdamChunk);
  return ch;
}

__device__ __forceinline__ bool adam_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ bool adam_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// ---------------------------------------------------------------------------------------
// Statistics: per chunk the sum of squares and a non-finite flag -> workspace[chunk] = {sum, flag}.  The in-lane order,
// the wave butterfly and the four waves in order: the same bits at every run.  No atomics.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void adam_stat(float x, float& ss, bool& bad) {
  ss += x * x;
  bad |= adam_nonfinite(x);
}

__global__ __launch_bounds__(kBlock) void adam_stats_kernel(const AdamPack pk, float2* __restrict__ ws, int chunk_base) {
  __shared__ float s_sum[kBlock / kWave];
  __shared__ int s_bad[kBlock / kWave];
  const AdamChunk ch = adam_chunk(pk, (int)blockIdx.x);
  const float* __restrict__ g = pk.g[ch.t] + ch.start;
  const int tid = (int)threadIdx.x;
  float ss = 0.0f;
  bool bad = false;
  if (adam_aligned16(g)) {  // (a chunk starts a multiple of 16 KB into its tensor: the base's alignment is the chunk's)
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    if (ch.len == kAdamChunk) {
      f32x4 x[kAdamVecIters];
#pragma unroll
      for (int i = 0; i < kAdamVecIters; ++i) x[i] = g4[i * kBlock + tid];
#pragma unroll
      for (int i = 0; i < kAdamVecIters; ++i)
        for (int j = 0; j < 4; ++j) adam_stat(x[i][j], ss, bad);
    } else {
      const int n4 = ch.len >> 2;
      for (int q = tid; q < n4; q += kBlock) {
        const f32x4 x = g4[q];
        for (int j = 0; j < 4; ++j) adam_stat(x[j], ss, bad);
      }
      const int r = (n4 << 2) + tid;  // the scalar tail: len % 4 elements
      if (r < ch.len) adam_stat(g[r], ss, bad);
    }
  } else {
    for (int i = tid; i < ch.len; i += kBlock) adam_stat(g[i], ss, bad);
  }
  ss = wave_sum(ss);
  const bool wave_bad = __ballot(bad) != 0;
  if ((tid & (kWave - 1)) == 0) {
    s_sum[tid / kWave] = ss;
    s_bad[tid / kWave] = wave_bad;
  }
  __syncthreads();
  if (tid == 0) {
    float s = s_sum[0];
    int b = s_bad[0];
    for (int w = 1; w < kBlock / kWave; ++w) s += s_sum[w], b |= s_bad[w];
    ws[(int64_t)chunk_base + blockIdx.x] = make_float2(s, b ? 1.0f : 0.0f);
  }
}

// ---------------------------------------------------------------------------------------
// Finalize: ONE workgroup.  Thread i adds a contiguous run of the partials in index order, thread 0 the 256 runs in index
// order, all in double; thread 0 then does the step's scalar arithmetic in double and writes state and the scale.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void adam_finalize_kernel(const float2* __restrict__ ws, int chunks,
                                                               const float* __restrict__ loss, float* __restrict__ state,
                                                               float* __restrict__ hyper) {
  __shared__ double s_sum[kBlock];
  __shared__ int s_bad[kBlock];
  const int tid = (int)threadIdx.x;
  const int per = (chunks + kBlock - 1) / kBlock;
  const int64_t b0 = (int64_t)tid * per;
  const int64_t b1 = b0 + per < chunks ? b0 + per : chunks;
  double s = 0.0;
  int bad = 0;
  for (int64_t i = b0; i < b1; ++i) {
    const float2 w = ws[i];
    s += (double)w.x;
    bad |= w.y != 0.0f;
  }
  s_sum[tid] = s;
  s_bad[tid] = bad;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < kBlock; ++i) s += s_sum[i], bad |= s_bad[i];
  if (loss != nullptr && isnan(*loss)) bad = 1;  // the reference's test (models/synthesizer.py:1057)

  const double lr = hyper[kHyLr], beta1 = hyper[kHyBeta1], beta2 = hyper[kHyBeta2], max_norm = hyper[kHyMaxNorm];
  double scale = hyper[kHyScale];
  const double norm = sqrt(s) / scale;  // what clip_grad_norm_ sees after unscale_
  double coef = 1.0;
  if (max_norm > 0.0) coef = fmin(1.0, max_norm / (norm + 1e-6));
  state[kStNorm] = (float)norm;
  state[kStCoef] = (float)coef;
  state[kStMult] = (float)(coef / scale);
  state[kStFinite] = bad ? 0.0f : 1.0f;
  if (!bad) {
    const double step = (double)state[kStStep] + 1.0;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    state[kStStep] = (float)step;
    state[kStBc1] = (float)bc1;
    state[kStSqrtBc2] = (float)sqrt(bc2);
    state[kStStepSize] = (float)(lr / bc1);
    state[kStSkipRow] = 0.0f;
    // GradScaler.update: growth_factor after growth_interval finite steps in a row
    float tracker = state[kStGrowth] + 1.0f;
    const float interval = hyper[kHyGrowthInterval];
    if (interval > 0.0f && tracker >= interval) {
      scale *= (double)hyper[kHyGrowthFactor];
      tracker = 0.0f;
    }
    state[kStGrowth] = tracker;
  } else {
    state[kStSkipRow] += 1.0f;
    state[kStSkipped] += 1.0f;
    state[kStGrowth] = 0.0f;
    scale *= (double)hyper[kHyBackoffFactor];
  }
  hyper[kHyScale] = (float)scale;
}

// ---------------------------------------------------------------------------------------
// Update: torch.optim.Adam / AdamW's single-tensor arithmetic per element, in its order of operations (no contraction:
// the library is compiled with -ffp-contract=off).  A skipped step returns before any load.
// ---------------------------------------------------------------------------------------
struct AdamConsts {
  float mult, w1, beta2, w2, sqrt_bc2, eps, step_size, keep;  // w1 = 1 - beta1, w2 = 1 - beta2, keep = 1 - lr wd
  bool decay;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamConsts& c) {
  if (c.decay) p = p * c.keep;                                    // AdamW: p.mul_(1 - lr wd) = p - lr wd p
  g = g * c.mult;                                                 // unscale and clip in one factor
  const float d = g - m;                                          // exp_avg.lerp_(g, 1 - beta1), torch's two forms
  m = c.w1 < 0.5f ? m + c.w1 * d : g - d * (1.0f - c.w1);
  v = v * c.beta2 + (c.w2 * g) * g;                               // mul_(beta2).addcmul_(g, g, value=1 - beta2)
  const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = p + (-c.step_size) * (m / denom);                           // addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void adam_element4(f32x4& p, f32x4 g, f32x4& m, f32x4& v, const AdamConsts& c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float pj = p[j], mj = m[j], vj = v[j];
    adam_element(pj, g[j], mj, vj, c);
    p[j] = pj, m[j] = mj, v[j] = vj;
  }
}

__global__ __launch_bounds__(kBlock) void adam_update_kernel(const AdamPack pk, const float* __restrict__ state,
                                                             const float* __restrict__ hyper, int adamw) {
  if (state[kStFinite] == 0.0f) return;  // a skipped step writes nothing
  const AdamChunk ch = adam_chunk(pk, (int)blockIdx.x);
  AdamConsts c;
  const float lr = hyper[kHyLr], wd = pk.wd[ch.t];
  c.mult = state[kStMult];
  c.w1 = 1.0f - hyper[kHyBeta1];
  c.beta2 = hyper[kHyBeta2];
  c.w2 = 1.0f - c.beta2;
  c.sqrt_bc2 = state[kStSqrtBc2];
  c.eps = hyper[kHyEps];
  c.step_size = state[kStStepSize];
  c.decay = adamw && wd != 0.0f;
  c.keep = 1.0f - lr * wd;
  float* p = pk.p[ch.t] + ch.start;
  const float* g = pk.g[ch.t] + ch.start;
  float* m = pk.m[ch.t] + ch.start;
  float* v = pk.v[ch.t] + ch.start;
  const int tid = (int)threadIdx.x;
  if (adam_aligned16(p) && adam_aligned16(g) && adam_aligned16(m) && adam_aligned16(v)) {
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    if (ch.len == kAdamChunk) {
#pragma unroll
      for (int i = 0; i < kAdamVecIters; ++i) {
        const int q = i * kBlock + tid;
        f32x4 pp = p4[q], gg = g4[q], mm = m4[q], vv = v4[q];
        adam_element4(pp, gg, mm, vv, c);
        p4[q] = pp, m4[q] = mm, v4[q] = vv;
      }
    } else {
      const int n4 = ch.len >> 2;
      for (int q = tid; q < n4; q += kBlock) {
        f32x4 pp = p4[q], gg = g4[q], mm = m4[q], vv = v4[q];
        adam_element4(pp, gg, mm, vv, c);
        p4[q] = pp, m4[q] = mm, v4[q] = vv;
      }
      const int r = (n4 << 2) + tid;  // the scalar tail
      if (r < ch.len) adam_element(p[r], g[r], m[r], v[r], c);
    }
  } else {
    for (int i = tid; i < ch.len; i += kBlock) adam_element(p[i], g[i], m[i], v[i], c);
  }
}

static int64_t adam_chunks_of(int64_t numel) { return (numel + kAdamChunk - 1) / kAdamChunk; }

// the chunks of all tensors, or -1 where a size is negative, -2 where the chunks pass one launch's grid
static int64_t adam_total_chunks(int64_t n_tensors, const int64_t* numels) {
  int64_t total = 0;
  for (int64_t i = 0; i < n_tensors; ++i)
    if (numels[i] < 0) return -1;
  for (int64_t i = 0; i < n_tensors; ++i) {
    if (numels[i] > kAdamMaxChunks * kAdamChunk) return -2;
    total += adam_chunks_of(numels[i]);
    if (total > kAdamMaxChunks) return -2;
  }
  return total;
}

static int64_t adam_ws_bytes(int64_t chunks) {
  const int64_t b = chunks * (int64_t)sizeof(float2);
  return b < 256 ? 256 : (b + 255) / 256 * 256;
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_adam_limits(int* out, int n) {
  const int limits[4] = {kAdamK, kAdamChunk, WALDO_ADAM_STATE_WORDS, WALDO_ADAM_HYPER_WORDS};
  for (int i = 0; i < 4 && i < n && out; ++i) out[i] = limits[i];
  return 4;
}

extern "C" int64_t waldo_adam_workspace_bytes(int64_t n_tensors, const int64_t* numels) {
  if (n_tensors < 0 || (n_tensors > 0 && !numels)) return 0;
  const int64_t chunks = adam_total_chunks(n_tensors, numels);
  return chunks < 0 ? 0 : adam_ws_bytes(chunks);
}

extern "C" int waldo_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs,
                               float* const* exp_avg_sqs, const int64_t* numels, const float* weight_decays,
                               int64_t n_tensors, float* state, float* hyper, const float* loss, void* workspace,
                               int64_t workspace_bytes, int adamw, int* launches, waldo_stream_t stream) {
  const char* fn = "waldo_adam_step";
  if (launches) *launches = 0;
  if (n_tensors < 0) {
    set_error("%s: bad shape n_tensors=%lld", fn, (long long)n_tensors);
    return WALDO_EINVAL;
  }
  if (!state || !hyper || !workspace || (n_tensors > 0 && (!params || !grads || !exp_avgs || !exp_avg_sqs || !numels))) {
    set_error("%s: null pointer (only loss, weight_decays and launches may be null)", fn);
    return WALDO_EINVAL;
  }
  const int64_t chunks = adam_total_chunks(n_tensors, numels);
  if (chunks == -1) {
    set_error("%s: bad shape: a tensor with a negative number of elements", fn);
    return WALDO_EINVAL;
  }
  if (chunks < 0) {
    set_error("%s: too large: more than 2^31 - 1 chunks of %d elements", fn, kAdamChunk);
    return WALDO_EINVAL;
  }
  auto off4 = [](const void* p) { return ((uintptr_t)p & 3) != 0; };
  for (int64_t i = 0; i < n_tensors; ++i) {
    if (numels[i] == 0) continue;  // an empty tensor is skipped: its pointers are not looked at
    if (!params[i] || !grads[i] || !exp_avgs[i] || !exp_avg_sqs[i]) {
      set_error("%s: null pointer among the buffers of tensor %lld", fn, (long long)i);
      return WALDO_EINVAL;
    }
    if (off4(params[i]) || off4(grads[i]) || off4(exp_avgs[i]) || off4(exp_avg_sqs[i])) {
      set_error("%s: not aligned: a buffer of tensor %lld is off a 4-byte boundary", fn, (long long)i);
      return WALDO_EINVAL;
    }
  }
  if (off4(state) || off4(hyper) || off4(loss) || ((uintptr_t)workspace & 7) != 0) {
    set_error("%s: not aligned: state, hyper and loss need 4-byte, the workspace 8-byte alignment", fn);
    return WALDO_EINVAL;
  }
  if (workspace_bytes < adam_ws_bytes(chunks)) {
    set_error("%s: workspace of %lld bytes, waldo_adam_workspace_bytes says %lld", fn, (long long)workspace_bytes,
              (long long)adam_ws_bytes(chunks));
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  float2* ws = reinterpret_cast<float2*>(workspace);
  int count = 0;
  // phase 0: statistics, phase 1: update; the same packs of at most kAdamK non-empty tensors in both
  for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1) {
      adam_finalize_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(ws, (int)chunks, loss, state, hyper);
      ++count;
    }
    AdamPack pk;
    pk.n = 0;
    int pack_chunks = 0;
    int64_t chunk_base = 0;
    auto flush = [&]() {
      if (pk.n == 0) return;
      if (phase == 0) adam_stats_kernel<<<dim3((unsigned)pack_chunks), dim3(kBlock), 0, st>>>(pk, ws, (int)chunk_base);
      else adam_update_kernel<<<dim3((unsigned)pack_chunks), dim3(kBlock), 0, st>>>(pk, state, hyper, adamw);
      ++count;
      chunk_base += pack_chunks;
      pack_chunks = 0;
      pk.n = 0;
    };
    for (int64_t i = 0; i < n_tensors; ++i) {
      if (numels[i] == 0) continue;
      const int k = pk.n++;
      pk.p[k] = params[i], pk.g[k] = grads[i], pk.m[k] = exp_avgs[i], pk.v[k] = exp_avg_sqs[i];
      pk.numel[k] = numels[i];
      pk.wd[k] = weight_decays ? weight_decays[i] : 0.0f;
      pack_chunks += (int)adam_chunks_of(numels[i]);
      pk.chunk_end[k] = pack_chunks;
      if (pk.n == kAdamK) flush();
    }
    flush();
  }
  if (launches) *launches = count;
  return launch_status(fn);
}
