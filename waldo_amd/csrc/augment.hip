// Clip augmentation (include/waldo_hip.h "Clip augmentation"): a training sample from the packed clip in one pass -- crop,
// bilinear resize, flips, colour jitter and normalisation of the frames, the resized layout logits from the class bytes
// of the same four words, and the flow through its two resizes.  Store-bound: 4 (3 + Nl + 2) bytes written per output
// pixel against four cached word reads, so every plane gets one coalesced store per wave and nothing goes through LDS.
#include "packed_clip.hip.h"

// sizing knobs (tools_dev/build_variant.py; none changes what is computed; measured: DESIGN.md 4r)
#ifndef WALDO_AUG_PX
#define WALDO_AUG_PX 4  // output pixels per lane along x where Wo % 4 == 0 and the outputs are 16-byte aligned (else 1)
#endif
#ifndef WALDO_AUG_NT
#define WALDO_AUG_NT 1  // non-temporal stores for the planes (written once, read next by another kernel); 0: plain
#endif
#ifndef WALDO_AUG_LAUNCHES
#define WALDO_AUG_LAUNCHES 1  // 2: the frames and the flow in a launch each
#endif

namespace waldo {

constexpr int kAugMaxSize = 32767;
// the three operations (0 brightness, 1 saturation, 2 hue) of each order, two bits each, six bits per order
constexpr uint64_t kAugOrders = 36ull | 24ull << 6 | 33ull << 12 | 9ull << 18 | 18ull << 24 | 6ull << 30;

struct AugTap {
  int i0, i1;
  float f;
};

// the two source indices and the weight of index o of an axis resized from n_src (scale = n_src / the axis' length):
// F.interpolate's align_corners=False position, clamped to the source
__device__ __forceinline__ AugTap aug_tap(int o, float scale, int n_src) {
  float s = ((float)o + 0.5f) * scale - 0.5f;
  s = fminf(fmaxf(s, 0.0f), (float)(n_src - 1));
  AugTap t;
  t.i0 = (int)s;
  t.i1 = min(t.i0 + 1, n_src - 1);
  t.f = s - (float)t.i0;
  return t;
}

__device__ __forceinline__ float aug_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ void aug_hue(float& r, float& g, float& b, float hue) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  if (maxc == minc) return;  // s = 0: the pixel comes back as it is
  const float cr = maxc - minc, s = cr / maxc;
  const float rc = (maxc - r) / cr, gc = (maxc - g) / cr, bc = (maxc - b) / cr;
  float h = maxc == r ? bc - gc : maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc;
  h = h / 6.0f + 1.0f;
  h -= floorf(h);
  h += hue;
  h -= floorf(h);  // (h + hue) mod 1, in [0, 1]
  const float h6 = h * 6.0f, fi = floorf(h6), f = h6 - fi;
  const float v = maxc, p = aug_clamp01(v * (1.0f - s)), q = aug_clamp01(v * (1.0f - s * f)),
              t = aug_clamp01(v * (1.0f - s * (1.0f - f)));
  switch ((int)fi % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// the frame's jitter operations in its order (ops: wave-uniform, six bits of kAugOrders)
__device__ __forceinline__ void aug_jitter(float& r, float& g, float& b, unsigned ops, float jb, float js, float jh) {
  for (int j = 0; j < 3; ++j) {
    const unsigned op = (ops >> (2 * j)) & 3u;
    if (op == 0) {
      r = aug_clamp01(r * jb), g = aug_clamp01(g * jb), b = aug_clamp01(b * jb);
    } else if (op == 1) {
      const float grey = (0.299f * r + 0.587f * g) + 0.114f * b, k = (1.0f - js) * grey;
      r = aug_clamp01(js * r + k), g = aug_clamp01(js * g + k), b = aug_clamp01(js * b + k);
    } else {
      aug_hue(r, g, b, jh);
    }
  }
}

template <int PX>
__device__ __forceinline__ void aug_store(float* p, const float (&v)[PX]) {
  if constexpr (PX == 4) {
    typedef float f32x4_a __attribute__((ext_vector_type(4)));
    f32x4_a q = {v[0], v[1], v[2], v[3]};
    if (WALDO_AUG_NT) __builtin_nontemporal_store(q, reinterpret_cast<f32x4_a*>(p));
    else *reinterpret_cast<f32x4_a*>(p) = q;
  } else {
    for (int i = 0; i < PX; ++i) {
      if (WALDO_AUG_NT) __builtin_nontemporal_store(v[i], p + i);
      else p[i] = v[i];
    }
  }
}

// one lane per PX consecutive output pixels of a row; a workgroup = 256 lanes of ONE frame (its table entries are
// wave-uniform loads).  FRAMES: the 3 + Nl planes of `out`; FLOW: the two planes of `flow_out`.
template <int PX, bool FRAMES, bool FLOW>
__global__ __launch_bounds__(kBlock) void augment_clip_kernel(
    const uint32_t* __restrict__ clip, const float* __restrict__ flow, const int32_t* __restrict__ box,
    const uint8_t* __restrict__ flip, const float* __restrict__ jitter, const uint8_t* __restrict__ order,
    const float* __restrict__ zoom, float* __restrict__ out, float* __restrict__ flow_out, int T, int Nl, int Hd, int Wd,
    int Hf, int Wf, int Ho, int Wo, int tiles) {
  const unsigned f = blockIdx.x / (unsigned)tiles;  // frame (b, t)
  const unsigned b = f / (unsigned)T;
  const int wq = Wo / PX;
  const int e = (int)(blockIdx.x - f * (unsigned)tiles) * kBlock + (int)threadIdx.x;
  if (e >= Ho * wq) return;
  const int y = e / wq, x = (e - y * wq) * PX;
  // the box, clamped into the clip: no table value moves a read outside it
  const int top = min(max(box[b * 4 + 0], 0), Hd - 1), left = min(max(box[b * 4 + 1], 0), Wd - 1);
  const int hc = min(max(box[b * 4 + 2], 1), Hd - top), wc = min(max(box[b * 4 + 3], 1), Wd - left);
  const unsigned fl = flip[b];
  const bool lr = fl & 1u, tb = fl & 2u;
  const float ys = (float)hc / (float)Ho, xs = (float)wc / (float)Wo;
  const AugTap ty = aug_tap(tb ? Ho - 1 - y : y, ys, hc);
  AugTap tx[PX];
  float a00[PX], a01[PX], a10[PX], a11[PX];
  for (int p = 0; p < PX; ++p) {
    tx[p] = aug_tap(lr ? Wo - 1 - (x + p) : x + p, xs, wc);
    a00[p] = (1.0f - ty.f) * (1.0f - tx[p].f), a01[p] = (1.0f - ty.f) * tx[p].f;
    a10[p] = ty.f * (1.0f - tx[p].f), a11[p] = ty.f * tx[p].f;
  }
  const int64_t HWo = (int64_t)Ho * Wo, pix = (int64_t)y * Wo + x;

  if constexpr (FRAMES) {
    const uint32_t* r0 = clip + ((int64_t)f * Hd + top + ty.i0) * Wd + left;
    const uint32_t* r1 = clip + ((int64_t)f * Hd + top + ty.i1) * Wd + left;
    uint32_t w00[PX], w01[PX], w10[PX], w11[PX];
    for (int p = 0; p < PX; ++p)
      w00[p] = r0[tx[p].i0], w01[p] = r0[tx[p].i1], w10[p] = r1[tx[p].i0], w11[p] = r1[tx[p].i1];
    const unsigned ord = order[f];
    const unsigned ops = ord < 6u ? (unsigned)(kAugOrders >> (6u * ord)) & 63u : 0u;
    const float jb = jitter[b * 3 + 0], js = jitter[b * 3 + 1], jh = jitter[b * 3 + 2];
    float rgb[3][PX];
    for (int p = 0; p < PX; ++p) {
      float u[3];
      for (int c = 0; c < 3; ++c) {
        const unsigned sh = 8u * c;
        u[c] = ((a00[p] * (float)((w00[p] >> sh) & 255u) + a01[p] * (float)((w01[p] >> sh) & 255u)) +
                (a10[p] * (float)((w10[p] >> sh) & 255u) + a11[p] * (float)((w11[p] >> sh) & 255u))) / 255.0f;
      }
      if (ord < 6u) aug_jitter(u[0], u[1], u[2], ops, jb, js, jh);
      for (int c = 0; c < 3; ++c) rgb[c][p] = (u[c] - 0.5f) / 0.5f;
    }
    float* o = out + (int64_t)f * (3 + Nl) * HWo + pix;
    for (int c = 0; c < 3; ++c) aug_store<PX>(o + c * HWo, rgb[c]);
    o += 3 * HWo;
    for (int n = 0; n < Nl; ++n) {
      float v[PX];
      for (int p = 0; p < PX; ++p) {
        const float s = ((packed_class(w00[p]) == n ? a00[p] : 0.0f) + (packed_class(w01[p]) == n ? a01[p] : 0.0f)) +
                        ((packed_class(w10[p]) == n ? a10[p] : 0.0f) + (packed_class(w11[p]) == n ? a11[p] : 0.0f));
        v[p] = kLytLogit * (2.0f * s - 1.0f);
      }
      aug_store<PX>(o + n * HWo, v);
    }
  }

  if constexpr (FLOW) {
    // the four taps are positions of the Hd x Wd grid: each a bilinear sample of the (Hf, Wf) flow (the first resize)
    const bool same = Hf == Hd && Wf == Wd;
    const float fys = (float)Hf / (float)Hd, fxs = (float)Wf / (float)Wd;
    const AugTap g0 = aug_tap(top + ty.i0, fys, Hf), g1 = aug_tap(top + ty.i1, fys, Hf);
    const float z = zoom[b];
    const float* src = flow + (int64_t)f * 2 * Hf * Wf;
    float* o = flow_out + (int64_t)f * 2 * HWo + pix;
    for (int c = 0; c < 2; ++c, src += (int64_t)Hf * Wf) {
      float v[PX];
      for (int p = 0; p < PX; ++p) {
        float s[2][2];
        for (int i = 0; i < 2; ++i) {
          const AugTap gy = i ? g1 : g0;
          for (int j = 0; j < 2; ++j) {
            const AugTap gx = aug_tap(left + (j ? tx[p].i1 : tx[p].i0), fxs, Wf);
            const float* q0 = src + (int64_t)gy.i0 * Wf;
            if (same) {  // the first resize is the identity: its weights are (1, 0)
              s[i][j] = q0[gx.i0];
            } else {
              const float* q1 = src + (int64_t)gy.i1 * Wf;
              s[i][j] = ((1.0f - gy.f) * (1.0f - gx.f) * q0[gx.i0] + (1.0f - gy.f) * gx.f * q0[gx.i1]) +
                        (gy.f * (1.0f - gx.f) * q1[gx.i0] + gy.f * gx.f * q1[gx.i1]);
            }
          }
        }
        const float r = ((a00[p] * s[0][0] + a01[p] * s[0][1]) + (a10[p] * s[1][0] + a11[p] * s[1][1])) * z;
        v[p] = (c == 0 ? lr : tb) ? -r : r;
      }
      aug_store<PX>(o + c * HWo, v);
    }
  }
}

template <int PX, bool FRAMES, bool FLOW>
static void augment_launch(const uint8_t* clip, const float* flow, const int32_t* box, const uint8_t* flip,
                           const float* jitter, const uint8_t* order, const float* zoom, float* out, float* flow_out,
                           int64_t frames, int T, int Nl, int Hd, int Wd, int Hf, int Wf, int Ho, int Wo, int64_t tiles,
                           hipStream_t stream) {
  augment_clip_kernel<PX, FRAMES, FLOW><<<dim3((unsigned)(frames * tiles)), dim3(kBlock), 0, stream>>>(
      reinterpret_cast<const uint32_t*>(clip), flow, box, flip, jitter, order, zoom, out, flow_out, T, Nl, Hd, Wd, Hf, Wf,
      Ho, Wo, (int)tiles);
}

template <int PX>
static void augment_launches(const uint8_t* clip, const float* flow, const int32_t* box, const uint8_t* flip,
                             const float* jitter, const uint8_t* order, const float* zoom, float* out, float* flow_out,
                             int64_t frames, int T, int Nl, int Hd, int Wd, int Hf, int Wf, int Ho, int Wo, int64_t tiles,
                             hipStream_t stream) {
#define WALDO_AUG_ARGS clip, flow, box, flip, jitter, order, zoom, out, flow_out, frames, T, Nl, Hd, Wd, Hf, Wf, Ho, Wo, \
                       tiles, stream
  if (!flow) {
    augment_launch<PX, true, false>(WALDO_AUG_ARGS);
  } else if (WALDO_AUG_LAUNCHES == 2) {
    augment_launch<PX, true, false>(WALDO_AUG_ARGS);
    augment_launch<PX, false, true>(WALDO_AUG_ARGS);
  } else {
    augment_launch<PX, true, true>(WALDO_AUG_ARGS);
  }
#undef WALDO_AUG_ARGS
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_augment_clip_fwd(const uint8_t* clip, const float* flow, const int32_t* box, const uint8_t* flip,
                                      const float* jitter, const uint8_t* order, const float* zoom, float* out,
                                      float* flow_out, int B, int T, int Nl, int Hd, int Wd, int Hf, int Wf, int Ho,
                                      int Wo, waldo_stream_t stream) {
  const char* fn = "waldo_augment_clip_fwd";
  const bool with_flow = flow || flow_out;
  auto size_ok = [](int v) { return v >= 1 && v <= kAugMaxSize; };
  if (B < 0 || T < 0 || Nl < 0 || Nl > kMaxPackedCls || !size_ok(Hd) || !size_ok(Wd) || !size_ok(Ho) || !size_ok(Wo) ||
      (with_flow && (!size_ok(Hf) || !size_ok(Wf)))) {
    set_error("%s: bad shape B=%d T=%d Nl=%d clip %dx%d flow %dx%d out %dx%d (0 <= Nl <= %d, sizes in [1, %d])", fn, B, T,
              Nl, Hd, Wd, Hf, Wf, Ho, Wo, kMaxPackedCls, kAugMaxSize);
    return WALDO_EINVAL;
  }
  if (Ho < Hd || Wo < Wd) {
    set_error("%s: out %dx%d is smaller than the clip %dx%d: a downsample needs an antialiasing filter", fn, Ho, Wo, Hd,
              Wd);
    return WALDO_EINVAL;
  }
  if (with_flow && (Hf > Hd || Wf > Wd)) {
    set_error("%s: flow larger than the clip (%dx%d > %dx%d)", fn, Hf, Wf, Hd, Wd);
    return WALDO_EINVAL;
  }
  const int64_t frames = (int64_t)B * T;
  if (frames == 0) return WALDO_OK;
  if (!clip || !box || !flip || !jitter || !order || !zoom || !out || (with_flow && (!flow || !flow_out))) {
    set_error("%s: null pointer (only flow and flow_out, together, may be null)", fn);
    return WALDO_EINVAL;
  }
  const bool vec = WALDO_AUG_PX == 4 && Wo % 4 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)flow_out % 16 == 0;
  const int64_t tiles = ((int64_t)Ho * (Wo / (vec ? 4 : 1)) + kBlock - 1) / kBlock;
  if (frames * tiles > 2147483647) {
    set_error("%s: problem too large for one launch (%lld workgroups)", fn, (long long)(frames * tiles));
    return WALDO_EINVAL;
  }
  if (vec)
    augment_launches<4>(clip, flow, box, flip, jitter, order, zoom, out, flow_out, frames, T, Nl, Hd, Wd, Hf, Wf, Ho, Wo,
                        tiles, (hipStream_t)stream);
  else
    augment_launches<1>(clip, flow, box, flip, jitter, order, zoom, out, flow_out, frames, T, Nl, Hd, Wd, Hf, Wf, Ho, Wo,
                        tiles, (hipStream_t)stream);
  return launch_status(fn);
}
