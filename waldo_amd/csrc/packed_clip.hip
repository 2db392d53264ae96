// The packed clip (packed_clip.hip.h): its unpacked fp32 form, and the low-resolution copy of its layout channels that
// Warper.grid_to_flow[_ctx] takes (waldo_downscale_frames_fwd's packed twin).  The frame warp and the first
// full-resolution pass read the packed clip in flow_ctx_kernels.hip.h (flow_ctx_packed*.hip).
#include "packed_clip.hip.h"

namespace waldo {

// one thread per pixel: its word in, its 3 + Nl channels out (one coalesced plane store each).  A workgroup = 256
// consecutive pixels of ONE frame; the RGB table in LDS.
__global__ __launch_bounds__(kBlock) void unpack_clip_kernel(const uint32_t* __restrict__ clip,
                                                             const float* __restrict__ rgb_table,
                                                             float* __restrict__ out, int C, int64_t HWd, int tiles) {
  __shared__ float stab[kRgbTable];
  static_assert(kBlock == kRgbTable, "one table entry per thread");
  stab[threadIdx.x] = rgb_table[threadIdx.x];
  __syncthreads();
  const unsigned f = blockIdx.x / (unsigned)tiles;  // frame (b, t)
  const int64_t e = (int64_t)(blockIdx.x - f * (unsigned)tiles) * kBlock + threadIdx.x;
  if (e >= HWd) return;
  const uint32_t w = clip[(int64_t)f * HWd + e];
  float* o = out + (int64_t)f * C * HWd + e;
  for (int c = 0; c < C; ++c) o[(int64_t)c * HWd] = packed_channel(stab, w, c);
}

// A7 (time_gather.hip: downscale_frames_kernel) on the packed clip: the four words of an output pixel's 2 x 2 middle
// texels are read ONCE and all Nl layout channels are written from them (one thread per output pixel of one frame) --
// the fp32 kernel reads the four texels of every one of the Nl planes.  The same down_mean4 of the same +-5: the same bits.
__global__ __launch_bounds__(kBlock) void downscale_frames_packed_kernel(const uint32_t* __restrict__ clip,
                                                                         float* __restrict__ out, int T, int Tw, int Nl,
                                                                         int H, int W, int S, int tiles) {
  typedef uint32_t u32x2_d __attribute__((ext_vector_type(2)));
  const unsigned n = blockIdx.x / (unsigned)tiles;  // (b, t) of the output, t < Tw
  const unsigned e = (blockIdx.x - n * (unsigned)tiles) * kBlock + threadIdx.x;
  if (e >= (unsigned)(H * W)) return;
  const unsigned y = e / (unsigned)W, x = e - y * (unsigned)W;
  const int64_t b = n / (unsigned)Tw, t = n % (unsigned)Tw;
  const int64_t Wd = (int64_t)W * S, Hd = (int64_t)H * S;
  const uint32_t* src = clip + ((b * T + t) * Hd + ((int64_t)y * S + S / 2 - 1)) * Wd + (int64_t)x * S + S / 2 - 1;
  const u32x2_d r0 = *reinterpret_cast<const u32x2_d*>(src);
  const u32x2_d r1 = *reinterpret_cast<const u32x2_d*>(src + Wd);
  float* o = out + (int64_t)n * Nl * H * W + e;
  for (int c = 0; c < Nl; ++c)
    o[(int64_t)c * H * W] = down_mean4(packed_lyt(r0[0], c), packed_lyt(r0[1], c), packed_lyt(r1[0], c),
                                       packed_lyt(r1[1], c));
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_unpack_clip_fwd(const uint8_t* clip, const float* rgb_table, float* out, int B, int T, int Nl,
                                     int Hd, int Wd, waldo_stream_t stream) {
  const char* fn = "waldo_unpack_clip_fwd";
  if (B < 0 || T < 0 || Nl < 0 || Nl > kMaxPackedCls || Hd < 0 || Wd < 0) {
    set_error("%s: bad shape B=%d T=%d Nl=%d Hd=%d Wd=%d (0 <= Nl <= %d)", fn, B, T, Nl, Hd, Wd, kMaxPackedCls);
    return WALDO_EINVAL;
  }
  const int64_t frames = (int64_t)B * T, HWd = (int64_t)Hd * Wd;
  if (frames * HWd == 0) return WALDO_OK;
  if (!clip || !rgb_table || !out) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const int64_t tiles = (HWd + kBlock - 1) / kBlock;
  if (frames * tiles > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  unpack_clip_kernel<<<dim3((unsigned)(frames * tiles)), dim3(kBlock), 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t*>(clip), rgb_table, out, 3 + Nl, HWd, (int)tiles);
  return launch_status(fn);
}

extern "C" int waldo_downscale_frames_packed_fwd(const uint8_t* clip, float* out, int B, int T, int Tw, int Nl, int H,
                                                 int W, int S, waldo_stream_t stream) {
  const char* fn = "waldo_downscale_frames_packed_fwd";
  if (B < 0 || T < 1 || Tw < 0 || Tw > T || Nl < 1 || Nl > kMaxPackedCls || H < 1 || W < 1 || S < 2 || (S & (S - 1)) ||
      (int64_t)H * S > 32767 || (int64_t)W * S > 32767) {
    set_error("%s: bad shape B=%d T=%d Tw=%d Nl=%d H=%d W=%d S=%d (1 <= Nl <= %d, S: a power of two >= 2)", fn, B, T, Tw,
              Nl, H, W, S, kMaxPackedCls);
    return WALDO_EINVAL;
  }
  const int64_t frames = (int64_t)B * Tw;
  if (frames == 0) return WALDO_OK;
  if (!clip || !out) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  const int64_t tiles = ((int64_t)H * W + kBlock - 1) / kBlock;
  if (frames * tiles > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  downscale_frames_packed_kernel<<<dim3((unsigned)(frames * tiles)), dim3(kBlock), 0, (hipStream_t)stream>>>(
      reinterpret_cast<const uint32_t*>(clip), out, T, Tw, Nl, H, W, S, (int)tiles);
  return launch_status(fn);
}
