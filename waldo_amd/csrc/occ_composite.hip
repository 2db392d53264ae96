// A6: occlusion product  out_j = alpha_j * prod_i (1 - alpha_i * occ[i,j])  over L layers per
// pixel -- the (1 - alpha * occ).prod(dim) * alpha pattern of models/nets/lvd.py:651-652, 686,
// 764-765, 809 (spec: LVD.reduce_comp, lvd.py:109-111).  The reference materialises an
// (L, L, h, w) tensor per map; here every thread keeps its L alphas in registers, occ is
// wave-uniform (scalar cache), and nothing of size L*L*h*w exists.
#include "det_common.hip.h"
#include "flow_ctx_common.hip.h"

namespace waldo {

template <int LP>
__global__ __launch_bounds__(kBlock) void occ_composite_fwd_kernel(
    const float* __restrict__ alpha, const float* __restrict__ occ, float* __restrict__ out,
    int L, int64_t HW, int tiles, int64_t occ_div) {
  const int64_t m = blockIdx.x / tiles;
  const int64_t p = (int64_t)(blockIdx.x % tiles) * kBlock + threadIdx.x;
  if (p >= HW) return;
  const float* ap = alpha + m * L * HW + p;
  const float* oc = occ + (m / occ_div) * L * L;
  float a[LP];
#pragma unroll
  for (int l = 0; l < LP; ++l) a[l] = (l < L) ? ap[(int64_t)l * HW] : 0.0f;
#pragma unroll
  for (int j = 0; j < LP; ++j) {
    if (j < L) {
      float pr = 1.0f;
#pragma unroll
      for (int i = 0; i < LP; ++i)
        if (i < L) pr *= (1.0f - a[i] * oc[i * L + j]);
      out[(m * L + j) * HW + p] = a[j] * pr;
    }
  }
}

// Backward.  grad_alpha is per pixel; grad_occ[m_occ][i][j] is a sum over ALL pixels of all maps that
// share the matrix.  A workgroup walks `tiles_per_block` pixel tiles of one map (BwdTileWalk): per tile and
// column j every wave reduces its 64 pixels (wave_transpose_reduce: lane bitrev(i) ends up with row i) and
// adds the result to ITS OWN row of an LDS table (WaveTable) -- no atomics, no barrier; at the end
// the four rows are summed in a fixed order and leave the workgroup as ONE float atomic per matrix entry (the
// first version issued one per wave, tile and entry: thousands of waves on a few hundred addresses,
// 0.37 ms for 22 MB at the LVD recipe -- the pattern measured 14x below the streaming atomic rate).
// DET (deterministic mode): grad_occ is a slab of one L x L row per workgroup, stored, not added (det_common.hip.h).
template <int LP, bool DET = false>
__global__ __launch_bounds__(kBlock) void occ_composite_bwd_kernel(
    const float* __restrict__ alpha, const float* __restrict__ occ,
    const float* __restrict__ grad_out, float* __restrict__ grad_alpha,
    float* __restrict__ grad_occ, int L, int64_t HW, int tiles, int tiles_per_block, int groups,
    int64_t occ_div) {
  const int64_t m = blockIdx.x / groups;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const float* oc = occ + (m / occ_div) * L * L;
  __shared__ float acc_s[4][LP * LP];
  const WaveTable<LP * LP> acc{acc_s};
  if (grad_occ != nullptr) acc.zero(wave, lane);
  for (BwdTileWalk w(tiles, tiles_per_block, groups); w.more();) {
    const BwdTile q = w.next<false>(HW);
    const float* ap = alpha + m * L * HW + q.pc;
    float a[LP], ga[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) {
      a[l] = (l < L) ? ap[(int64_t)l * HW] : 0.0f;
      ga[l] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < LP; ++j) {
      if (j < L) {
        float tf[LP], ex[LP];
        float pre = 1.0f;
#pragma unroll
        for (int i = 0; i < LP; ++i) {
          tf[i] = (i < L) ? (1.0f - a[i] * oc[i * L + j]) : 1.0f;
          ex[i] = pre;
          pre *= tf[i];
        }
        float suf = 1.0f;
#pragma unroll
        for (int i = LP - 1; i >= 0; --i) {
          ex[i] *= suf;
          suf *= tf[i];
        }
        const float go = q.live ? grad_out[(m * L + j) * HW + q.pc] : 0.0f;
        ga[j] = fmaf(go, pre, ga[j]);
        const float gaj = go * a[j];
        float gocc[LP];
#pragma unroll
        for (int i = 0; i < LP; ++i) {
          if (i < L) {
            ga[i] = fmaf(-gaj * oc[i * L + j], ex[i], ga[i]);
            gocc[i] = -gaj * a[i] * ex[i];
          } else {
            gocc[i] = 0.0f;
          }
        }
        if (grad_occ != nullptr) {
          const float red = wave_transpose_reduce<LP>(gocc, lane);
          const int i = bitrev6(lane);
          if (i < L) acc.row(wave)[i * LP + j] += red;  // one lane per entry: plain read-modify-write
        }
      }
    }
    if (q.live) {
#pragma unroll
      for (int l = 0; l < LP; ++l)
        if (l < L) grad_alpha[(m * L + l) * HW + q.p] = ga[l];
    }
  }
  if (grad_occ != nullptr) {
    __syncthreads();
    acc.template flush<DET>(grad_occ, L * L, m / occ_div, PaddedSquare<LP>{L});
  }
}

static int check_occ(const char* fn, int64_t M, int L, int64_t HW, int64_t occ_div) {
  if (M < 0 || L < 1 || L > 32 || HW < 1 || occ_div < 1) {
    set_error("%s: bad shape M=%lld L=%d HW=%lld occ_div=%lld (need 1<=L<=32)", fn, (long long)M,
              L, (long long)HW, (long long)occ_div);
    return WALDO_EINVAL;
  }
  if (M * ((HW + kBlock - 1) / kBlock) > 2147483647) {
    set_error("%s: problem too large for one launch", fn);
    return WALDO_EINVAL;
  }
  return WALDO_OK;
}

}  // namespace waldo

using namespace waldo;

extern "C" int waldo_occ_composite_fwd(const float* alpha, const float* occ, float* out,
                                       int64_t M, int L, int64_t HW, int64_t occ_div,
                                       waldo_stream_t stream) {
  int rc = check_occ("waldo_occ_composite_fwd", M, L, HW, occ_div);
  if (rc) return rc;
  if (M == 0) return WALDO_OK;
  if (!alpha || !occ || !out) {
    set_error("waldo_occ_composite_fwd: null pointer");
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((HW + kBlock - 1) / kBlock);
  with_padded_layers(L, [&](auto lp) {
    hipLaunchKernelGGL((occ_composite_fwd_kernel<decltype(lp)::value>), dim3((unsigned)(M * tiles)), dim3(kBlock), 0, st,
                       alpha, occ, out, L, HW, tiles, occ_div);
  });
  return launch_status("waldo_occ_composite_fwd");
}

static int occ_bwd_tiles_per_block(int64_t M, int tiles, bool want_occ) {
  // several pixel tiles per workgroup (fewer atomics per matrix entry) while keeping >= ~1024
  // workgroups in flight
  int tpb = (int)min((int64_t)16, max((int64_t)1, (M * tiles) / 1024));
  if (!want_occ) tpb = 1;
  return tpb;
}

// ---- deterministic mode: grad_occ (ceil(M / occ_div) matrices) OVERWRITTEN; slab form
extern "C" int64_t waldo_occ_composite_bwd_det_workspace_bytes(int64_t M, int L, int64_t HW) {
  if (M < 0 || L < 1 || L > 32 || HW < 1) return 0;
  const int tiles = (int)((HW + kBlock - 1) / kBlock);
  return round256(M * ((tiles + kDetTilesPerBlock - 1) / kDetTilesPerBlock) * L * L * 4);
}

// det: the *_det entry point -- the workgroups store their partial matrices to a slab in the workspace and a reduction
// overwrites grad_occ; without grad_occ the two modes are the same launch
static int occ_composite_bwd(const char* fn, const float* alpha, const float* occ, const float* grad_out,
                             float* grad_alpha, float* grad_occ, int64_t M, int L, int64_t HW, int64_t occ_div,
                             void* workspace, int64_t workspace_bytes, waldo_stream_t stream, bool det) {
  int rc = check_occ(fn, M, L, HW, occ_div);
  if (rc) return rc;
  const bool slabs = det && grad_occ != nullptr;
  const int64_t need = slabs ? waldo_occ_composite_bwd_det_workspace_bytes(M, L, HW) : 0;
  if (need > 0 && (rc = check_workspace(fn, workspace, workspace_bytes, need))) return rc;
  if (M == 0) return WALDO_OK;
  if (!alpha || !occ || !grad_out || !grad_alpha) {
    set_error("%s: null pointer", fn);
    return WALDO_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((HW + kBlock - 1) / kBlock);
  const int tpb = slabs ? kDetTilesPerBlock : occ_bwd_tiles_per_block(M, tiles, grad_occ != nullptr);
  const int groups = (tiles + tpb - 1) / tpb;
  float* slab = reinterpret_cast<float*>(workspace);
  auto pixels = [&](auto dt, float* table) {  // table: grad_occ itself (atomics), or the slab
    with_padded_layers(L, [&](auto lp) {
      hipLaunchKernelGGL((occ_composite_bwd_kernel<decltype(lp)::value, decltype(dt)::value>), dim3((unsigned)(M * groups)),
                         dim3(kBlock), 0, st, alpha, occ, grad_out, grad_alpha, table, L, HW, tiles, tpb, groups, occ_div);
    });
  };
  if (!slabs) pixels(std::false_type{}, grad_occ);
  else pixels(std::true_type{}, slab);
  if (slabs) {
    // matrix d sums the workgroups of maps d * occ_div .. (d + 1) * occ_div - 1: consecutive rows of the slab
    const int64_t D = (M + occ_div - 1) / occ_div;
    const int nparts = (int)((occ_div < M ? occ_div : M) * groups);
    slab_reduce(slab, grad_occ, D, nparts, L * L, SlabPlain{M * groups, D, D}, st);
  }
  return launch_status(fn);
}

extern "C" int waldo_occ_composite_bwd(const float* alpha, const float* occ,
                                       const float* grad_out, float* grad_alpha, float* grad_occ,
                                       int64_t M, int L, int64_t HW, int64_t occ_div,
                                       waldo_stream_t stream) {
  return occ_composite_bwd("waldo_occ_composite_bwd", alpha, occ, grad_out, grad_alpha, grad_occ, M, L, HW, occ_div,
                           nullptr, 0, stream, false);
}

extern "C" int waldo_occ_composite_bwd_det(const float* alpha, const float* occ, const float* grad_out,
                                           float* grad_alpha, float* grad_occ, int64_t M, int L, int64_t HW,
                                           int64_t occ_div, void* workspace, int64_t workspace_bytes,
                                           waldo_stream_t stream) {
  return occ_composite_bwd("waldo_occ_composite_bwd_det", alpha, occ, grad_out, grad_alpha, grad_occ, M, L, HW, occ_div,
                           workspace, workspace_bytes, stream, true);
}
