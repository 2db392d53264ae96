// Host wrappers of the fused warp/composite kernels for one padded layer count LP and layer element type T (float,
// __bf16, _Float16).  Each compile unit warp_composite_lp<LP>[_bf16 | _f16].hip holds the explicit instances of one
// (LP, T), so that the variants compile in parallel.  A 16-bit stack is served by the staged forward and the
// two-kernel backward only (instances for LP <= kBwd2MaxLayers); the C-ABI entry points check its shape first.
#pragma once
#include "warp_composite_kernels.hip.h"

namespace waldo {

template <int LP, typename T>
void wc_fwd(bool k19, const T* layers, const float* basis_t, const float* mapping, const float* inv_kernel,
            const float* src_pts, const float* occ, float* rgb, float* alpha, int F, int L, int H, int W, int K3,
            float delta, hipStream_t st) {
  if (k19)
    launch_fwd<LP, 19, true>(layers, basis_t, mapping, inv_kernel, src_pts, occ, rgb, alpha, F, L, H, W, K3, delta,
                             st);
  else if constexpr (std::is_same_v<T, float>)
    launch_fwd<LP, 32, false>(layers, basis_t, mapping, nullptr, nullptr, occ, rgb, alpha, F, L, H, W, K3, delta, st);
}

// `workspace` != nullptr selects the two-kernel backward (compiled for L <= kBwd2MaxLayers, K3 == 19); with
// `occ_slab` its deterministic grad_occ (launch_bwd2)
template <int LP, typename T>
void wc_bwd(bool k19, const T* layers, const float* basis_t, const float* mapping, const float* occ,
            const float* grad_rgb, const float* grad_alpha, T* grad_layers, float* grad_mapping, float* grad_occ,
            void* workspace, int F, int L, int H, int W, int K3, float delta, hipStream_t st, float* occ_slab) {
  if constexpr (LP <= kBwd2MaxLayers) {
    if (k19 && workspace != nullptr) {
      launch_bwd2<LP>(layers, basis_t, mapping, occ, grad_rgb, grad_alpha, workspace, grad_layers, grad_mapping,
                      grad_occ, F, L, H, W, delta, st, occ_slab);
      return;
    }
  }
  if constexpr (std::is_same_v<T, float>) {
    if (k19)
      launch_bwd<LP, 19>(layers, basis_t, mapping, occ, grad_rgb, grad_alpha, grad_layers, grad_mapping, grad_occ, F,
                         L, H, W, K3, delta, st);
    else
      launch_bwd<LP, 32>(layers, basis_t, mapping, occ, grad_rgb, grad_alpha, grad_layers, grad_mapping, grad_occ, F,
                         L, H, W, K3, delta, st);
  }
}

}  // namespace waldo
