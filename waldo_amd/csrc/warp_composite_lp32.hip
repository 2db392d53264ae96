// The fused warp/composite for padded layer count 32, fp32 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<32, float>) wc_fwd<32, float>;
template decltype(wc_bwd<32, float>) wc_bwd<32, float>;
}  // namespace waldo
