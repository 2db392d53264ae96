// The fused warp/composite for padded layer count 4, fp32 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<4, float>) wc_fwd<4, float>;
template decltype(wc_bwd<4, float>) wc_bwd<4, float>;
}  // namespace waldo
