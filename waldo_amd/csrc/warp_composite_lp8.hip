// The fused warp/composite for padded layer count 8, fp32 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<8, float>) wc_fwd<8, float>;
template decltype(wc_bwd<8, float>) wc_bwd<8, float>;
}  // namespace waldo
