// The fused warp/composite for padded layer count 12, fp32 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<12, float>) wc_fwd<12, float>;
template decltype(wc_bwd<12, float>) wc_bwd<12, float>;
}  // namespace waldo
