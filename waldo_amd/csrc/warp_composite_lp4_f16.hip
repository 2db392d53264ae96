// The fused warp/composite for padded layer count 4, f16 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<4, _Float16>) wc_fwd<4, _Float16>;
template decltype(wc_bwd<4, _Float16>) wc_bwd<4, _Float16>;
}  // namespace waldo
