// The fused warp/composite for padded layer count 12, bf16 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<12, __bf16>) wc_fwd<12, __bf16>;
template decltype(wc_bwd<12, __bf16>) wc_bwd<12, __bf16>;
}  // namespace waldo
