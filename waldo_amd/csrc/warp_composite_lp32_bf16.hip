// The fused warp/composite for padded layer count 32, bf16 layer stack (warp_composite_inst.hip.h)
#include "warp_composite_inst.hip.h"

namespace waldo {
template decltype(wc_fwd<32, __bf16>) wc_fwd<32, __bf16>;
}  // namespace waldo
