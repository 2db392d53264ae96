// The packed clip's flow_ctx_alpha and its frame warp with an fp32 `raw` (flow_ctx_kernels.hip.h): a compile unit of
// their own
#include "flow_ctx_kernels.hip.h"

namespace waldo {
template decltype(flow_ctx_alpha_launch<uint32_t>) flow_ctx_alpha_launch<uint32_t>;
template decltype(frame_warp_fuse_raw<float, uint32_t>) frame_warp_fuse_raw<float, uint32_t>;
}  // namespace waldo
