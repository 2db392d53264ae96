// The raw path with an fp16 `raw` (flow_ctx_kernels.hip.h): a compile unit of its own
#include "flow_ctx_kernels.hip.h"

namespace waldo {
template decltype(flow_ctx_warp_raw<_Float16>) flow_ctx_warp_raw<_Float16>;
template decltype(frame_warp_fuse_raw<_Float16, float>) frame_warp_fuse_raw<_Float16, float>;
}  // namespace waldo
