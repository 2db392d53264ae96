// The packed clip's frame warp with an fp16 `raw` (flow_ctx_kernels.hip.h): a compile unit of its own
#include "flow_ctx_kernels.hip.h"

namespace waldo {
template decltype(frame_warp_fuse_raw<_Float16, uint32_t>) frame_warp_fuse_raw<_Float16, uint32_t>;
}  // namespace waldo
