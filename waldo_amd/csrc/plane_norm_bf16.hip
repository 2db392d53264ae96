// The plane norm's kernels for __bf16 buffers (plane_norm_kernels.hip.h): a compile unit of its own
#include "plane_norm_kernels.hip.h"

namespace waldo {
WALDO_PLANE_NORM_INSTANCES(, __bf16)
}  // namespace waldo
