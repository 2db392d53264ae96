// The plane norm's kernels for _Float16 buffers (plane_norm_kernels.hip.h): a compile unit of its own
#include "plane_norm_kernels.hip.h"

namespace waldo {
WALDO_PLANE_NORM_INSTANCES(, _Float16)
}  // namespace waldo
