// The packed clip's frame warp of flow_ctx.hip with a bf16 `raw`: a compile unit of its own
#define WALDO_FC_PACKED 1
#define WALDO_FC_RAW_HALF __bf16
#define WALDO_FC_RAW_SUFFIX bf16
#include "flow_ctx.hip"
