// The packed clip's frame warp of flow_ctx.hip with an fp16 `raw`: a compile unit of its own
#define WALDO_FC_PACKED 1
#define WALDO_FC_RAW_HALF _Float16
#define WALDO_FC_RAW_SUFFIX f16
#include "flow_ctx.hip"
