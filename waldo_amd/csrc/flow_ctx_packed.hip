// The packed clip's passes of flow_ctx.hip with an fp32 `raw` (frame warp) and its flow_ctx_alpha: a compile unit of
// their own
#define WALDO_FC_PACKED 1
#include "flow_ctx.hip"
