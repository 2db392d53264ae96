// The bf16 instances of the raw path of flow_ctx.hip (a 16-bit `raw`): a compile unit of their own
#define WALDO_FC_RAW_HALF __bf16
#define WALDO_FC_RAW_SUFFIX bf16
#include "flow_ctx.hip"
