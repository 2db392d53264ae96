// The f16 instances of the raw path of flow_ctx.hip (a 16-bit `raw`): a compile unit of their own
#define WALDO_FC_RAW_HALF _Float16
#define WALDO_FC_RAW_SUFFIX f16
#include "flow_ctx.hip"
