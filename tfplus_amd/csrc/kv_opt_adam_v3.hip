// kv_opt_adam_v3.hip — the GroupAdam V3 apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_ADAM_V3
#include "kv_opt_unit.h"
