// kv_opt_adam_v4.hip — the GroupAdam V4 apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_ADAM_V4
#include "kv_opt_unit.h"
