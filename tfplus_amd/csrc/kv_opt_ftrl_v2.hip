// kv_opt_ftrl_v2.hip — the FTRL-V2 apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_FTRL_V2
#include "kv_opt_unit.h"
