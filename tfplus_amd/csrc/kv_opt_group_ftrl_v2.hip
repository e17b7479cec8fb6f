// kv_opt_group_ftrl_v2.hip — the group FTRL-V2 apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_GROUP_FTRL_V2
#include "kv_opt_unit.h"
