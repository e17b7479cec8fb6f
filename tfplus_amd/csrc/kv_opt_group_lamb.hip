// kv_opt_group_lamb.hip — the group LAMB apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_GROUP_LAMB
#include "kv_opt_unit.h"
