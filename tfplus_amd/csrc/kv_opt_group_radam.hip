// kv_opt_group_radam.hip — the group RectifiedAdam apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_GROUP_RADAM
#include "kv_opt_unit.h"
