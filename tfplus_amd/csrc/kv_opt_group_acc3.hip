// kv_opt_group_acc3.hip — the group Momentum / group Adadelta apply kernels, one family (kv_opt_unit.h)
#define KV_OPT OPT_GROUP_ACC3
#include "kv_opt_unit.h"
