// kv_opt_group_adam4.hip — the group AMSGrad / group AdaBelief apply kernels, one family (kv_opt_unit.h)
#define KV_OPT OPT_GROUP_ADAM4
#include "kv_opt_unit.h"
