// kv_opt_ftrl.hip — the SparseGroupFtrl apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_FTRL
#include "kv_opt_unit.h"
