// kv_opt_radam.hip — the plain RectifiedAdam apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_RADAM
#include "kv_opt_unit.h"
