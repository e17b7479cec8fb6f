// kv_opt_adam.hip — the plain Adam apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_ADAM
#include "kv_opt_unit.h"
