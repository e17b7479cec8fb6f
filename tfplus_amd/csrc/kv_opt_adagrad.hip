// kv_opt_adagrad.hip — the Adagrad apply kernels (kv_opt_unit.h)
#define KV_OPT OPT_ADAGRAD
#include "kv_opt_unit.h"
