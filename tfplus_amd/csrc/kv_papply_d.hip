// kv_papply_d.hip — instantiates k_papply (kv_papply.h: partition pass + optimizer apply in one launch) and k_uapply
// (kv_uapply.h) for FTRL-V2 and group FTRL-V2.  A translation unit of its own (see kv_papply_a.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/kvhip.h"

namespace {
#include "kv_device.h"
#include "kv_kernels.h"
#include "kv_fused.h"
#include "kv_papply.h"
#include "kv_uapply.h"
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int kvp_launch_papply_d(int opt, const void* wd_, const void* pa_, int mode,
                                                                      void* stream, const void* md_, int ntab) {
  const WsDev& wd = *static_cast<const WsDev*>(wd_);
  const PartArgs& pa = *static_cast<const PartArgs*>(pa_);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MultiDesc* md = static_cast<const MultiDesc*>(md_);
  if (opt == OPT_FTRL_V2) return launch_papply_t<OPT_FTRL_V2>(wd, pa, mode, s, md, ntab);
  if (opt == OPT_GROUP_FTRL_V2) return launch_papply_t<OPT_GROUP_FTRL_V2>(wd, pa, mode, s, md, ntab);
  return KV_INTERNAL;
}

// k_uapply (kv_uapply.h): the apply on unique ids + pre-summed rows, one launch
extern "C" __attribute__((visibility("hidden"))) int kvp_launch_uapply_d(int opt, const void* pa_, const void* ids, int ids32,
                                                                      long long n, void* stream, const void* md_, int ntab) {
  const PartArgs& pa = *static_cast<const PartArgs*>(pa_);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MultiDesc* md = static_cast<const MultiDesc*>(md_);
  if (opt == OPT_FTRL_V2) return launch_uapply_t<OPT_FTRL_V2>(pa, ids, ids32, n, s, md, ntab);
  if (opt == OPT_GROUP_FTRL_V2) return launch_uapply_t<OPT_GROUP_FTRL_V2>(pa, ids, ids32, n, s, md, ntab);
  return KV_INTERNAL;
}
