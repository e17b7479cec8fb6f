// kv_opt_unit.h — the body of an optimizer's instantiation unit, kv_opt_<name>.hip, which defines KV_OPT (an OPT_*) and
// includes this: the optimizer's sorted-position (k_apply / k_apply_fin), entry-list (k_papply) and unique-ids (k_uapply)
// apply kernels behind the launchers of kv_launch.h.  One unit per optimizer, so that `make -j` builds them side by side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/kvhip.h"
#include "kv_launch.h"

using namespace kvhip_internal;

namespace {
#include "kv_device.h"
#include "kv_key_update.h"
#include "kv_kernels.h"
#include "kv_fused.h"
#include "kv_papply.h"
#include "kv_uapply.h"
}  // namespace

namespace kvhip_internal {
template <>
int launch_sorted_apply<KV_OPT>(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab,
                                unsigned nchunks, int span) {
  return launch_apply_t<MODE_APPLY, KV_OPT>(wd, pa, s, md, ntab, nchunks, span);
}
template <>
int launch_papply<KV_OPT>(const WsDev& wd, const PartArgs& pa, int mode, hipStream_t s, const MultiDesc* md, int ntab) {
  return launch_papply_t<KV_OPT>(wd, pa, mode, s, md, ntab);
}
template <>
int launch_uapply<KV_OPT>(const PartArgs& pa, const void* ids, int ids32, long long n, hipStream_t s, const MultiDesc* md,
                          int ntab, const long long* n_dev) {
  return launch_uapply_t<KV_OPT>(pa, ids, ids32, n, s, md, ntab, n_dev);
}
}  // namespace kvhip_internal
