// kv_sums.hip — the optimizer-free launchers of kv_launch.h: the tile sums of the entry-list pipeline (k_tsum, k_ltsum), the
// table-less forms of its partition pass (k_papply_uniq: the distinct ids of a batch numbered — the sharded route, kv_unique,
// kv_dedup_segment_sum; k_papply_dedup: the gradient rows summed per distinct id) and the plain segment fold of the
// sorted-position pipeline (k_apply in MODE_DEDUP).  A translation unit of its own, next to the optimizers' (kv_opt_unit.h).
// Each launcher takes its kernel's row geometry from the one table of kv_row_geom.h (with_row_geom).
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
}  // namespace

namespace kvhip_internal {

// k_tsum: same row geometry as k_papply.  grid = ntiles blocks of TBC threads.  md: wd = the largest ntiles.
int launch_tsum(const TableDev& td, const WsDev& wd, const float* grad, hipStream_t s, const MultiDesc* md, int ntab) {
  return with_row_geom<ENTRY_MAX_Q>(td.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    if (md) k_tsum_multi<V, LPR, K><<<dim3(wd.ntiles, (unsigned)ntab), TBC, 0, s>>>(md);
    else k_tsum<V, LPR, K><<<wd.ntiles, TBC, (size_t)TILE * 4, s>>>(td, wd, grad);
    return KV_OK;
  });
}

// k_ltsum: one block per tile
template <typename IdT>
static int launch_ltsum_t(const TableDev& td, const WsDev& wd, const IdT* ids, long long n, int det, const float* grad,
                          hipStream_t s) {
  const size_t sh = ltile_smem_bytes();
  return with_row_geom<ENTRY_MAX_Q>(td.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    k_ltsum<IdT, V, LPR, K><<<(int)wd.ntiles, TBT, sh, s>>>(td, wd, ids, nullptr, n, det, grad);
    return KV_OK;
  });
}
int launch_ltsum(const TableDev& td, const WsDev& wd, const void* ids, int ids_kind, long long n, int det, const float* grad,
                 hipStream_t s) {
  if (ids_kind == 1) return launch_ltsum_t<int>(td, wd, static_cast<const int*>(ids), n, det, grad, s);
  return launch_ltsum_t<long long>(td, wd, static_cast<const long long*>(ids), n, det, grad, s);
}

// PA_UNIQUE: one kernel whatever the dim; PA_DEDUP: by row geometry
int launch_papply_ud(const WsDev& wd, const PartArgs& pa, int mode, hipStream_t s, const MultiDesc* md, int ntab) {
  const size_t sh = (size_t)wd.ntiles * 4 + 32;
  if (mode == PA_UNIQUE) {
    if (md) k_papply_uniq_multi<<<dim3(wd.P, (unsigned)ntab), 256, sh, s>>>(md, mode);
    else if (wd.P <= 512u && !pa.det) k_papply_uniq<512><<<(int)wd.P, 512, sh, s>>>(wd, pa, mode);
    else k_papply_uniq<256><<<(int)wd.P, 256, sh, s>>>(wd, pa, mode);
    return KV_OK;
  }
  if (mode != PA_DEDUP) return KV_UNIMPLEMENTED;
  return with_row_geom<ENTRY_MAX_Q>(pa.tv.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    if (md) k_papply_dedup_multi<V, LPR, K><<<dim3(wd.P, (unsigned)ntab), 256, sh, s>>>(md);
    else if (pa.dd_number) {
      if (wd.P <= 512u && !pa.det) k_papply_dedup<V, LPR, K, 512, true><<<(int)wd.P, 512, sh, s>>>(wd, pa);
      else k_papply_dedup<V, LPR, K, 256, true><<<(int)wd.P, 256, sh, s>>>(wd, pa);
    }
    else if (wd.P <= 512u && !pa.det) k_papply_dedup<V, LPR, K, 512><<<(int)wd.P, 512, sh, s>>>(wd, pa);
    else k_papply_dedup<V, LPR, K, 256><<<(int)wd.P, 256, sh, s>>>(wd, pa);
    return KV_OK;
  });
}

int launch_dedup_fold(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab, unsigned nchunks,
                      int span) {
  return launch_apply_t<MODE_DEDUP, OPT_ADAGRAD>(wd, pa, s, md, ntab, nchunks, span);
}

}  // namespace kvhip_internal
