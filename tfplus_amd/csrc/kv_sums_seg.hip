// kv_sums_seg.hip — the gradient pre-sum of the sharded SPARSE apply (kv_shard_apply_route_sparse): kv_sums.hip's two launches
// — the tile sums, then the per-id sums over the route's entries — in the forms whose source row of a position comes from the
// segments' gradients (kv_types.h SegSrc: pscale[p] * seg_grad[pseg[p], :]) instead of a [n, dim] values buffer.  k_tsum_seg
// and k_papply_dedup_seg are tsum_body and papply_body with the row fetch replaced (their SEG template argument) and nothing
// else: the same mrow lists, entries, partitions and source lists drive the same additions in the same order.  A unit of its
// own, with kernels of their own names, so that nothing the training step runs is rebuilt.  Row geometry: kv_row_geom.h.
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

// k_tsum_seg: grid = ntiles blocks of TBC threads, the tile's mrow image in LDS.  md / sd: wd = the largest ntiles.
int launch_tsum_seg(const TableDev& td, const WsDev& wd, const SegSrc& sg, hipStream_t s, const MultiDesc* md, const SegDesc* sd,
                    int ntab) {
  return with_row_geom<ENTRY_MAX_Q>(td.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    if (md) k_tsum_seg_multi<V, LPR, K><<<dim3(wd.ntiles, (unsigned)ntab), TBC, (size_t)TILE * 4, s>>>(md, sd);
    else k_tsum_seg<V, LPR, K><<<wd.ntiles, TBC, (size_t)TILE * 4, s>>>(td, wd, sg);
    return KV_OK;
  });
}

// k_papply_dedup_seg: the block shapes of k_papply_dedup (launch_papply_ud)
int launch_papply_dedup_seg(const WsDev& wd, const PartArgs& pa, const SegSrc& sg, hipStream_t s, const MultiDesc* md,
                            const SegDesc* sd, int ntab) {
  const size_t sh = (size_t)wd.ntiles * 4 + 32;
  return with_row_geom<ENTRY_MAX_Q>(pa.tv.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    if (md) k_papply_dedup_seg_multi<V, LPR, K><<<dim3(wd.P, (unsigned)ntab), 256, sh, s>>>(md, sd);
    else if (wd.P <= 512u && !pa.det) k_papply_dedup_seg<V, LPR, K, 512><<<(int)wd.P, 512, sh, s>>>(wd, pa, sg);
    else k_papply_dedup_seg<V, LPR, K, 256><<<(int)wd.P, 256, sh, s>>>(wd, pa, sg);
    return KV_OK;
  });
}

}  // namespace kvhip_internal
