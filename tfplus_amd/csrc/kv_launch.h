// kv_launch.h — the launchers kvhip.hip, kv_ops.hip and kv_apply.hip call and the translation unit that defines each.  The optimizer apply kernels are
// instantiated once per OPT_*, in kv_opt_<name>.hip (kv_opt_unit.h); the optimizer-free sums in kv_sums.hip and, where the
// gradient arrives per segment, kv_sums_seg.hip.  A launcher
// dispatches on the row geometry — the one table of kv_row_geom.h, through with_row_geom — and returns KV_OK, or
// KV_UNIMPLEMENTED for a dim its kernels do not serve.
// md != nullptr: `ntab` tables in one launch (wd / n: the largest table's; pa: the first table's, only its dim is read).
#pragma once

#include "kv_types.h"
#include "kv_row_geom.h"

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// ---- per optimizer -----------------------------------------------------------------------------------------------------
// k_apply / k_apply_fin (kv_kernels.h, sorted positions): span 0 = k_apply over at most `nchunks` blocks, 1 = k_apply_fin;
// md: float4 rows only
template <int OPT>
int launch_sorted_apply(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab, unsigned nchunks,
                        int span);
// k_papply (kv_papply.h): partition pass + update in one launch; mode = PA_LOOKUP / PA_APPLYIDX / PA_NONE
template <int OPT>
int launch_papply(const WsDev& wd, const PartArgs& pa, int mode, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0);
// k_uapply (kv_uapply.h): the apply on unique ids and pre-summed rows, one launch.  n_dev != nullptr (one table): n bounds
// the batch and the kernel reads the id count from the device word (k_uapply_counted)
template <int OPT>
int launch_uapply(const PartArgs& pa, const void* ids, int ids32, long long n, hipStream_t s, const MultiDesc* md = nullptr,
                  int ntab = 0, const long long* n_dev = nullptr);

#define KV_OPT_LAUNCHERS(OPT)                                                                                                \
  template <> int launch_sorted_apply<OPT>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int, unsigned, int); \
  template <> int launch_papply<OPT>(const WsDev&, const PartArgs&, int, hipStream_t, const MultiDesc*, int);                 \
  template <> int launch_uapply<OPT>(const PartArgs&, const void*, int, long long, hipStream_t, const MultiDesc*, int, \
                                     const long long*)
KV_OPT_LAUNCHERS(OPT_ADAM_V4);         // kv_opt_adam_v4.hip
KV_OPT_LAUNCHERS(OPT_ADAM_V3);         // kv_opt_adam_v3.hip
KV_OPT_LAUNCHERS(OPT_ADAGRAD);         // kv_opt_adagrad.hip
KV_OPT_LAUNCHERS(OPT_FTRL);            // kv_opt_ftrl.hip
KV_OPT_LAUNCHERS(OPT_FTRL_V2);         // kv_opt_ftrl_v2.hip
KV_OPT_LAUNCHERS(OPT_GROUP_FTRL_V2);   // kv_opt_group_ftrl_v2.hip
KV_OPT_LAUNCHERS(OPT_GROUP_RADAM);     // kv_opt_group_radam.hip
KV_OPT_LAUNCHERS(OPT_ADAM);            // kv_opt_adam.hip

// ---- optimizer-free (kv_sums.hip) --------------------------------------------------------------------------------------
// k_tsum (kv_fused.h): the tile sums in front of k_papply
int launch_tsum(const TableDev& td, const WsDev& wd, const float* grad, hipStream_t s, const MultiDesc* md = nullptr,
                int ntab = 0);
// k_ltsum (kv_fused.h): the tile pass of a batch and its tile sums in one launch; ids_kind 0 int64, 1 int32
int launch_ltsum(const TableDev& td, const WsDev& wd, const void* ids, int ids_kind, long long n, int det, const float* grad,
                 hipStream_t s);
// k_papply_uniq (PA_UNIQUE: the distinct ids of a batch numbered) and k_papply_dedup (PA_DEDUP: the gradient rows summed per
// distinct id), kv_papply.h
int launch_papply_ud(const WsDev& wd, const PartArgs& pa, int mode, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0);
// k_apply / k_apply_fin in MODE_DEDUP: the plain segment fold (sorted positions), as launch_sorted_apply; no md form
int launch_dedup_fold(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab, unsigned nchunks,
                      int span);

// ---- optimizer-free, the gradient per segment (kv_sums_seg.hip; kv_types.h SegSrc) ---------------------------------------
// k_tsum_seg / k_papply_dedup_seg: launch_tsum and launch_papply_ud's PA_DEDUP where the row of a position is
// sg.pscale[p] * sg.seg_grad[sg.pseg[p], :].  md != nullptr: sd is the tables' SegDesc array next to it (sg is not read)
int launch_tsum_seg(const TableDev& td, const WsDev& wd, const SegSrc& sg, hipStream_t s, const MultiDesc* md = nullptr,
                    const SegDesc* sd = nullptr, int ntab = 0);
int launch_papply_dedup_seg(const WsDev& wd, const PartArgs& pa, const SegSrc& sg, hipStream_t s, const MultiDesc* md = nullptr,
                            const SegDesc* sd = nullptr, int ntab = 0);

}  // namespace kvhip_internal
