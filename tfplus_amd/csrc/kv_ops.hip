// kv_ops.hip — the table ops of the C ABI on the table core (kv_host.h): the training and inference lookups,
// kv_lookup_sparse with its backward and their batched forms, unique / dedup / segment sums, point queries, delete, export / import / delta, scatter.  Its own kernels
// are kv_op_kernels.h's; the pipelines' kernels are reached through the core's launchers.
//
// An entry point reads as its checks — in the reference's order, which differs per op: where n == 0 returns and where
// require_initialized stands is each op's own — then TableOp (device, lock, stream), how it enters the table, and what it
// launches.  The bodies two ops share are in the unnamed namespace: tile_pass_notable and segment_sums (the distinct-id
// ops), export_pass (the four export calls), read_figure (size / sum_freq / map size), scatter_like, delete_locked.
#include <hip/hip_runtime.h>

#include <iterator>

#include "kv_host.h"

using namespace kvhip_internal;

namespace {

#include "kv_device.h"
#include "kv_op_kernels.h"

// keys recorded by Delete while the table tracks deltas (kv_variable.h:747,772): no row carries them
static int record_deleted(kv_table* t, const void* ids, int64_t n, bool int32_ids, hipStream_t s) {
  if (!t->track_delta || n <= 0) return KV_OK;
  const size_t base = t->del_train.size();
  t->del_train.resize(base + (size_t)n);
  if (int32_ids) {
    std::vector<int> tmp((size_t)n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), ids, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t i = 0; i < n; ++i) t->del_train[base + (size_t)i] = tmp[(size_t)i];
  } else {
    HIP_TRY(hipMemcpyAsync(t->del_train.data() + base, ids, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return KV_OK;
}

// one recorded list: sorted, unique; keys that have a row again hand their membership to that row
static int delta_resolve(kv_table* t, std::vector<long long>* list, int which, hipStream_t s) {
  std::sort(list->begin(), list->end());
  list->erase(std::unique(list->begin(), list->end()), list->end());
  const size_t n = list->size();
  if (n == 0) return KV_OK;
  long long* dk = nullptr;
  unsigned char* dp = nullptr;
  HIP_TRY(hipMalloc(&dk, n * sizeof(long long)));
  if (hipMalloc(&dp, n) != hipSuccess) { hipFree(dk); return fail(KV_RESOURCE_EXHAUSTED, "delta export scratch"); }
  std::vector<unsigned char> present(n);
  hipError_t e = hipMemcpyAsync(dk, list->data(), n * sizeof(long long), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    k_delta_resolve<<<nblocks((long long)n, TB, 4096), TB, 0, s>>>(dev_view(t), dk, (long long)n, which, dp);
    e = hipMemcpyAsync(present.data(), dp, n, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(dk); hipFree(dp);
  if (e != hipSuccess) return fail(KV_INTERNAL, "delta export: %s", hipGetErrorString(e));
  size_t o = 0;
  for (size_t i = 0; i < n; ++i)
    if (!present[i]) (*list)[o++] = (*list)[i];
  list->resize(o);
  return KV_OK;
}

// all_delta minus the keys that have rows (dynamic_save.hpp:213-228): the recorded deletions still absent
static int delta_prepare(kv_table* t, int first_n, hipStream_t s, std::vector<long long>* absent) {
  int rc;
  if ((rc = delta_resolve(t, &t->del_train, 0, s))) return rc;
  *absent = t->del_train;
  if (first_n <= 3) {
    if ((rc = delta_resolve(t, &t->del_pred, 1, s))) return rc;
    std::vector<long long> u;
    std::set_union(t->del_train.begin(), t->del_train.end(), t->del_pred.begin(), t->del_pred.end(), std::back_inserter(u));
    absent->swap(u);
  }
  return KV_OK;
}

static int delta_after_export(kv_table* t, int first_n, unsigned nrows, hipStream_t s) {
  if (!t->track_delta && !t->track_pred && t->del_train.empty() && t->del_pred.empty()) return KV_OK;
  const int mode = first_n <= 3 ? 1 : 0;
  k_delta_clear<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, mode, t->track_pred ? 1 : 0);
  HIP_TRY(hipGetLastError());
  if (mode == 1) {
    t->del_pred.clear();
  } else {
    if (t->track_pred) t->del_pred.insert(t->del_pred.end(), t->del_train.begin(), t->del_train.end());
    t->del_train.clear();
  }
  return KV_OK;
}

// tf.unique_with_counts on the entry-list kernels (any dim: no row is touched): a table-less tile pass (entries, every
// position's entry) and k_papply PA_UNIQUE with dense numbers — uniq / uniq_counts written, every entry learns its id's
// number, the count in wd.ctr[0].  The table's mutex is held by the caller.
// the table-less tile pass of the distinct-id ops: entries and, file_pos, every position's entry number (pos_ent)
static int tile_pass_notable(kv_table* t, WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                             bool int32_ids, bool file_pos, hipStream_t s) {
  int rc;
  if (file_pos) {
    if ((rc = ensure_pos_ent(t, n, s))) return rc;
    wd.pos_ent = t->ws.pos_ent;
  }
  choose_partitions(t, wd, n);
  launch_ltile_notable(t, pa.tv, wd, ids, n, s, counts, int32_ids);
  return KV_OK;
}
static int fused_unique_pass(kv_table* t, WsDev& wd, PartArgs& pa, const void* ids, const int* counts, long long n, hipStream_t s) {
  int rc;
  if ((rc = tile_pass_notable(t, wd, pa, ids, counts, n, t->key_dtype == KV_DT_INT32, true, s))) return rc;
  // (k_papply_uniq: numbering only, nothing of the row geometry is touched — one kernel whatever the table's dim)
  if ((rc = launch_papply_ud(wd, pa, PA_UNIQUE, s))) return fail(rc, "unique: no kernel");
  return KV_OK;
}

// the count a synchronous op returns: device word -> pinned host word -> the caller (a copy into pageable memory goes through
// the runtime's staging path: measured against this in bench.py's unchanged_graph record)
static int read_count(kv_table* t, const unsigned* dev, hipStream_t s, unsigned* out) {
  if (!t->cnt_host) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->cnt_host), 64, hipHostMallocDefault));
  HIP_TRY(hipMemcpyAsync(t->cnt_host, dev, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out = *reinterpret_cast<volatile unsigned*>(t->cnt_host);
  return KV_OK;
}

// The rows pa.grad of one id folded (pa.fold_op) into one output row, on the batch pipeline; the table's mutex is held by the
// caller, which set the outputs in pa: out_keys + out_sum with dd_number (kv_dedup_segment_sum: the distinct ids numbered,
// summed[number]) or out_sum with direct_rows (kv_unsorted_segment_sum: an id IS its output row).  Sums on a table of the
// entry-list kernels' dims take those (sums_on_entries): the table-less tile pass — file_pos: with every
// position's entry, for an inverse — the tile sums of the ids repeated inside their tile (k_tsum), then ONE partition pass
// (k_papply PA_DEDUP: the per-id sums over the tiles' entries; dd_number, which launch_papply_ud alone reads: it numbers
// the ids it sums).  Everything else: the sorted positions (index_pass) and the segmented fold over them.
static bool sums_on_entries(const kv_table* t, int fold_op) { return fold_op == KV_SCATTER_ADD && fused_tab(t); }
static int segment_sums(kv_table* t, WsDev& wd, PartArgs& pa, const void* ids, long long n, bool int32_ids, bool file_pos,
                        const char* what, hipStream_t s) {
  int rc;
  if (!sums_on_entries(t, pa.fold_op)) {
    index_pass<MODE_UNIQUE>(t, wd, pa, ids, nullptr, n, int32_ids ? 1 : 0, nullptr, s);
    return launch_apply<MODE_DEDUP, OPT_ADAGRAD>(t, wd, pa, n, s);
  }
  if ((rc = tile_pass_notable(t, wd, pa, ids, nullptr, n, int32_ids, file_pos, s))) return rc;
  pa.epart = wd.epart;
  pa.day_lk = pa.day;
  if ((rc = launch_tsum(pa.tv, wd, pa.grad, s))) return fail(rc, "tile sums: no kernel for dim %d", t->dim);
  if ((rc = launch_papply_ud(wd, pa, PA_DEDUP, s))) return fail(rc, "%s: no kernel for dim %d", what, t->dim);
  return KV_OK;
}

// tf.unique + unsorted_segment_sum; the table's mutex is held by the caller.
// fold_op: how the rows of one id combine (KV_SCATTER_ADD = sum, MUL = product, MIN, MAX)
// The count goes to num_unique (host: the call synchronises, read_count) and / or to num_unique_dev (a device word, written
// by k_store_count behind the sums: nothing is synchronised), as kv_unique's.
static int dedup_locked(kv_table* t, const void* ids, const float* grad, int64_t n, int64_t* uniq,
                        float* summed, int32_t* inverse, int64_t* num_unique, int64_t* num_unique_dev, int fold_op,
                        hipStream_t s) {
  int rc;
  if ((rc = ensure_workspace(t, n, true, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch.drop();
  PartArgs pa = self_part_args(t, n);
  pa.grad = grad;
  pa.out_keys = (long long*)uniq;
  pa.out_sum = summed;
  pa.fold_op = fold_op;
  pa.dd_number = 1;
  if ((rc = segment_sums(t, wd, pa, ids, n, t->key_dtype == KV_DT_INT32, true, "per-id sums", s))) return rc;
  if (inverse && sums_on_entries(t, fold_op)) k_inverse_e<<<nblocks(n, TB, 2048), TB, 0, s>>>(t->ws.pos_ent, wd.ent_b, n, inverse);
  else if (inverse) k_dedup_inverse<<<nblocks(n, TB, 2048), TB, 0, s>>>(wd, n, inverse);
  if (num_unique_dev) {
    k_store_count<<<1, 1, 0, s>>>(wd.ctr, (long long*)num_unique_dev);
    HIP_TRY(hipGetLastError());
  }
  if (num_unique) {   // synchronous form
    unsigned U = 0;
    if ((rc = read_count(t, wd.ctr, s, &U))) return rc;
    *num_unique = U;
  }
  return KV_OK;
}

// after a kernel that pushed rows: read the counters, account the pushes (synchronous)
static int after_release(kv_table* t, hipStream_t s, unsigned long long* released) {
  unsigned c[3];
  unsigned long long n = 0;
  HIP_TRY(hipMemcpyAsync(&n, t->d_stat, sizeof n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(c, t->d_counters, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t->pushes_since += n;
  t->free_known = std::max(0, (int)c[2]);
  t->rows_ub = c[0];
  *released = n;
  return KV_OK;
}

static int delete_locked(kv_table* t, const void* ids, int64_t n, int64_t* num_deleted, hipStream_t s) {
  int rc;
  if ((rc = enter_op(t, s))) return rc;
  t->batch.drop();   // rows are released: an index of a batch that held them is void (its token goes stale)
  if ((rc = ensure_free_list(t, s))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  with_id_type(t->key_dtype == KV_DT_INT32, [&](auto id) {
    using IDT = decltype(id);
    k_delete<IDT><<<nblocks(n, TB, 4096), TB, 0, s>>>(dev_view(t), (const IDT*)ids, n, t->free_rows, t->d_stat);
  });
  HIP_TRY(hipGetLastError());
  unsigned long long rel = 0;
  if ((rc = after_release(t, s, &rel))) return rc;
  if (num_deleted) *num_deleted = (int64_t)rel;
  return KV_OK;
}

static int count_or_ts(kv_handle_t t, const void* ids, int64_t n, int what, uint32_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n < 0 || (n > 0 && (!ids || !out))) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  if ((rc = require_initialized(t))) return rc;
  if (n == 0) return KV_OK;
  TableOp op(t, stream);
  if ((rc = join_side(t, op.s))) return rc;
  with_id_type(t->key_dtype == KV_DT_INT32, [&](auto id) {
    using IDT = decltype(id);
    k_get_count_ts<IDT><<<nblocks(n, TB, 4096), TB, 0, op.s>>>(dev_view(t), (const IDT*)ids, n, what, today(t), out);
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// insert / scatter / import marks: tile pass (dedup) -> partition pass on the unique keys
static int scatter_like(kv_handle_t t, const void* ids, const float* vals, int64_t n, int op,
                        int is_insert, int mark, const unsigned* fvals, hipStream_t s) {
  int rc;
  if (n == 0) return KV_OK;
  if (n < 0 || !ids || (!vals && mark < 0)) return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (!is_insert && mark < 0 && (rc = require_initialized(t))) return rc;
  const long long CH = 1ll << 21;
  const size_t idsz = t->key_dtype == KV_DT_INT32 ? 4 : 8;
  for (long long off = 0; off < n; off += CH) {
    const long long m = std::min(CH, (long long)n - off);
    if ((rc = ensure_capacity(t, m, s))) return rc;
    if ((rc = ensure_workspace(t, m, false, s))) return rc;
    const WsDev wd = ws_view(t, m);
    PartArgs pa = self_part_args(t, m);   // (neither k_part_keys<MODE_SCATTER> nor <MODE_MARK> reads det or n)
    if (!t->initialized) {
      // InsertOrUpdate / import never consult the init table; new rows start from the zero row
      pa.tv.init_table = t->chunks[0].rows;
      pa.tv.init_rows = 1;
      pa.ts0 = pa.tv; pa.ts1 = pa.tv;
    }
    pa.grad = vals ? vals + (size_t)off * t->dim : nullptr;
    pa.scatter_op = op; pa.is_insert = is_insert;
    pa.mark_what = mark; pa.fvals = fvals ? fvals + off : nullptr;
    t->batch.drop();
    launch_tile<true>(t, wd, (const char*)ids + (size_t)off * idsz, nullptr, m, s);
    if (mark >= 0) launch_part_keys<MODE_MARK>(wd, pa, s);
    else launch_part_keys<MODE_SCATTER>(wd, pa, s);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// a figure of the table (kv_variable.h:139-175), which: 0 size(), 1 sum_freq(), 2 the map's rows (live keys, whatever
// their frequency)
static int read_figure(kv_handle_t t, int which, int64_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  unsigned long long o[2];
  unsigned nrows = 1;
  if ((rc = stats(t, op.s, which < 2 ? o : nullptr, which < 2 ? nullptr : &nrows))) return rc;
  *out = which < 2 ? (int64_t)o[which] : (int64_t)nrows - 1 - t->free_known;
  return KV_OK;
}

// One export kernel (k_export, k_export_delta) over the table's rows: d_stat cleared, the launch — a fill with the buffers
// it writes — and, c != nullptr, its three counters read back (synchronous).
template <class Kernel>
static int export_pass(kv_table* t, Kernel kernel, unsigned nrows, int first_n, unsigned long long* c, hipStream_t s,
                       bool fill = false, int64_t* keys = nullptr, float* values = nullptr, int64_t* blacklist = nullptr,
                       int64_t* fkeys = nullptr, uint32_t* fvals = nullptr) {
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  kernel<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, first_n, fill ? 1 : 0, t->d_stat, (long long*)keys, values,
                                                 (long long*)blacklist, (long long*)fkeys, fvals);
  if (fill) HIP_TRY(hipGetLastError());
  if (!c) return KV_OK;
  HIP_TRY(hipMemcpyAsync(c, t->d_stat, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return KV_OK;
}

// placeholder init table for tables that are marked initialised by an import
static int ensure_init_placeholder(kv_table* t, hipStream_t s) {
  if (!t->init_table) {
    // the import marks the variable initialised (dynamic_restore.hpp:249-255).  The checkpoint's
    // init table is the caller's to pass through kv_init_table; without one, keys inserted later
    // start from a one-row zero table instead of dereferencing nothing.
    HIP_TRY(hipMalloc(&t->init_table, (size_t)t->dim * sizeof(float)));
    HIP_TRY(hipMemsetAsync(t->init_table, 0, (size_t)t->dim * sizeof(float), s));
    t->init_rows = 1;
    t->init_placeholder = true;
  }
  return KV_OK;
}


// the argument checks kv_lookup_sparse, its backward and their batched forms share
static int sparse_call_checks(int combiner, int segment_dtype) {
  if (combiner < KV_COMBINER_SUM || combiner > KV_COMBINER_SQRTN)
    return fail(KV_INVALID_ARGUMENT, "combiner must be one of 'mean', 'sqrtn' or 'sum'");  // embedding_ops.py:345
  if (segment_dtype != KV_DT_INT32 && segment_dtype != KV_DT_INT64)
    return fail(KV_INVALID_ARGUMENT, "segment ids must be int32 or int64");
  return KV_OK;
}
static int sparse_size_checks(const kv_table* t, int64_t n, int64_t num_segments) {
  const bool fused = fused_tab(t);   // (dim is fixed at creation: readable without the lock)
  if (n < 0 || n > (fused ? FUSED_MAX_N : (1ll << 21)))
    return fail(KV_INVALID_ARGUMENT, "sp_ids: %lld values (at most 2^%d per call)", (long long)n, fused ? 23 : 21);
  if (num_segments < 0 || num_segments > (1ll << 31) - 2) return fail(KV_INVALID_ARGUMENT, "bad num_segments");
  return KV_OK;
}

// kv_lookup_sparse behind its checks; the table's mutex is held by the caller, its device is current
static int lookup_sparse_locked(kv_table* t, const void* ids, const void* segment_ids, int segment_dtype, const float* weights,
                                int64_t n, int64_t num_segments, int combiner, int count_occurrences, float* out, hipStream_t s) {
  int rc;
  const bool fused = fused_tab(t);
  if ((rc = enter_op(t, s, KEEP_VAR))) return rc;   // the table's own rows and records only
  const int D = t->dim;
  if (n == 0) {  // every segment is empty
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_segments * D * sizeof(float), s));
    return KV_OK;
  }
  if ((rc = ensure_capacity(t, n, s))) return rc;
  if ((rc = ensure_workspace(t, n, false, s))) return rc;
  if ((rc = ensure_seg(t, num_segments, false, s))) return rc;
  Workspace& ws = t->ws;
  // every position's entry in its tile (k_ltile files it for the combiner)
  if (fused && (rc = ensure_pos_ent(t, n, s))) return rc;
  WsDev wd = ws_view(t, n);
  PartArgs pa = self_part_args(t, n);
  const TableDev& td = pa.tv;
  pa.day = today(t);
  pa.count_once = count_occurrences ? 0 : 1;
  t->batch.drop();
  if (fused) {
    // the entry-list kernels: tile pass without rows (entries, every position's entry), the lookup's bookkeeping (which
    // also publishes the rows of new keys), then the combiner reads position -> entry -> row
    wd.pos_ent = ws.pos_ent;
    if ((rc = fused_lookup_pass(t, wd, pa, ids, nullptr, n, -1, nullptr, s, false))) return rc;
  } else {
    {
      ProfScope ps(t, KV_PROF_LOOKUP_TILE, s);
      launch_tile<false>(t, wd, ids, nullptr, n, s);
    }
    ProfScope ps(t, KV_PROF_LOOKUP_PART, s);
    launch_part_keys<MODE_LOOKUP>(wd, pa, s);
  }
  ProfScope ps_gather(t, KV_PROF_LOOKUP_ORDER, s);
  with_id_type(segment_dtype == KV_DT_INT32, [&](auto id) {
    using IDT = decltype(id);
    k_seg_offsets<IDT><<<nblocks(n + 1, TB, 2048), TB, 0, s>>>((const IDT*)segment_ids, n, num_segments, ws.seg_off);
  });
  const int q = pow2_vectors(D, 64);   // the sorted-position combiner's rows: a power of two of float4, or <0>
  const int grid = nblocks(num_segments * (fused ? row_lanes(D) : q ? q : 1), TB, 8192);
  if (fused)
    with_lanes(row_lanes(D), [&](auto vq) {
      k_seg_combine_e<decltype(vq)::value><<<grid, TB, 0, s>>>(td, ws.pos_ent, wd.ent_b, wd.ent_key, ws.seg_off, weights, num_segments, combiner, out);
    });
  else if (q)
    with_lanes(q, [&](auto vq) {
      k_seg_combine<decltype(vq)::value><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out);
    });
  else
    k_seg_combine<0><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// the expand kernels' lane group: float4 lanes for dims that are a multiple of 4 (64 at the most: wider rows take more
// than one round), 0 = one thread per element
static int expand_lanes(int D) { return D % 4 == 0 ? std::min(64, row_lanes(D)) : 0; }
// f(SegT{}, integral_constant<VQ>) for the expand kernels' template arguments
template <class F>
static void with_expand_types(bool int32_seg, int lanes, F&& f) {
  with_id_type(int32_seg, [&](auto id) {
    if (lanes == 0) f(id, std::integral_constant<int, 0>{});
    else with_lanes(lanes, [&](auto vq) { f(id, vq); });
  });
}

// kv_lookup_sparse_grad behind its checks (n > 0, num_segments > 0); the table's mutex is held by the caller
static int lookup_sparse_grad_locked(kv_table* t, const float* seg_grad, const void* segment_ids, int segment_dtype,
                                     const float* weights, int64_t n, int64_t num_segments, int combiner, float* values,
                                     hipStream_t s) {
  int rc;
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, s, KEEP_VAR | KEEP_SLOT))) return rc;
  const bool need_den = weights != nullptr && combiner != KV_COMBINER_SUM;
  if ((rc = ensure_seg(t, num_segments, need_den, s))) return rc;
  Workspace& ws = t->ws;
  const int D = t->dim;
  const bool seg32 = segment_dtype == KV_DT_INT32;
  with_id_type(seg32, [&](auto id) {
    using IDT = decltype(id);
    k_seg_offsets<IDT><<<nblocks(n + 1, TB, 2048), TB, 0, s>>>((const IDT*)segment_ids, n, num_segments, ws.seg_off);
  });
  if (need_den) k_seg_den<<<nblocks(num_segments, TB, 4096), TB, 0, s>>>(ws.seg_off, weights, num_segments, combiner, ws.seg_den);
  const int lanes = expand_lanes(D);
  const int grid = nblocks(n * (lanes ? lanes : D), TB, 16384);
  with_expand_types(seg32, lanes, [&](auto id, auto vq) {
    using IDT = decltype(id);
    k_seg_expand<IDT, decltype(vq)::value><<<grid, TB, 0, s>>>(seg_grad, (const IDT*)segment_ids, ws.seg_off, ws.seg_den, weights, n,
                                                               num_segments, D, combiner, values);
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// what the batched sparse ops check of every table's sizes and pointers beyond multi_common (whose id lists are the ids —
// forward — or the segment ids — backward).  rows: outs (forward: written whenever the table has segments) or values
// (backward: written where it has positions too); src: the segment ids (forward) or the segments' gradients (backward).
// en: the ids per table that take part — none for a table without segments, a no-op as in the single-table ops
static int multi_sparse_checks(int num_tables, const kv_handle_t* tables, const int64_t* ns, const int64_t* num_segments,
                               const void* const* rows, bool rows_without_ids, const void* const* src, std::vector<int64_t>* en) {
  int rc;
  if (num_tables < 1) return fail(KV_INVALID_ARGUMENT, "N must be >= 1");
  if (!tables || !ns || !num_segments || !rows || !src) return fail(KV_INVALID_ARGUMENT, "null argument array");
  en->resize((size_t)num_tables);
  for (int i = 0; i < num_tables; ++i) {
    if ((rc = check_table(tables[i]))) return rc;
    if ((rc = sparse_size_checks(tables[i], ns[i], num_segments[i]))) return rc;
    const int64_t m = num_segments[i] == 0 ? 0 : ns[i];
    (*en)[(size_t)i] = m;
    if ((m > 0 && (!src[i] || !rows[i])) || (rows_without_ids && num_segments[i] > 0 && !rows[i]))
      return fail(KV_INVALID_ARGUMENT, "segment ids / gradient / output pointer is null");
  }
  return KV_OK;
}

// kv_lookup_sparse_zeros / kv_batch_lookup_sparse_zeros: the checks of one table's arguments, in the order of the header
static int sparse_zeros_checks(const kv_table* t, const void* ids, const void* segment_ids, int segment_dtype, int64_t n,
                               int64_t num_segments, int combiner, const float* out) {
  int rc;
  if ((rc = require_initialized(t))) return rc;   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
  if (num_segments > 0 && (!out || (n > 0 && (!ids || !segment_ids))))
    return fail(KV_INVALID_ARGUMENT, "ids / segment ids / output pointer is null");
  if (n < 0 || n >= (1ll << 31)) return fail(KV_INVALID_ARGUMENT, "sp_ids: %lld values (fewer than 2^31 per call)", (long long)n);
  if (num_segments < 0 || num_segments > (1ll << 31) - 2) return fail(KV_INVALID_ARGUMENT, "bad num_segments");
  if (segment_dtype != KV_DT_INT32 && segment_dtype != KV_DT_INT64)
    return fail(KV_INVALID_ARGUMENT, "segment ids must be int32 or int64");
  if (combiner < KV_COMBINER_SUM || combiner > KV_COMBINER_SQRTN)
    return fail(KV_INVALID_ARGUMENT, "combiner must be one of 'mean', 'sqrtn' or 'sum'");  // embedding_ops.py:345
  if (!dim_supported(t->dim)) return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported", t->dim);
  return KV_OK;
}
// lanes of a segment's group in lsz_body: dim / 4 for the dims 4, 8, ..., 256, else (0) the whole wave
static int sparse_zeros_lanes(int D) { return pow2_vectors(D, 64); }
}  // namespace

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// the sparse lookups' segment buffers: Workspace::seg_off holds num_segments + 1 offsets and, need_den, Workspace::seg_den
// num_segments denominators (grown behind ws_sync like the rest of the workspace)
int ensure_seg(kv_table* t, long long num_segments, bool need_den, hipStream_t s) {
  int rc;
  Workspace& ws = t->ws;
  if (ws.seg_cap < num_segments) {
    if ((rc = ws_sync(s))) return rc;
    const long long want = std::max<long long>(num_segments, ws.seg_cap * 2);
    ws.seg_cap = 0;
    if ((rc = regrow(&ws.seg_off, (size_t)(want + 1)))) return rc;
    ws.seg_cap = want;
  }
  if (need_den && ws.den_cap < num_segments) {
    if ((rc = ws_sync(s))) return rc;
    const long long want = std::max<long long>(num_segments, ws.den_cap * 2);
    ws.den_cap = 0;
    if ((rc = regrow(&ws.seg_den, (size_t)want))) return rc;
    ws.den_cap = want;
  }
  return KV_OK;
}

// the position records of the sharded sparse apply (kv_host.h; the kernels: kv_op_kernels.h).  The tables' buffers are
// sized by the caller (ensure_seg, ensure_pos_records); a descriptor with n == 0 takes no part.
int launch_pos_records(int m, const SegDesc* host, const SegDesc* dev, int seg32, int combiner, hipStream_t s) {
  long long nmax = 0, segmax = 0;
  bool any_den = false;
  for (int j = 0; j < m; ++j) {
    if (host[j].n == 0) continue;
    nmax = std::max(nmax, host[j].n);
    segmax = std::max(segmax, host[j].nseg);
    any_den |= host[j].den != nullptr;
  }
  if (nmax == 0) return KV_OK;
  const unsigned go = (unsigned)nblocks(nmax + 1, TB, 2048), gd = (unsigned)nblocks(segmax, TB, 4096), gr = (unsigned)nblocks(nmax, TB, 2048);
  with_id_type(seg32 != 0, [&](auto id) {
    using IDT = decltype(id);
    if (m == 1) {
      const SegDesc d = host[0];
      k_seg_offsets<IDT><<<go, TB, 0, s>>>((const IDT*)d.seg, d.n, d.nseg, d.off);
      if (any_den) k_seg_den<<<gd, TB, 0, s>>>(d.off, d.wts, d.nseg, combiner, d.den);
      k_pos_records<IDT><<<gr, TB, 0, s>>>(d, combiner);
    } else {
      k_pos_offsets_multi<IDT><<<dim3(go, (unsigned)m), TB, 0, s>>>(dev);
      if (any_den) k_pos_den_multi<<<dim3(gd, (unsigned)m), TB, 0, s>>>(dev, combiner);
      k_pos_records_multi<IDT><<<dim3(gr, (unsigned)m), TB, 0, s>>>(dev, combiner);
    }
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// ---- many tables, one launch per pipeline stage (26-feature CTR step: 5 launches, not 130) ------
// All tables: same device, same dim, same key dtype; each batch <= 2^21 ids.
int multi_common(int num_tables, const kv_handle_t* tables, const void* const* ids, const int64_t* ns) {
  int rc;
  if ((rc = check_same_shape(num_tables, tables, "tables"))) return rc;
  if (!ids || !ns) return fail(KV_INVALID_ARGUMENT, "null argument array");
  for (int i = 0; i < num_tables; ++i) {
    if (tables[i]->dim != tables[0]->dim || tables[i]->key_dtype != tables[0]->key_dtype)
      return fail(KV_INVALID_ARGUMENT, "batched op: tables must share dim and key dtype (group them by shape)");
    if (tables[i]->occurrence_order)
      return fail(KV_UNIMPLEMENTED, "batched op: a table in occurrence-order mode (kv_set_deterministic(h, 2)) takes the per-table ops");
    // (the entry-list kernels index up to FUSED_MAX_N ids per table and call, like the single-table ops; other dims 2^21)
    if (ns[i] < 0 || ns[i] > (fused_tab(tables[0]) ? FUSED_MAX_N : (1ll << 21)))
      return fail(KV_INVALID_ARGUMENT, "indices: bad length %lld", (long long)ns[i]);
    if (ns[i] > 0 && !ids[i]) return fail(KV_INVALID_ARGUMENT, "indices pointer is null");
    if ((rc = require_initialized(tables[i]))) return rc;
    for (int j = 0; j < i; ++j)
      if (tables[j] == tables[i]) return fail(KV_INVALID_ARGUMENT, "batched op: table listed twice");
  }
  return KV_OK;
}

// seg_cap + self: the (id, count) records of a sharded owner lookup, in fixed-capacity segments (kv_shard_lookup_serve)
int gather_or_insert_impl(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, float* out,
                          kv_stream_t stream, int pairs, kv_batch_token_t* token, unsigned seg_cap,
                          const SelfSegment* self) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n == 0) return KV_OK;  // kv_variable_ops.cc:530-532
  if (n < 0 || n > (1ll << 30)) return fail(KV_INVALID_ARGUMENT, "indices: bad length %lld", (long long)n);
  if (!ids || !out) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  if ((rc = require_initialized(t))) return rc;
  TableOp tab(t, stream);
  const hipStream_t s = tab.s;
  if ((rc = enter_op(t, s, KEEP_VAR))) return rc;   // a training lookup touches the var's rows and records, never a slot record or a mirror
  // any batch length: chunks of 2^21 ids are looked up one after another (same semantics as one
  // pass: the frequency adds saturate identically and rows are inserted by the first chunk)
  // the entry-list pipeline indexes a batch of up to FUSED_MAX_N ids in one pass; the sorted-position one 2^21
  const long long CHK = fused_tab(t) ? FUSED_MAX_N : (1ll << 21);
  const size_t idsz = pairs ? 16 : (t->key_dtype == KV_DT_INT32 ? 4 : 8);
  t->batch.drop();
  const bool tok = token != nullptr && n <= CHK;   // a token is asked for, one pass indexes the batch: an apply of it follows
  // ... and takes the lookup's partition pass with it — but not under a stream capture: a pass still pending when the capture
  // ends would be launched by the table's next op, outside the graph, and no replay would do the lookup's bookkeeping
  // (frequency words, the rows of new keys).  A captured lookup runs its pass itself; the apply takes the entries (TAKE_DONE).
  const bool defer = tok && !stream_is_capturing(s);
  unsigned P = 0;
  for (long long off = 0; off < n; off += CHK) {
    const long long m = std::min(CHK, (long long)n - off);
    const void* idp = (const char*)ids + (size_t)off * idsz;
    const int32_t* cp = counts ? counts + off : nullptr;
    float* op = out + (size_t)off * t->dim;
    if ((rc = ensure_capacity(t, m, s))) return rc;
    if ((rc = ensure_workspace(t, m, false, s))) return rc;
    WsDev wd = ws_view(t, m, self);
    wd.seg_cap = seg_cap;
    PartArgs pa = self_part_args(t, m);
    pa.day = today(t);
    if (fused_tab(t)) { if ((rc = fused_lookup_pass(t, wd, pa, idp, cp, m, pairs ? 2 : -1, op, s, defer))) return rc; }
    else index_pass<MODE_LOOKUP>(t, wd, pa, idp, cp, m, pairs ? 2 : -1, op, s, tok);
    P = wd.P;
  }
  HIP_TRY(hipGetLastError());
  // the workspace now holds the index of exactly this batch, positions filed
  if (tok) *token = t->batch.publish(++g_serial, n, fused_tab(t) ? BatchIndex::ENTRIES : BatchIndex::SORTED, P);
  return KV_OK;
}

// ids_kind 2 + seg_caps + selfs (one per table): the (id, count) records of the sharded owner lookups, in fixed-capacity
// segments (kv_multi_shard_lookup)
int multi_lookup_impl(int num_tables, const kv_handle_t* tables, const void* const* ids,
                      const int32_t* const* counts, const int64_t* ns, float* const* outs,
                      kv_batch_token_t* tokens, kv_stream_t stream, int ids_kind, const unsigned* seg_caps,
                      const SelfSegment* selfs) {
  int rc;
  if (tokens && num_tables > 0) std::memset(tokens, 0, (size_t)num_tables * sizeof(kv_batch_token_t));
  if ((rc = multi_common(num_tables, tables, ids, ns))) return rc;
  if (!outs) return fail(KV_INVALID_ARGUMENT, "null argument array");
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));
  if ((rc = lock.enter(s, [](const kv_table*) { return (unsigned)KEEP_VAR; }))) return rc;   // lookups: the tables' own rows and records only
  long long nmax = 0;
  for (int i = 0; i < num_tables; ++i) {
    tables[i]->batch.drop();
    if (ns[i] > 0 && !outs[i]) return fail(KV_INVALID_ARGUMENT, "output pointer is null");
    if ((rc = ensure_capacity(tables[i], ns[i], s))) return rc;
    if ((rc = ensure_workspace(tables[i], std::max<long long>(ns[i], 1), false, s))) return rc;
    nmax = std::max<long long>(nmax, ns[i]);
  }
  if (nmax == 0) return KV_OK;
  Staged<MultiDesc> hd(device, 1, num_tables);
  if (hd.rc) return hd.rc;
  WsDev wmax{};
  for (int i = 0; i < num_tables; ++i) {
    MultiDesc& d = hd[i];
    d.w = ws_view(tables[i], std::max<long long>(ns[i], 1), selfs ? &selfs[i] : nullptr);
    if (seg_caps) d.w.seg_cap = seg_caps[i];
    if (fused_tab(tables[i])) use_partitions(d.w, fused_default_P(std::max<long long>(ns[i], 1)));
    d.a = self_part_args(tables[i], ns[i]);   // (det: multi_common refuses occurrence-order tables)
    d.a.day = today(tables[i]);
    d.ids = ids[i];
    d.counts = counts ? counts[i] : nullptr;
    d.out = outs[i];
    d.n = ns[i];
    if (ns[i] == 0) d.w.ntiles = 0;
    widen(wmax, d.w);
  }
  const MultiDesc* md;
  if ((rc = hd.upload(s, &md))) return rc;
  kv_table* t0 = tables[0];
  if (fused_tab(t0)) {
    launch_ltile(t0, hd[0].a.tv, wmax, nullptr, nullptr, nmax, nullptr, s, ids_kind, md, num_tables, true);
    // tokens asked for: an optimizer apply of these batches follows — every table's partition pass stays pending
    // (kv_multi_apply_*_tok completes it inside k_papply_multi; any other op on a table settles that table first)
    // (not under a stream capture: gather_or_insert_impl)
    const bool defer = tokens != nullptr && !stream_is_capturing(s);
    if (!defer) launch_part2(wmax, hd[0].a, s, md, num_tables);
    if (tokens)   // every table's workspace now holds the index of exactly its batch (kv_multi_apply_*_tok takes it over)
      for (int i = 0; i < num_tables; ++i) {
        if (ns[i] <= 0) continue;
        tokens[i] = tables[i]->batch.publish(++g_serial, ns[i], BatchIndex::ENTRIES, hd[i].w.P);
        if (defer) set_pending_part(tables[i], hd[i].w, hd[i].a);
      }
  } else {
    launch_tile<false>(t0, wmax, nullptr, nullptr, nmax, s, -1, md, num_tables, wmax.ntiles);
    launch_part_keys<MODE_LOOKUP>(wmax, hd[0].a, s, md, num_tables);
    launch_gather(hd[0].a.tv, wmax, nullptr, nmax, s, md, num_tables);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}
}  // namespace kvhip_internal

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int kv_size(kv_handle_t t, int64_t* out, kv_stream_t stream) { return read_figure(t, 0, out, stream); }
int kv_sum_freq(kv_handle_t t, int64_t* out, kv_stream_t stream) { return read_figure(t, 1, out, stream); }
int kv_map_size(kv_handle_t t, int64_t* out, kv_stream_t stream) { return read_figure(t, 2, out, stream); }

int kv_get_meta(kv_handle_t t, const int64_t* ids, int64_t n, uint32_t* fw, uint8_t* fl, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n <= 0) return KV_OK;
  TableOp op(t, stream);
  if ((rc = join_side(t, op.s))) return rc;
  k_get_meta<long long><<<nblocks(n, TB), TB, 0, op.s>>>(dev_view(t), (const long long*)ids, n, fw, fl);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_gather_or_insert(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, float* out,
                        kv_stream_t stream) {
  return gather_or_insert_impl(t, ids, counts, n, out, stream, 0, nullptr);
}
int kv_gather_or_insert_tok(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, float* out,
                            kv_batch_token_t* token, kv_stream_t stream) {
  if (token) *token = 0;
  return gather_or_insert_impl(t, ids, counts, n, out, stream, 0, token);
}
int kv_gather_or_insert_pairs(kv_handle_t t, const int64_t* id_count_pairs, int64_t n, float* out,
                              kv_stream_t stream) {
  if (t && t->key_dtype == KV_DT_INT32) return fail(KV_INVALID_ARGUMENT, "id/count pairs carry int64 ids");
  return gather_or_insert_impl(t, id_count_pairs, nullptr, n, out, stream, 1, nullptr);
}

int kv_lookup_sparse(kv_handle_t t, const void* ids, const void* segment_ids, int segment_dtype,
                     const float* weights, int64_t n, int64_t num_segments, int combiner, int count_occurrences,
                     float* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if ((rc = sparse_call_checks(combiner, segment_dtype))) return rc;
  if ((rc = sparse_size_checks(t, n, num_segments))) return rc;
  if (num_segments == 0) return KV_OK;
  if (!out || (n > 0 && (!ids || !segment_ids))) return fail(KV_INVALID_ARGUMENT, "ids / segment ids / output pointer is null");
  if ((rc = require_initialized(t))) return rc;
  TableOp op(t, stream);
  return lookup_sparse_locked(t, ids, segment_ids, segment_dtype, weights, n, num_segments, combiner, count_occurrences, out, op.s);
}

int kv_lookup_sparse_grad(kv_handle_t t, const float* seg_grad, const void* segment_ids, int segment_dtype,
                          const float* weights, int64_t n, int64_t num_segments, int combiner, float* values,
                          kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if ((rc = sparse_call_checks(combiner, segment_dtype))) return rc;
  if ((rc = sparse_size_checks(t, n, num_segments))) return rc;
  if (num_segments == 0 || n == 0) return KV_OK;
  if (!seg_grad || !segment_ids || !values) return fail(KV_INVALID_ARGUMENT, "gradient / segment ids / output pointer is null");
  if ((rc = require_initialized(t))) return rc;
  TableOp op(t, stream);
  return lookup_sparse_grad_locked(t, seg_grad, segment_ids, segment_dtype, weights, n, num_segments, combiner, values, op.s);
}

int kv_multi_lookup_sparse(int num_tables, const kv_handle_t* tables, const void* const* ids,
                           const void* const* segment_ids, int segment_dtype, const float* const* weights,
                           const int64_t* ns, const int64_t* num_segments, int combiner,
                           const int* count_occurrences, float* const* outs, kv_stream_t stream) {
  int rc;
  if ((rc = sparse_call_checks(combiner, segment_dtype))) return rc;
  std::vector<int64_t> en;   // ids per table that take part (0 for a table without segments)
  if ((rc = multi_sparse_checks(num_tables, tables, ns, num_segments, (const void* const*)outs, true, segment_ids, &en))) return rc;
  if ((rc = multi_common(num_tables, tables, ids, en.data()))) return rc;
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));
  auto wts = [&](int i) { return weights ? weights[i] : nullptr; };
  auto occ = [&](int i) { return count_occurrences ? count_occurrences[i] : 0; };
  kv_table* t0 = tables[0];
  if (!fused_tab(t0)) {
    // a dim the entry-list kernels do not serve: the single-table path, table by table, under the same locks
    for (int i = 0; i < num_tables; ++i)
      if (num_segments[i] > 0 &&
          (rc = lookup_sparse_locked(tables[i], ids[i], segment_ids[i], segment_dtype, wts(i), ns[i], num_segments[i], combiner,
                                     occ(i), outs[i], s)))
        return rc;
    return KV_OK;
  }
  if ((rc = lock.enter(s, [](const kv_table*) { return (unsigned)KEEP_VAR; }))) return rc;   // the tables' own rows and records only
  // every buffer that may have to grow, before anything is queued
  long long nmax = 0, segmax = 0;
  for (int i = 0; i < num_tables; ++i) {
    kv_table* t = tables[i];
    t->batch.drop();
    if (num_segments[i] == 0) continue;
    if ((rc = ensure_capacity(t, en[i], s))) return rc;
    if ((rc = ensure_workspace(t, std::max<long long>(en[i], 1), false, s))) return rc;
    if ((rc = ensure_seg(t, num_segments[i], false, s))) return rc;
    if ((rc = ensure_pos_ent(t, std::max<long long>(en[i], 1), s))) return rc;
    nmax = std::max<long long>(nmax, en[i]);
    segmax = std::max<long long>(segmax, num_segments[i]);
  }
  if (segmax == 0) return KV_OK;
  Staged<MultiDesc> hd(device, 1, num_tables);
  if (hd.rc) return hd.rc;
  Staged<SparseDesc> sd(device, 2, num_tables);
  if (sd.rc) return sd.rc;
  WsDev wmax{};
  for (int i = 0; i < num_tables; ++i) {
    kv_table* t = tables[i];
    MultiDesc& d = hd[i];
    d.w = ws_view(t, std::max<long long>(en[i], 1));
    use_partitions(d.w, fused_default_P(std::max<long long>(en[i], 1)));
    d.w.pos_ent = t->ws.pos_ent;
    d.a = self_part_args(t, en[i]);   // (det: multi_common refuses occurrence-order tables)
    d.a.day = today(t);
    d.a.count_once = occ(i) ? 0 : 1;
    d.ids = ids[i];
    d.n = en[i];
    if (en[i] == 0) d.w.ntiles = 0;
    widen(wmax, d.w);
    SparseDesc& q = sd[i];
    q.seg = segment_ids[i];
    q.wts = en[i] > 0 ? wts(i) : nullptr;   // no ids: zero rows, whatever the weights would divide by
    q.off = t->ws.seg_off;
    q.out = outs[i];
    q.n = en[i];
    q.nseg = num_segments[i];
  }
  const MultiDesc* md;
  const SparseDesc* sp;
  if ((rc = hd.upload(s, &md))) return rc;
  if ((rc = sd.upload(s, &sp))) return rc;
  // four launches whatever num_tables is: the tile pass without rows (entries, every position's entry), the lookups'
  // bookkeeping (which publishes the rows of new keys), the offsets, the combiner
  if (nmax > 0) {
    launch_ltile(t0, hd[0].a.tv, wmax, nullptr, nullptr, nmax, nullptr, s, -1, md, num_tables, false);
    launch_part2(wmax, hd[0].a, s, md, num_tables);
  }
  with_id_type(segment_dtype == KV_DT_INT32, [&](auto id) {
    using IDT = decltype(id);
    k_seg_offsets_multi<IDT><<<dim3((unsigned)nblocks(nmax + 1, TB, 2048), (unsigned)num_tables), TB, 0, s>>>(sp);
  });
  const int lanes = row_lanes(t0->dim);
  with_lanes(lanes, [&](auto vq) {
    k_seg_combine_e_multi<decltype(vq)::value><<<dim3((unsigned)nblocks(segmax * lanes, TB, 8192), (unsigned)num_tables), TB, 0, s>>>(
        md, sp, combiner);
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_multi_lookup_sparse_grad(int num_tables, const kv_handle_t* tables, const float* const* seg_grads,
                                const void* const* segment_ids, int segment_dtype, const float* const* weights,
                                const int64_t* ns, const int64_t* num_segments, int combiner,
                                float* const* values, kv_stream_t stream) {
  int rc;
  if ((rc = sparse_call_checks(combiner, segment_dtype))) return rc;
  std::vector<int64_t> en;
  if ((rc = multi_sparse_checks(num_tables, tables, ns, num_segments, (const void* const*)values, false,
                                (const void* const*)seg_grads, &en)))
    return rc;
  if (!segment_ids) return fail(KV_INVALID_ARGUMENT, "null argument array");
  if ((rc = multi_common(num_tables, tables, segment_ids, en.data()))) return rc;   // (its id lists: the segment ids)
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));
  // the tables lend their workspaces: neither rows nor records are touched
  if ((rc = lock.enter(s, [](const kv_table*) { return (unsigned)(KEEP_VAR | KEEP_SLOT); }))) return rc;
  auto wts = [&](int i) { return weights ? weights[i] : nullptr; };
  long long nmax = 0, segmax = 0;
  bool any_den = false;
  for (int i = 0; i < num_tables; ++i) {
    if (en[i] == 0) continue;
    const bool need_den = wts(i) != nullptr && combiner != KV_COMBINER_SUM;
    if ((rc = ensure_seg(tables[i], num_segments[i], need_den, s))) return rc;
    any_den |= need_den;
    nmax = std::max<long long>(nmax, en[i]);
    segmax = std::max<long long>(segmax, num_segments[i]);
  }
  if (nmax == 0) return KV_OK;
  Staged<SparseDesc> sd(device, 2, num_tables);
  if (sd.rc) return sd.rc;
  for (int i = 0; i < num_tables; ++i) {
    SparseDesc& q = sd[i];
    if (en[i] == 0) continue;   // (zeroed: nseg == 0, no part in the launches)
    q.seg = segment_ids[i];
    q.wts = wts(i);
    q.off = tables[i]->ws.seg_off;
    q.den = tables[i]->ws.seg_den;
    q.seg_grad = seg_grads[i];
    q.out = values[i];
    q.n = en[i];
    q.nseg = num_segments[i];
  }
  const SparseDesc* sp;
  if ((rc = sd.upload(s, &sp))) return rc;
  // at most three launches: the offsets, the weighted denominators (if any table has them), the expand
  const bool seg32 = segment_dtype == KV_DT_INT32;
  const int D = tables[0]->dim;
  with_id_type(seg32, [&](auto id) {
    using IDT = decltype(id);
    k_seg_offsets_multi<IDT><<<dim3((unsigned)nblocks(nmax + 1, TB, 2048), (unsigned)num_tables), TB, 0, s>>>(sp);
  });
  if (any_den) k_seg_den_multi<<<dim3((unsigned)nblocks(segmax, TB, 4096), (unsigned)num_tables), TB, 0, s>>>(sp, combiner);
  const int lanes = expand_lanes(D);
  const dim3 grid((unsigned)nblocks(nmax * (lanes ? lanes : D), TB, 16384), (unsigned)num_tables);
  with_expand_types(seg32, lanes, [&](auto id, auto vq) {
    k_seg_expand_multi<decltype(id), decltype(vq)::value><<<grid, TB, 0, s>>>(sp, D, combiner);
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_gather_or_zeros(kv_handle_t t, const void* ids, int64_t n, float* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if ((rc = require_initialized(t))) return rc;   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
  if (n == 0) return KV_OK;
  if (n < 0 || !ids || !out) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  // a read: behind the table's last op on whatever stream, no serial bump.  It reads rows and flags of THIS table: as a var
  // it leaves the mirrors alone.  (hand_over, not enter_op: unlike kv_batch_gather_or_zeros this op does not report the
  // deferred error of the table's last batch — the next op that does will)
  if ((rc = hand_over(t, s, KEEP_VAR, true, false))) return rc;
  const TableDev td = dev_view(t);
  const int q = pow2_vectors(t->dim, 64);   // a wave of whole rows (k_gather_or_zeros_w); 0: the 8-lane kernel
  const int gw = nblocks(n, TB, 8192);  // a 64-id step per wave at 1 M ids: residency hides the hops
  with_id_type(t->key_dtype == KV_DT_INT32, [&](auto id) {
    using IDT = decltype(id);
    if (q)
      with_lanes(q, [&](auto vq) { k_gather_or_zeros_w<IDT, decltype(vq)::value><<<gw, TB, 0, s>>>(td, (const IDT*)ids, out, n); });
    else
      k_gather_or_zeros<IDT><<<nblocks(n, TB / 8, 8192), TB, 0, s>>>(td, (const IDT*)ids, out, n);
  });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_batch_gather_or_zeros(int num_tables, const kv_handle_t* tables, const void* const* ids,
                             const int64_t* ns, float* const* outs, kv_stream_t stream) {
  int rc;
  if ((rc = check_same_shape(num_tables, tables, "tables"))) return rc;  // Attr("N: int >= 1")
  if (!ids || !ns || !outs) return fail(KV_INVALID_ARGUMENT, "null argument array");
  for (int i = 0; i < num_tables; ++i) {
    if (ns[i] < 0 || (ns[i] > 0 && (!ids[i] || !outs[i]))) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
    if ((rc = require_initialized(tables[i]))) return rc;   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
  }
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));
  // every table is read on the op's stream: behind whatever its own last op queued on another stream (an optimizer
  // apply that has not finished), and its next op behind this read (rows and flags only: as vars they keep their mirrors)
  for (kv_table* tb : lock.ts)
    if ((rc = enter_op(tb, s, KEEP_VAR, true, false))) return rc;
  Staged<BatchGatherDesc> hd(device, 0, num_tables);
  if (hd.rc) return hd.rc;
  long long nmax = 0;
  for (int i = 0; i < num_tables; ++i) {
    BatchGatherDesc& d = hd[i];
    d.t = dev_view(tables[i]);
    d.ids = ids[i];
    d.out = outs[i];
    d.n = ns[i];
    d.ids_int32 = tables[i]->key_dtype == KV_DT_INT32;
    nmax = std::max<long long>(nmax, ns[i]);
  }
  if (nmax == 0) return KV_OK;
  const BatchGatherDesc* md;
  if ((rc = hd.upload(s, &md))) return rc;
  dim3 grid((unsigned)nblocks(nmax, TB / 8, 2048), (unsigned)num_tables);
  k_batch_gather_or_zeros<<<grid, TB, 0, s>>>(md);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_lookup_sparse_zeros(kv_handle_t t, const void* ids, const void* segment_ids, int segment_dtype,
                           const float* weights, int64_t n, int64_t num_segments, int combiner, float* out,
                           kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if ((rc = sparse_zeros_checks(t, ids, segment_ids, segment_dtype, n, num_segments, combiner, out))) return rc;
  if (num_segments == 0) return KV_OK;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  // a read, entered like kv_gather_or_zeros: behind the table's last op on whatever stream, no serial bump, no workspace;
  // as a var the table keeps its mirrors.  Only the kernel is queued: capturable with no precondition
  if ((rc = hand_over(t, s, KEEP_VAR, true, false))) return rc;
  const TableDev td = dev_view(t);
  const int q = sparse_zeros_lanes(t->dim);
  const int grid = nblocks(num_segments * (q ? q : 64), TB, 8192);
  const int ids32 = t->key_dtype == KV_DT_INT32, seg32 = segment_dtype == KV_DT_INT32;
  if (q)
    with_lanes(q, [&](auto vq) {
      k_lookup_sparse_zeros<decltype(vq)::value><<<grid, TB, 0, s>>>(td, ids, ids32, segment_ids, seg32, weights, (int)n,
                                                                    num_segments, combiner, out);
    });
  else
    k_lookup_sparse_zeros<0><<<grid, TB, 0, s>>>(td, ids, ids32, segment_ids, seg32, weights, (int)n, num_segments, combiner, out);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_batch_lookup_sparse_zeros(int num_tables, const kv_handle_t* tables, const void* const* ids,
                                 const void* const* segment_ids, int segment_dtype, const float* const* weights,
                                 const int64_t* ns, const int64_t* num_segments, int combiner,
                                 float* const* outs, kv_stream_t stream) {
  int rc;
  if ((rc = check_same_shape(num_tables, tables, "tables"))) return rc;
  if (!ids || !segment_ids || !ns || !num_segments || !outs) return fail(KV_INVALID_ARGUMENT, "null argument array");
  for (int i = 0; i < num_tables; ++i)
    if ((rc = sparse_zeros_checks(tables[i], ids[i], segment_ids[i], segment_dtype, ns[i], num_segments[i], combiner, outs[i])))
      return rc;
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));   // (a table listed twice is locked and entered once)
  // entered like kv_batch_gather_or_zeros: every table is read on the op's stream, and reports its deferred error
  for (kv_table* tb : lock.ts)
    if ((rc = enter_op(tb, s, KEEP_VAR, true, false))) return rc;
  Staged<BatchSparseZerosDesc> hd(device, 0, num_tables);
  if (hd.rc) return hd.rc;
  long long work = 0;   // lanes of the table with the most of them
  for (int i = 0; i < num_tables; ++i) {
    BatchSparseZerosDesc& d = hd[i];
    const int q = sparse_zeros_lanes(tables[i]->dim);
    d.t = dev_view(tables[i]);
    d.ids = ids[i];
    d.seg = segment_ids[i];
    d.wts = weights ? weights[i] : nullptr;
    d.out = outs[i];
    d.nseg = num_segments[i];
    d.n = (int)ns[i];
    d.ids_int32 = tables[i]->key_dtype == KV_DT_INT32;
    work = std::max<long long>(work, num_segments[i] * (q ? q : 64));
  }
  if (work == 0) return KV_OK;
  const BatchSparseZerosDesc* md;
  if ((rc = hd.upload(s, &md))) return rc;
  dim3 grid((unsigned)nblocks(work, TB, 4096), (unsigned)num_tables);
  k_batch_lookup_sparse_zeros<<<grid, TB, 0, s>>>(md, segment_dtype == KV_DT_INT32, combiner);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_multi_gather_or_insert_tok(int num_tables, const kv_handle_t* tables, const void* const* ids,
                                  const int32_t* const* counts, const int64_t* ns, float* const* outs,
                                  kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_lookup_impl(num_tables, tables, ids, counts, ns, outs, tokens, stream, -1, nullptr, nullptr);
}
int kv_multi_gather_or_insert(int num_tables, const kv_handle_t* tables, const void* const* ids,
                              const int32_t* const* counts, const int64_t* ns, float* const* outs,
                              kv_stream_t stream) {
  return kv_multi_gather_or_insert_tok(num_tables, tables, ids, counts, ns, outs, nullptr, stream);
}

int kv_dedup_segment_sum(kv_handle_t t, const void* ids, const float* grad, int64_t n, int64_t* uniq,
                         float* summed, int32_t* inverse, int64_t* num_unique, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!num_unique) return fail(KV_INVALID_ARGUMENT, "num_unique is null");
  *num_unique = 0;
  if (n == 0) return KV_OK;
  if (n < 0 || !ids || !grad || !uniq || !summed) return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (n > (fused_tab(t) ? FUSED_MAX_N : (1ll << 21)))
    return fail(KV_UNIMPLEMENTED, "%lld ids in one call (limit 2^%d)", (long long)n, fused_tab(t) ? 23 : 21);
  if (!dim_supported(t->dim)) return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported", t->dim);
  TableOp op(t, stream);
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, op.s, KEEP_VAR | KEEP_SLOT))) return rc;
  return dedup_locked(t, ids, grad, n, uniq, summed, inverse, num_unique, nullptr, KV_SCATTER_ADD, op.s);
}

// ... with the count left on the device: no synchronisation, no blocking copy (the checks are the synchronous form's)
int kv_dedup_segment_sum_dev(kv_handle_t t, const void* ids, const float* grad, int64_t n, int64_t* uniq,
                             float* summed, int32_t* inverse, int64_t* num_unique_dev, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!num_unique_dev) return fail(KV_INVALID_ARGUMENT, "num_unique_dev is null");
  if (n == 0) {
    DeviceGuard dg(t->device);
    HIP_TRY(hipMemsetAsync(num_unique_dev, 0, sizeof(int64_t), (hipStream_t)stream));
    return KV_OK;
  }
  if (n < 0 || !ids || !grad || !uniq || !summed) return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (n > (fused_tab(t) ? FUSED_MAX_N : (1ll << 21)))
    return fail(KV_UNIMPLEMENTED, "%lld ids in one call (limit 2^%d)", (long long)n, fused_tab(t) ? 23 : 21);
  if (!dim_supported(t->dim)) return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported", t->dim);
  TableOp op(t, stream);
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, op.s, KEEP_VAR | KEEP_SLOT))) return rc;
  return dedup_locked(t, ids, grad, n, uniq, summed, inverse, nullptr, num_unique_dev, KV_SCATTER_ADD, op.s);
}

int kv_unsorted_segment_sum(kv_handle_t t, const int32_t* segment_ids, const float* data, int64_t n,
                            int64_t num_segments, float* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n < 0 || num_segments < 0 || num_segments > 0x7FFFFFFFll || (n > 0 && (!segment_ids || !data)) ||
      (num_segments > 0 && !out))
    return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (n > (fused_tab(t) ? FUSED_MAX_N : (1ll << 21)))
    return fail(KV_UNIMPLEMENTED, "%lld rows in one call (limit 2^%d)", (long long)n, fused_tab(t) ? 23 : 21);
  if (!dim_supported(t->dim)) return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported", t->dim);
  if (num_segments == 0) return KV_OK;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, s, KEEP_VAR | KEEP_SLOT))) return rc;
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_segments * t->dim * sizeof(float), s));  // segments nobody names
  if (n == 0) return KV_OK;
  if ((rc = ensure_workspace(t, n, true, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch.drop();
  PartArgs pa = self_part_args(t, n);
  pa.grad = data;
  pa.out_sum = out;
  pa.direct_rows = num_segments;   // no numbering: an id IS its output row
  pa.fold_op = KV_SCATTER_ADD;
  if ((rc = segment_sums(t, wd, pa, segment_ids, n, true, false, "segment sums", s))) return rc;
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_unique(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, int64_t* uniq, int32_t* uniq_counts,
              int32_t* inverse, int64_t* num_unique, int64_t* num_unique_dev, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!num_unique && !num_unique_dev) return fail(KV_INVALID_ARGUMENT, "num_unique and num_unique_dev are both null");
  if (num_unique) *num_unique = 0;
  if (n == 0) {
    if (num_unique_dev) HIP_TRY(hipMemsetAsync(num_unique_dev, 0, sizeof(int64_t), (hipStream_t)stream));
    return KV_OK;
  }
  if (n < 0 || !ids || !uniq) return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (n > FUSED_MAX_N) return fail(KV_UNIMPLEMENTED, "%lld ids in one call (limit 2^23)", (long long)n);
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, s, KEEP_VAR | KEEP_SLOT))) return rc;
  if ((rc = ensure_workspace(t, n, false, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch.drop();
  PartArgs pa = self_part_args(t, n);
  pa.out_keys = (long long*)uniq;
  pa.out_counts = uniq_counts;
  // the entry-list kernels, whatever the table's dim (no row is touched)
  if ((rc = fused_unique_pass(t, wd, pa, ids, counts, n, s))) return rc;
  if (inverse) k_inverse_e<<<nblocks(n, TB, 2048), TB, 0, s>>>(t->ws.pos_ent, wd.ent_b, n, inverse);
  if (num_unique_dev) k_store_count<<<1, 1, 0, s>>>(wd.ctr, (long long*)num_unique_dev);
  HIP_TRY(hipGetLastError());
  if (num_unique) {   // synchronous form
    unsigned U = 0;
    if ((rc = read_count(t, wd.ctr, s, &U))) return rc;
    *num_unique = U;
  }
  return KV_OK;
}

int kv_delete(kv_handle_t t, const void* ids, int64_t n, int64_t* num_deleted, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (num_deleted) *num_deleted = 0;
  if (n < 0 || (n > 0 && !ids)) return fail(KV_INVALID_ARGUMENT, "indices pointer is null");
  if ((rc = require_initialized(t))) return rc;
  if (n == 0) return KV_OK;
  TableOp op(t, stream);
  if ((rc = record_deleted(t, ids, n, t->key_dtype == KV_DT_INT32, op.s))) return rc;
  return delete_locked(t, ids, n, num_deleted, op.s);
}

int kv_delete_with_timestamp(kv_handle_t t, int threshold, int dry_run, int64_t* out_keys, int64_t* count,
                             kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!count || (!dry_run && !out_keys)) return fail(KV_INVALID_ARGUMENT, "count / delete_keys pointer is null");
  if ((rc = require_initialized(t))) return rc;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  if (!dry_run) {   // out_keys was sized by a dry run: nothing may have touched the table (or its clock) since
    if (t->expire_serial != t->op_serial)
      return fail(KV_FAILED_PRECONDITION, "the table was used between the dry run and kv_delete_with_timestamp: the key "
                                          "buffer sized from the count may be too small; count again");
    ++t->op_serial;
    t->batch.drop();   // rows are released: an index of a batch that held them is void (a pending pass: stats settles it below)
  }
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  if (!dry_run && (rc = ensure_free_list(t, s))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  const unsigned thr = (unsigned)(threshold & 0xFFFF);  // static_cast<uint16_t>(threshold), kv_variable.h:771
  k_delete_by_time<<<nblocks(nrows, TB, 4096), TB, 0, s>>>(dev_view(t), nrows, today(t), thr, dry_run ? 0 : 1,
                                                        t->free_rows, t->d_stat, (long long*)out_keys);
  HIP_TRY(hipGetLastError());
  unsigned long long rel = 0;
  if (dry_run) {
    HIP_TRY(hipMemcpyAsync(&rel, t->d_stat, sizeof rel, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else if ((rc = after_release(t, s, &rel))) {
    return rc;
  }
  *count = (int64_t)rel;
  if (dry_run) t->expire_serial = t->op_serial;
  if (!dry_run && (rc = record_deleted(t, out_keys, (int64_t)rel, false, s))) return rc;
  return KV_OK;
}

int kv_get_count(kv_handle_t t, const void* ids, int64_t n, int32_t* counts, kv_stream_t stream) {
  return count_or_ts(t, ids, n, 0, (uint32_t*)counts, stream);
}
int kv_get_timestamp(kv_handle_t t, const void* ids, int64_t n, uint32_t* days, kv_stream_t stream) {
  return count_or_ts(t, ids, n, 1, days, stream);
}

int kv_take_rows(int device, const void* src, const int32_t* index, const int32_t* index_outer, int64_t n,
                 int64_t row_bytes, int scatter, void* out, kv_stream_t stream) {
  if (index_outer && scatter) return fail(KV_INVALID_ARGUMENT, "kv_take_rows: the two-level index is gather only");
  if (n < 0 || row_bytes <= 0 || row_bytes % 4 || (n > 0 && (!src || !index || !out)))
    return fail(KV_INVALID_ARGUMENT, "kv_take_rows: n %lld, row_bytes %lld (a positive multiple of 4)",
                (long long)n, (long long)row_bytes);
  if (n == 0) return KV_OK;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  const bool wide = row_bytes % 16 == 0 && ((uintptr_t)src % 16 == 0) && ((uintptr_t)out % 16 == 0);
  const unsigned nu = (unsigned)(row_bytes / (wide ? 16 : 4));
  const int sh = (nu & (nu - 1)) == 0 ? ilog2(nu) : -1;
  const int grid = nblocks(n * nu, TB * 4, 8192);
  if (wide) {
    if (scatter) k_take_rows<float4, 1><<<grid, TB, 0, s>>>((const float4*)src, index, n, nu, sh, (float4*)out);
    else k_take_rows<float4, 0><<<grid, TB, 0, s>>>((const float4*)src, index, n, nu, sh, (float4*)out, index_outer);
  } else {
    if (scatter) k_take_rows<float, 1><<<grid, TB, 0, s>>>((const float*)src, index, n, nu, sh, (float*)out);
    else k_take_rows<float, 0><<<grid, TB, 0, s>>>((const float*)src, index, n, nu, sh, (float*)out, index_outer);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_export_count(kv_handle_t t, int first_n, int64_t* counts, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  unsigned nrows = 1;
  if ((rc = stats(t, op.s, nullptr, &nrows))) return rc;
  unsigned long long c[3];
  if ((rc = export_pass(t, k_export, nrows, first_n, c, op.s))) return rc;
  t->export_serial = t->op_serial;
  counts[0] = (int64_t)c[0]; counts[1] = (int64_t)c[1]; counts[2] = (int64_t)c[2];
  return KV_OK;
}

int kv_export_fill(kv_handle_t t, int first_n, int64_t* keys, float* values, int64_t* blacklist,
                   int64_t* fkeys, uint32_t* fvals, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  if (t->export_serial != t->op_serial)
    return fail(KV_FAILED_PRECONDITION, "the table was used between kv_export_count and kv_export_fill: the buffers sized "
                                        "from the counts may be too small; count again");
  ++t->op_serial;   // a fill ends the export (delta lists handed on): the next fill needs a new count
  unsigned nrows = 1;
  if ((rc = stats(t, op.s, nullptr, &nrows))) return rc;
  if ((rc = export_pass(t, k_export, nrows, first_n, nullptr, op.s, true, keys, values, blacklist, fkeys, fvals))) return rc;
  if (first_n > 2 && (rc = delta_after_export(t, first_n, nrows, op.s))) return rc;  // dynamic_save.hpp:179-192
  return KV_OK;
}

int kv_set_delta_tracking(kv_handle_t t, int support_delta_export, int support_prediction_delta_export) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, nullptr);
  if ((rc = settle_pending(t))) return rc;
  t->track_delta = support_delta_export != 0;
  t->track_pred = support_prediction_delta_export != 0;
  return KV_OK;
}

int kv_export_delta_count(kv_handle_t t, int first_n, int64_t* counts, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!counts) return fail(KV_INVALID_ARGUMENT, "counts pointer is null");
  if ((rc = require_initialized(t))) return rc;
  TableOp op(t, stream);
  unsigned nrows = 1;
  if ((rc = stats(t, op.s, nullptr, &nrows))) return rc;
  std::vector<long long> absent;
  if ((rc = delta_prepare(t, first_n, op.s, &absent))) return rc;
  unsigned long long c[3];
  if ((rc = export_pass(t, k_export_delta, nrows, first_n, c, op.s))) return rc;
  counts[0] = (int64_t)c[0];
  counts[1] = first_n > 3 ? (int64_t)c[1] : 0;
  counts[2] = first_n > 4 ? (int64_t)(c[2] + absent.size()) : 0;
  counts[3] = (int64_t)absent.size() + (first_n > 3 ? 0 : (int64_t)c[1]);
  t->delta_serial = t->op_serial;
  return KV_OK;
}

int kv_export_delta_fill(kv_handle_t t, int first_n, int64_t* keys, float* values, int64_t* blacklist,
                         int64_t* fkeys, uint32_t* fvals, int64_t* delete_keys, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if ((rc = require_initialized(t))) return rc;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  if (t->delta_serial != t->op_serial)
    return fail(KV_FAILED_PRECONDITION, "the table was used between kv_export_delta_count and kv_export_delta_fill: the "
                                        "buffers sized from the counts may be too small; count again");
  ++t->op_serial;
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  std::vector<long long> absent;
  if ((rc = delta_prepare(t, first_n, s, &absent))) return rc;
  // prediction exports move the blacklisted keys to the delete list (dynamic_save.hpp:345-351)
  unsigned long long c[3];
  if ((rc = export_pass(t, k_export_delta, nrows, first_n, c, s, true, keys, values, first_n > 3 ? blacklist : delete_keys,
                        fkeys, fvals)))
    return rc;
  if (!absent.empty()) {  // keys without a row: deleted (:233-236), frequency 0 (kv_variable.h:950)
    if (!delete_keys) return fail(KV_INVALID_ARGUMENT, "delete_keys pointer is null");
    const size_t off = first_n > 3 ? 0 : (size_t)c[1];
    HIP_TRY(hipMemcpyAsync(delete_keys + off, absent.data(), absent.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    if (first_n > 4 && fkeys && fvals) {
      HIP_TRY(hipMemcpyAsync(fkeys + c[2], absent.data(), absent.size() * sizeof(long long), hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemsetAsync(fvals + c[2], 0, absent.size() * sizeof(uint32_t), s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // `absent` is the copy source
  }
  return delta_after_export(t, first_n, nrows, s);
}

int kv_insert(kv_handle_t t, const void* ids, const float* values, int64_t n, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  if ((rc = enter_op(t, op.s))) return rc;
  return scatter_like(t, ids, values, n, KV_SCATTER_ASSIGN, 1, -1, nullptr, op.s);
}

int kv_scatter_update(kv_handle_t t, const void* ids, const float* updates, int64_t n, int op,
                      kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (op < KV_SCATTER_ASSIGN || op > KV_SCATTER_MAX) return fail(KV_INVALID_ARGUMENT, "unsupported update operation %d", op);
  // a folding operation counts every occurrence of a repeated id: the de-duplication below does that, and it runs on the dims
  // of the fused kernels only.  The per-position path would keep ONE occurrence: refused, before anything is queued
  if (op != KV_SCATTER_ASSIGN && n > 1 && !dim_supported(t->dim))
    return fail(KV_UNIMPLEMENTED, "kv_scatter_update: operation %d on more than one id at embedding dim %d (multiples of 4 up to "
                                  "1024, any dim up to 256; assign, or one id per call, works at every dim)", op, t->dim);
  TableOp tab(t, stream);
  const hipStream_t s = tab.s;
  if ((rc = enter_op(t, s))) return rc;
  if (op != KV_SCATTER_ASSIGN && n > 1 && ids && updates && dim_supported(t->dim)) {
    // ScatterUpdate applies every occurrence of an id in turn (kv_variable.h:616-734): the update rows of a
    // repeated id are combined first (sum for add / sub, product for mul / div, min, max — one row per
    // distinct id), then applied once.  Chunks of 2^21 ids one after another: occurrences in a later
    // chunk meet the row the earlier chunk left, as in the reference's sequential order.
    const int fold = (op == KV_SCATTER_ADD || op == KV_SCATTER_SUB) ? KV_SCATTER_ADD
                   : (op == KV_SCATTER_MUL || op == KV_SCATTER_DIV) ? KV_SCATTER_MUL : op;
    const long long CHK = 1ll << 21;
    const size_t idsz = t->key_dtype == KV_DT_INT32 ? 4 : 8;
    Workspace& w = t->ws;
    const long long want = std::min<long long>(n, CHK);
    if (w.scat_cap < want) {
      if ((rc = ws_sync(s))) return rc;
      const long long cap = std::max<long long>(want, std::min<long long>(w.scat_cap * 2, CHK));
      w.scat_cap = 0;
      if ((rc = regrow(&w.scat_keys, (size_t)cap)) || (rc = regrow(&w.scat_sum, (size_t)cap * t->dim))) return rc;
      w.scat_cap = cap;
    }
    for (long long off = 0; off < n; off += CHK) {
      const long long m = std::min(CHK, (long long)n - off);
      int64_t U = 0;
      if ((rc = dedup_locked(t, (const char*)ids + (size_t)off * idsz, updates + (size_t)off * t->dim, m,
                             (int64_t*)w.scat_keys, w.scat_sum, nullptr, &U, nullptr, fold, s)))
        return rc;
      if (t->key_dtype == KV_DT_INT32 && U > 0)   // the unique list is int64; the table's ops take its own key type
        k_narrow_keys<<<1, 1024, 0, s>>>(w.scat_keys, U);
      if ((rc = scatter_like(t, w.scat_keys, w.scat_sum, U, op, 0, -1, nullptr, s))) return rc;
    }
    return KV_OK;
  }
  // assign: one of the occurrences of a repeated id stays (the reference's result depends on its thread
  // interleaving there); a single id of any operation, at any dim
  return scatter_like(t, ids, updates, n, op, 0, -1, nullptr, s);
}

int kv_import_delta(kv_handle_t t, const int64_t* keys, const float* values, int64_t n, const int64_t* blacklist,
                    int64_t n_black, const int64_t* fkeys, const uint32_t* fvals, int64_t n_freq,
                    const int64_t* delete_keys, int64_t n_delete, int first_n, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  if (t->key_dtype == KV_DT_INT32) return fail(KV_UNIMPLEMENTED, "import with int32 keys");
  if ((rc = enter_op(t, s))) return rc;
  // Stage 1 (dynamic_restore.hpp:58-77): insert or overwrite, lift the blacklist, re-evaluate under_threshold
  if ((rc = scatter_like(t, keys, values, n, KV_SCATTER_ASSIGN, 3, -1, nullptr, s))) return rc;
  // Stage 2 (:92-112): first_n > 3 marks the blacklist, otherwise (inference load) those keys are removed
  if (n_black > 0) {
    if (first_n > 3) {
      if ((rc = scatter_like(t, blacklist, nullptr, n_black, 0, 1, 0, nullptr, s))) return rc;
    } else if ((rc = delete_locked(t, blacklist, n_black, nullptr, s))) {
      return rc;
    }
  }
  // Stage 3/4 (:114-135): frequency words of keys that exist
  if (n_freq > 0 && (rc = scatter_like(t, fkeys, nullptr, n_freq, 0, 1, 1, fvals, s))) return rc;
  // Stage 5 (:137-145): keys deleted since the checkpoint this delta follows
  if (n_delete > 0 && (rc = delete_locked(t, delete_keys, n_delete, nullptr, s))) return rc;
  if ((rc = ensure_init_placeholder(t, s))) return rc;
  t->initialized = true;
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_import(kv_handle_t t, const int64_t* keys, const float* values, int64_t n, const int64_t* blacklist,
              int64_t n_black, const int64_t* fkeys, const uint32_t* fvals, int64_t n_freq,
              kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  TableOp op(t, stream);
  const hipStream_t s = op.s;
  if (t->key_dtype == KV_DT_INT32) return fail(KV_UNIMPLEMENTED, "import with int32 keys");
  if ((rc = enter_op(t, s))) return rc;
  // clear(): dynamic_restore.hpp:60-62
  HIP_TRY(hipStreamSynchronize(s));
  t->gen += 1;            // row ids start over: slot-row hints into this table are void
  t->slot_uid = 0;        // and the fresh index carries none of its own
  t->batch.drop();
  unsigned init[3] = {1, 0, 0};
  HIP_TRY(hipMemcpy(t->d_counters, init, sizeof init, hipMemcpyHostToDevice));  // stack source: synchronous
  launch_fill_entries(t, s);
  t->rows_ub = 1;
  t->idx_ub = t->idx_base = 0; t->bump_base = 1; t->pushes_since = 0; t->free_base = 0; t->free_known = 0;
  t->del_train.clear(); t->del_pred.clear();  // dynamic_restore.hpp:258-259 (the rows start over, and so do their bytes)
  if ((rc = scatter_like(t, keys, values, n, KV_SCATTER_ASSIGN, 2, -1, nullptr, s))) return rc;
  if (n_black > 0 && (rc = scatter_like(t, blacklist, nullptr, n_black, 0, 1, 0, nullptr, s))) return rc;
  if (n_freq > 0 && (rc = scatter_like(t, fkeys, nullptr, n_freq, 0, 1, 1, fvals, s))) return rc;
  if ((rc = ensure_init_placeholder(t, s))) return rc;
  t->initialized = true;
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

}  // extern "C"
