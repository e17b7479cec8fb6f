// kv_apply.hip — the optimizer layer of the C ABI on the table core (kv_host.h): one parser per optimizer family, the two
// bodies (apply_one: one table; multi_apply: many tables, one launch per stage; the PartArgs of all their launches start
// from opt_part_args), the 42 kv_apply_* / kv_multi_apply_* entry points and kv_attach_slot.  It compiles no kernel: the
// optimizers' kernels are reached through the typed launchers of kv_launch.h, the pipelines' through the core's.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kv_host.h"

using namespace kvhip_internal;

namespace {

// The slot table whose rows the var's index entries remember (Entry::hint): the first slot-0 table an
// optimizer uses with the var, or the one kv_attach_slot names.  Hints of a table that was cleared since
// (import) mean nothing any more and are forgotten; another table simply goes without hints.
static bool claim_slot(kv_table* v, kv_table* sl, hipStream_t s) {
  if (v->slot_uid == sl->uid && v->slot_gen == sl->gen) return true;
  if (v->slot_uid != 0 && v->slot_uid != sl->uid) return false;
  if (v->slot_uid == sl->uid)   // same table, cleared since
    launch_clear_hints(v, s);
  v->slot_uid = sl->uid;
  v->slot_gen = sl->gen;
  return true;
}

// the 16-bit stamp of the unique-ids launches wraps (once per 65535 launches): every row back to "none", in front of the
// launch that takes the next serial
static void wrap_uniq_serial(kv_table* v, hipStream_t s) {
  if (v->uniq_serial < 65535u) return;
  launch_clear_stamps(v, s);
  v->uniq_serial = 0;
}

// What the PartArgs of every optimizer launch starts from: the var's and slots' views, the hyperparameters with the var's
// fast-math flag, the gradient rows, the day, the batch size and whether the var's hints name s0 (claim_slot: in front of
// the site's mirror_decide).  det, day_lk / count_once, epart and uniq_serial are the sites' own.
static void opt_part_args(PartArgs& pa, kv_table* v, kv_table* s0, kv_table* s1, const OptArgs& a, const float* grad, long long n,
                          hipStream_t s) {
  pa.tv = dev_view(v); pa.ts0 = dev_view(s0); pa.ts1 = s1 ? dev_view(s1) : pa.ts0;
  pa.opt = a; pa.grad = grad; pa.day = today(v);
  pa.opt.fast = fast_math_on(v) ? 1 : 0;
  pa.n = n;
  pa.use_hints = claim_slot(v, s0, s) ? 1 : 0;
}

// ... and the optimizer apply over the tiles' entries: the tile sums of the repeated ids (k_tsum; tile_ids != nullptr: the
// batch's tile pass has not run yet and runs in the same launch, k_ltsum), then partition pass + update in one launch
// (k_papply, kv_papply.h: pa_mode = PA_LOOKUP / PA_APPLYIDX / PA_NONE)
template <int OPT>
int fused_apply(kv_table* v, WsDev& wd, PartArgs& pa, long long n, hipStream_t s, int pa_mode, const void* tile_ids = nullptr) {
  pa.epart = wd.epart;
  if (tile_ids) {
    ProfScope ps(v, KV_PROF_APPLY_TILE, s);
    const int rc = launch_ltsum(pa.tv, wd, tile_ids, v->key_dtype == KV_DT_INT32 ? 1 : 0, n, v->deterministic ? 1 : 0,
                                pa.grad, s);
    if (rc) return fail(rc, "tile pass + tile sums: no kernel for dim %d", pa.tv.dim);
  } else {
    ProfScope ps(v, KV_PROF_APPLY_TSUM, s);
    const int rc = launch_tsum(pa.tv, wd, pa.grad, s);
    if (rc) return fail(rc, "tile sums: no kernel for dim %d", pa.tv.dim);
  }
  ProfScope ps(v, KV_PROF_APPLY_SORTED, s);
  const int rc = launch_papply<OPT>(wd, pa, pa_mode, s);
  if (rc) return fail(rc, "partition + apply pass: no kernel for dim %d", pa.tv.dim);
  return KV_OK;
}

// What the wide-slot ops call their slot table and say about its shape (the reference's wording where it has an op), one
// row per optimizer, for apply_one and the batched body alike: a new wide-slot OPT_* gets the neutral row until it has its
// own.  same_first: the same-table test comes in front of the shape test.  (Behind it the test is never reached — a table
// never has a multiple of its own dim; the older ops keep their order and answer var == slot with the shape message.)
struct WideSlotWords { const char* slot; const char* shape; const char* mult; bool same_first; };
static WideSlotWords wide_slot_words(int opt) {
  switch (opt) {
    case OPT_ADAM_V4: case OPT_ADAM_V3:
      return {"m_v_linear", "kv_variable and linear do not have the same shape [%d] [%d] (m_v_linear must be 3x)", "", false};
    case OPT_GROUP_RADAM:
      return {"opt", "kv_variable and opt_shape do not have the same shape [%d] [%d] (opt must be 5x)", "", false};
    case OPT_ADAM: return {"m_v", "var and m_v do not have matching shapes [%d] [%d] (m_v must be 2x)", ": m_v must be 2x", true};
    default: return {"slot", "var and slot do not have matching shapes [%d] [%d]", "", false};
  }
}

// shared body of the batched optimizer ops: slots1 only for the FTRL family (linear); slot_mult = slot dim / var dim.
// unique and the capture rule: as apply_common's.  require_reuse: the batched sharded apply — the tables must still hold
// their lookups' indexes — and, selfs (one per table), read their ranks' own segments in place.
template <int OPT>
static int multi_apply_common(int num_tables, const kv_handle_t* vars, const kv_handle_t* slots0,
                              const kv_handle_t* slots1, int slot_mult, const float* const* grads,
                              const void* const* ids, const int64_t* ns, const OptArgs& hp, kv_stream_t stream,
                              const kv_batch_token_t* tokens, bool unique, bool require_reuse, const SelfSegment* selfs) {
  int rc;
  if ((rc = multi_common(num_tables, vars, ids, ns))) return rc;
  if ((rc = check_same_shape(num_tables, slots0, "slot tables"))) return rc;
  if (slots1 && (rc = check_same_shape(num_tables, slots1, "slot tables"))) return rc;
  if (!grads) return fail(KV_INVALID_ARGUMENT, "null argument array");
  const int D = vars[0]->dim;
  if ((D & 3) != 0 || !dim_supported(D))
    return fail(KV_UNIMPLEMENTED, "batched optimizer op: embedding dim %d (multiples of 4 up to 1024)", D);
  OptArgs a = hp;
  a.l21_norm = a.l21 * std::sqrt((float)D);   // training_ops.cc:728
  std::vector<kv_table*> all;
  for (int i = 0; i < num_tables; ++i) {
    for (const kv_handle_t* sl : {slots0, slots1}) {
      if (!sl) continue;
      if ((rc = require_initialized(sl[i], "optimizer slot"))) return rc;
      if (sl[i]->dim != slot_mult * D || sl[i]->device != vars[0]->device || sl[i]->key_dtype != vars[0]->key_dtype)
        return fail(KV_INVALID_ARGUMENT, "var and slot do not have matching shapes (slot dim must be %d x var dim, same device / key dtype)%s",
                    slot_mult, wide_slot_words(OPT).mult);
      all.push_back(sl[i]);
    }
    if (ns[i] > 0 && !grads[i]) return fail(KV_INVALID_ARGUMENT, "grad pointer is null");
    all.push_back(vars[i]);
  }
  {
    std::vector<kv_table*> u(all);
    std::sort(u.begin(), u.end());
    if (std::adjacent_find(u.begin(), u.end()) != u.end())
      return fail(KV_INVALID_ARGUMENT, "batched op: a table is listed twice (var or slot)");
  }
  const int device = vars[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(all);
  // GroupAdam / Adagrad over pairs (var_i, slot_i): the lean update works on the var rows' slot mirrors (mirror_decide per
  // table below); FTRL reads and writes the slot tables' own records: its entry ends the tables' epochs
  auto keep = [&](const kv_table* tb) -> unsigned {
    unsigned k = KEEP_NONE;
    if (!two_slots(OPT))
      for (int i = 0; i < num_tables; ++i) k |= (vars[i] == tb ? KEEP_VAR : KEEP_NONE) | (slots0[i] == tb ? KEEP_SLOT : KEEP_NONE);
    return k;
  };
  if (unique && fused_ok(D) && !stream_is_capturing(s)) {
    // The caller promises that no table's ids hold an id twice (kv_multi_apply_*_unique; kv_uapply.h): ONE launch for all
    // tables, one lane group per id (grid.y = table).  Pending lookup passes are settled first.
    long long nmax = 0;
    if ((rc = lock.enter(s, keep))) return rc;
    for (int i = 0; i < num_tables; ++i) {
      if ((rc = ensure_capacity(vars[i], ns[i], s)) || (rc = ensure_capacity(slots0[i], ns[i], s)) ||
          (slots1 && (rc = ensure_capacity(slots1[i], ns[i], s))))
        return rc;
      nmax = std::max<long long>(nmax, ns[i]);
    }
    if (nmax == 0) return KV_OK;
    Staged<MultiDesc> hd(device, 1, num_tables);
    if (hd.rc) return hd.rc;
    for (int i = 0; i < num_tables; ++i) {
      kv_table* v = vars[i];
      wrap_uniq_serial(v, s);
      MultiDesc& d = hd[i];
      opt_part_args(d.a, v, slots0[i], slots1 ? slots1[i] : nullptr, a, grads[i], ns[i], s);
      if ((rc = mirror_decide(v, slots0[i], d.a, !two_slots(OPT), s))) return rc;
      d.a.uniq_serial = ns[i] > 0 ? ++v->uniq_serial : 0u;
      d.ids = ids[i];
      d.n = ns[i];
    }
    const MultiDesc* md;
    if ((rc = hd.upload(s, &md))) return rc;
    const int ids32 = vars[0]->key_dtype == KV_DT_INT32 ? 1 : 0;
    ProfScope ps(vars[0], KV_PROF_APPLY_UNIQUE, s);
    rc = launch_uapply<OPT>(hd[0].a, nullptr, ids32, nmax, s, md, num_tables);
    if (rc) return fail(rc, "batched unique apply: no kernel for dim %d", D);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  // The entry-list kernels (fused_ok): every table still holds the tiles' entries of its batch (kv_multi_gather_or_insert_tok)
  // and every token matches -> k_papply_multi over them: PA_LOOKUP when the lookups' partition passes are still pending (it
  // completes them together with the update), PA_NONE when they have been settled since.  One stale token and all tables
  // are indexed again (PA_APPLYIDX: one launch either way); pending passes that are not taken over are settled on entry.
  const bool fz = fused_ok(D);
  bool reuse = tokens != nullptr && fz;       // every table holds its batch's entries
  bool pa_reuse = reuse;                      // ... and its partition pass is still pending
  for (int i = 0; i < num_tables && reuse; ++i)
    if (ns[i] > 0) {
      const BatchIndex::Plan p = vars[i]->batch.plan(tokens[i], ns[i], fz);
      if (!BatchIndex::takes_entries(p)) reuse = false;
      if (p != BatchIndex::TAKE_PENDING) pa_reuse = false;
    }
  if (!reuse) pa_reuse = false;
  for (kv_table* tb : lock.ts) {
    bool taken = false;   // this table's pending pass is taken over by k_papply_multi
    if (pa_reuse)
      for (int i = 0; i < num_tables; ++i) taken = taken || (vars[i] == tb && ns[i] > 0);
    if ((rc = enter_op(tb, s, keep(tb), !taken))) return rc;
  }
  // (a table whose pass was pending while another's was not: hand_over has just settled it — the batch's entries stay valid)
  long long nmax = 0;
  if (require_reuse && !reuse)
    return fail(KV_FAILED_PRECONDITION, "batched sharded apply: another op used a table since this batch's lookup");
  for (int i = 0; i < num_tables; ++i) {
    if (!reuse) vars[i]->batch.drop();
    if (!reuse && (rc = ensure_capacity(vars[i], ns[i], s))) return rc;
    if ((rc = ensure_capacity(slots0[i], ns[i], s))) return rc;
    if (slots1 && (rc = ensure_capacity(slots1[i], ns[i], s))) return rc;
    if ((rc = ensure_workspace(vars[i], std::max<long long>(ns[i], 1), true, s))) return rc;
    nmax = std::max<long long>(nmax, ns[i]);
  }
  if (nmax == 0) return KV_OK;
  Staged<MultiDesc> hd(device, 1, num_tables);
  if (hd.rc) return hd.rc;
  WsDev wmax{};
  for (int i = 0; i < num_tables; ++i) {
    MultiDesc& d = hd[i];
    d.w = ws_view(vars[i], std::max<long long>(ns[i], 1), selfs ? &selfs[i] : nullptr);
    if (fz) { d.a.epart = d.w.epart; use_partitions(d.w, fused_default_P(std::max<long long>(ns[i], 1))); }
    opt_part_args(d.a, vars[i], slots0[i], slots1 ? slots1[i] : nullptr, a, grads[i], ns[i], s);
    d.a.det = vars[i]->deterministic ? 1 : 0;
    if ((rc = mirror_decide(vars[i], slots0[i], d.a, fz && !two_slots(OPT), s))) return rc;   // (fz: k_papply_multi; else the sorted-position kernels, no mirrors)
    d.ids = ids[i];
    d.n = ns[i];
    if (ns[i] == 0) d.w.ntiles = 0;
    if (reuse && ns[i] > 0 && vars[i]->batch.P()) use_partitions(d.w, vars[i]->batch.P());   // the lookup's partitioning
    d.a.day_lk = d.a.day;
    if (pa_reuse && ns[i] > 0) {   // the pending lookup's own day stamp and counting rule
      PartArgs pend;
      take_pending_part(vars[i], &pend);
      d.a.day_lk = pend.day; d.a.count_once = pend.count_once;
    }
    widen(wmax, d.w);
  }
  const MultiDesc* md;
  if ((rc = hd.upload(s, &md))) return rc;
  if (fz) {
    // partition pass + update in one launch (k_papply_multi) behind the tile sums; an optimizer that meets the ids first
    // runs the tile pass of all tables in front (PA_APPLYIDX)
    int pa_mode = pa_reuse ? PA_LOOKUP : PA_NONE;
    if (!reuse) {
      launch_ltile(vars[0], hd[0].a.tv, wmax, nullptr, nullptr, nmax, nullptr, s, -1, md, num_tables, false);
      pa_mode = PA_APPLYIDX;
      for (int i = 0; i < num_tables; ++i)
        if (ns[i] > 0) vars[i]->batch.publish(++g_serial, ns[i], BatchIndex::ENTRIES, hd[i].w.P);
    }
    if ((rc = launch_tsum(hd[0].a.tv, wmax, nullptr, s, md, num_tables)))
      return fail(rc, "tile sums: no kernel for dim %d", D);
    rc = launch_papply<OPT>(wmax, hd[0].a, pa_mode, s, md, num_tables);
    if (rc) return fail(rc, "partition + apply pass: no kernel for dim %d", D);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  launch_tile<false>(vars[0], wmax, nullptr, nullptr, nmax, s, -1, md, num_tables, wmax.ntiles);
  launch_part_keys<MODE_APPLYIDX>(wmax, hd[0].a, s, md, num_tables);
  launch_order(hd[0].a.tv, wmax, nmax, s, md, num_tables);
  if ((rc = launch_apply<MODE_APPLY, OPT>(vars[0], wmax, hd[0].a, nmax, s, md, num_tables))) return rc;
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// shared body of the optimizer ops.  `token` names the batch index a lookup left in the var's workspace
// (kv_gather_or_insert_tok): the same ids, so the index pass is skipped.  unique: the caller promises unique ids
// (kv_apply_*_unique), the one-launch path.  Its duplicate guard stamps rows with a launch serial that lives on the HOST: a
// captured launch would be replayed with the serial it was captured with and find its own stamps.  Under stream capture the
// unique forms therefore run the batch pipeline (which needs no promise; same results, bit for bit): stream_is_capturing().
// The caller holds the locks.  self: kv_shard_apply_serve's own segment, read in place.  counted (kv_apply_unique_counted,
// with unique): n bounds the batch, the kernel reads the count from the device; apply_one has refused what only the batch
// pipeline serves.
template <int OPT>
static int apply_common(kv_table* v, kv_table* s0, kv_table* s1, const float* grad, const void* ids, int64_t n,
                        const OptArgs& a, kv_batch_token_t token, hipStream_t s, bool unique, const SelfSegment* self,
                        const DevCount* counted) {
  const long long nmax = fused_tab(v) ? FUSED_MAX_N : (1ll << 21);
  if (n < 0 || n > nmax)
    return fail(n < 0 ? KV_INVALID_ARGUMENT : KV_UNIMPLEMENTED,
                "indices: %lld ids in one optimizer call (limit %lld for this embedding dim; split the batch)", (long long)n, nmax);
  if (n > 0 && (!grad || !ids)) return fail(KV_INVALID_ARGUMENT, "grad / indices pointer is null");
  if (!dim_supported(v->dim))
    return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported by the fused kernels", v->dim);
  int rc;
  if (counted && (!unique || !fused_ok(v->dim) || stream_is_capturing(s)))
    return fail(KV_INTERNAL, "counted apply off the one-launch path");
  if (unique && fused_ok(v->dim) && !stream_is_capturing(s)) {
    // The caller promises unique ids (kv_apply_*_unique; kv_uapply.h): one launch, one lane group per id.  A pending
    // partition pass was settled by the caller's hand_over (no token is given).  Dims the kernel does not serve take the
    // batch pipeline below, which needs no promise.
    if ((rc = ensure_capacity(v, n, s)) || (rc = ensure_capacity(s0, n, s)) || (s1 && (rc = ensure_capacity(s1, n, s)))) return rc;
    wrap_uniq_serial(v, s);
    PartArgs pa{};
    opt_part_args(pa, v, s0, s1, a, grad, n, s);
    if ((rc = mirror_decide(v, s0, pa, !two_slots(OPT), s))) return rc;
    pa.uniq_serial = ++v->uniq_serial;
    ProfScope ps(v, KV_PROF_APPLY_UNIQUE, s);
    if (counted) rc = launch_uapply<OPT>(pa, ids, counted->ids32, n, s, nullptr, 0, counted->n_dev);
    else rc = launch_uapply<OPT>(pa, ids, v->key_dtype == KV_DT_INT32 ? 1 : 0, n, s);
    if (rc) return fail(rc, "unique apply: no kernel for dim %d", v->dim);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  // What the token is worth (BatchIndex::plan), and with it the apply's kernels.  The entry-list ones: the tile sums, then
  // k_papply — the partition pass and the update in one launch — in the mode the batch's state asks for:
  //   PA_LOOKUP    TAKE_PENDING: the token names the lookup whose partition pass is still pending: k_papply completes its bookkeeping too
  //   PA_NONE      TAKE_DONE: the token names a batch whose bookkeeping is done (a second optimizer on the token; a pass another op settled)
  //   PA_APPLYIDX  REBUILD on a table of their dims: the optimizer meets the ids first — the tile pass runs with the tile sums (k_ltsum)
  // TAKE_SORTED, and REBUILD on any other table: the sorted positions and the segmented fold over them (launch_apply).
  const BatchIndex::Plan plan = v->batch.plan(token, n, fused_tab(v));
  const bool reuse = plan != BatchIndex::REBUILD;
  const bool entries = reuse ? BatchIndex::takes_entries(plan) : fused_tab(v);
  const int pa_mode = plan == BatchIndex::TAKE_PENDING ? PA_LOOKUP : reuse ? PA_NONE : PA_APPLYIDX;
  PartArgs pend{};
  const void* tile_ids = nullptr;   // != nullptr: the batch's tile pass runs in front of the apply (k_ltsum)
  if (plan == BatchIndex::TAKE_PENDING) take_pending_part(v, &pend);
  else if ((rc = flush_part(v, s))) return rc;   // (a pass nobody takes over; the caller's entry left it only to a token of this batch)
  if (!reuse && (rc = ensure_capacity(v, n, s))) return rc;
  if ((rc = ensure_capacity(s0, n, s))) return rc;
  if (s1 && (rc = ensure_capacity(s1, n, s))) return rc;
  if ((rc = ensure_workspace(v, n, true, s))) return rc;
  WsDev wd = ws_view(v, n, self);
  PartArgs pa{};
  opt_part_args(pa, v, s0, s1, a, grad, n, s);
  pa.det = det_mode(v);
  pa.day_lk = pa.day;
  if (pa_mode == PA_LOOKUP) { pa.day_lk = pend.day; pa.count_once = pend.count_once; }
  if (!reuse) {
    if (entries) {   // tile pass + tile sums in one launch, then partition pass + update in one launch
      choose_partitions(v, wd, n);
      tile_ids = ids;
    } else {
      index_pass<MODE_APPLYIDX>(v, wd, pa, ids, nullptr, n, -1, nullptr, s);
    }
    // the index stays valid for this batch (e.g. a second optimizer on the same ids)
    v->batch.publish(++g_serial, n, entries ? BatchIndex::ENTRIES : BatchIndex::SORTED, wd.P);
  } else if (entries && v->batch.P()) {
    use_partitions(wd, v->batch.P());   // the lookup's partitioning
  }
  if ((rc = mirror_decide(v, s0, pa, entries && !two_slots(OPT), s))) return rc;
  if (entries) rc = fused_apply<OPT>(v, wd, pa, n, s, pa_mode, tile_ids);
  else rc = launch_apply<MODE_APPLY, OPT>(v, wd, pa, n, s);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// ---- the optimizer ops -----------------------------------------------------------------------------------------------

// the hyperparameter checks the reference's ops share, in their order and wording (an op without l21 / lr_power / l2s
// passes 0 for it)
static int check_hp(float lr, float l1, float l2, float l21, float lr_power, float l2s) {
  if (!(lr > 0.f)) return fail(KV_INVALID_ARGUMENT, "lr is not a positive scalar: %g", lr);
  if (!(l1 >= 0.f)) return fail(KV_INVALID_ARGUMENT, "l1 regularization strength is not a non-negative scalar: %g", l1);
  if (!(l2 >= 0.f)) return fail(KV_INVALID_ARGUMENT, "l2 regularization strength is not a non-negative scalar: %g", l2);
  if (!(l21 >= 0.f)) return fail(KV_INVALID_ARGUMENT, "l21 regularization strength is not a non-negative scalar: %g", l21);
  if (!(lr_power <= 0.f)) return fail(KV_INVALID_ARGUMENT, "lr_power is not a non-positive scalar: %g", lr_power);
  if (!(l2s >= 0.f)) return fail(KV_INVALID_ARGUMENT, "l2 shrinkage regularization strength is not a non-negative scalar: %g", l2s);
  return KV_OK;
}

// GroupAdam V4 / V3 (training_ops.cc:7001-7120, 5730-5849); slot row = m | v | z
static OptCall group_adam_call(int version, float lr, float b1p, float b2p, float b1, float b2, float eps, float l1, float l2,
                               float l21) {
  OptCall c;
  if (version != 3 && version != 4) {
    c.status = fail(KV_INVALID_ARGUMENT, "GroupAdam version %d: 3 or 4", version);
    return c;
  }
  c.opt = version == 4 ? OPT_ADAM_V4 : OPT_ADAM_V3;
  c.slot_mult = 3;
  if ((c.status = check_hp(lr, l1, l2, l21, 0.f, 0.f))) return c;
  OptArgs& a = c.a;
  a.lr = lr; a.b1p = b1p; a.b2p = b2p; a.b1 = b1; a.b2 = b2; a.eps = eps;
  if (version == 4) {  // training_ops.cc:7111-7120
    a.l1 = l1 * lr; a.l2 = l2 * lr; a.l21 = l21 * lr;
    a.alpha = lr * std::sqrt(1.f - b2p) / (1.f - b1p);
  } else {             // :5840-5849
    a.l1 = l1; a.l2 = l2; a.l21 = l21;
    a.alpha = std::sqrt(1.f - b2p) / (1.f - b1p);
  }
  return c;
}
// Adagrad (training_ops.cc:1372-1498): no checks of its own arguments
static OptCall adagrad_call(float lr, int update_slots) {
  OptCall c;
  c.opt = OPT_ADAGRAD;
  c.a.lr = lr; c.a.update_slots = update_slots;
  return c;
}
// SparseGroupFtrl (training_ops.cc:684-763); slots accum, linear
static OptCall sparse_group_ftrl_call(float lr, float l1, float l2, float l21, float l2s, float lr_power) {
  OptCall c;
  c.opt = OPT_FTRL;
  if ((c.status = check_hp(lr, l1, l2, l21, lr_power, l2s))) return c;
  c.a.lr = lr; c.a.l1 = l1; c.a.l2 = l2; c.a.l21 = l21; c.a.l2s = l2s; c.a.lr_power = lr_power;
  return c;
}
// FTRL-V2 (opt = OPT_FTRL_V2) and group FTRL-V2 (OPT_GROUP_FTRL_V2): the checks of the reference's Compute
// (training_ops.cc:281-440, 805-960), then the SparseGroupFtrl pipeline with the op's own row math
static OptCall ftrl_v2_call(int opt, float lr, float l1, float l2, float l2s, float lr_power) {
  OptCall c;
  c.opt = opt;
  if ((c.status = check_hp(lr, l1, l2, 0.f, lr_power, l2s))) return c;
  c.a.lr = lr; c.a.l1 = l1; c.a.l2 = l2; c.a.l2s = l2s; c.a.lr_power = lr_power;
  return c;
}

// Group RectifiedAdam (training_ops.cc:6714-6820; row math :6883-6936); slot row = m | v | linear | vhat | vamsgrad.
// alpha = sqrt(1 - beta2_power) (:6884) and 1 - beta1_power (:6895) once, in fp32
static OptCall group_radam_call(float lr, float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21,
                                float r_t, int tractable, int amsgrad, int use_nesterov) {
  OptCall c;
  c.opt = OPT_GROUP_RADAM;
  c.slot_mult = slot0_blocks(OPT_GROUP_RADAM);
  if ((c.status = check_hp(lr, l1, l2, l21, 0.f, 0.f))) return c;
  OptArgs& a = c.a;
  a.lr = lr; a.b1p = b1p; a.b2p = b2p; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.l1 = l1; a.l2 = l2; a.l21 = l21;
  radam_r_t(a) = r_t;
  radam_c1(a) = 1.f - b1p;
  a.alpha = std::sqrt(1.f - b2p);
  radam_flags(a) = (tractable ? RADAM_TRACTABLE : 0) | (amsgrad ? RADAM_AMSGRAD : 0) | (use_nesterov ? RADAM_NESTEROV : 0);
  return c;
}

// Plain Adam: the reference composes it from generic ops (python/training/adam.py:93-163), so the checks are this
// library's own.  slot row = m | v.  lr_t (adam.py:142-144) in fp32 in the composition's order; a power at or above 1 would
// make it inf or nan
static OptCall adam_call(float lr, float b1p, float b2p, float b1, float b2, float eps) {
  OptCall c;
  c.opt = OPT_ADAM;
  c.slot_mult = slot0_blocks(OPT_ADAM);
  if (!(lr > 0.f)) { c.status = fail(KV_INVALID_ARGUMENT, "lr is not a positive scalar: %g", lr); return c; }
  if (!(b1p < 1.f)) { c.status = fail(KV_INVALID_ARGUMENT, "beta1_power is not below 1: %g", b1p); return c; }
  if (!(b2p < 1.f)) { c.status = fail(KV_INVALID_ARGUMENT, "beta2_power is not below 1: %g", b2p); return c; }
  OptArgs& a = c.a;
  a.lr = lr; a.b1p = b1p; a.b2p = b2p; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.alpha = (lr * std::sqrt(1.f - b2p)) / (1.f - b1p);
  adam_omb1(a) = 1.f - b1;
  adam_omb2(a) = 1.f - b2;
  return c;
}

// the one place where a runtime OPT_* becomes the template argument of the pipelines
template <class F>
static int with_opt(int opt, F&& f) {
  switch (opt) {
    case OPT_ADAM_V4: return f(std::integral_constant<int, OPT_ADAM_V4>());
    case OPT_ADAM_V3: return f(std::integral_constant<int, OPT_ADAM_V3>());
    case OPT_ADAGRAD: return f(std::integral_constant<int, OPT_ADAGRAD>());
    case OPT_FTRL: return f(std::integral_constant<int, OPT_FTRL>());
    case OPT_FTRL_V2: return f(std::integral_constant<int, OPT_FTRL_V2>());
    case OPT_GROUP_FTRL_V2: return f(std::integral_constant<int, OPT_GROUP_FTRL_V2>());
    case OPT_GROUP_RADAM: return f(std::integral_constant<int, OPT_GROUP_RADAM>());
    case OPT_ADAM: return f(std::integral_constant<int, OPT_ADAM>());
    default: return fail(KV_INTERNAL, "optimizer %d", opt);
  }
}

}  // namespace

namespace __attribute__((visibility("hidden"))) kvhip_internal {
// The sharded ops' `optimizer` code is the OPT_* value; their hp[] layout:
// 0 GroupAdam V4, 1 GroupAdam V3 (hp = lr, beta1_power, beta2_power, beta1, beta2, epsilon, l1, l2, l21),
// 2 Adagrad (hp = lr, update_slots), 3 SparseGroupFtrl (hp = lr, l1, l2, l21, l2_shrinkage, lr_power; slot1 = linear),
// 4 FTRL-V2 / 5 group FTRL-V2 (hp = lr, l1, l2, l2_shrinkage, lr_power; slot1 = linear),
// 6 group RectifiedAdam (hp = lr, beta1_power, beta2_power, beta1, beta2, epsilon, l1, l2, l21, r_t, tractable, amsgrad,
// use_nesterov; the three flags as 0 / 1),
// 7 Adam (hp = lr, beta1_power, beta2_power, beta1, beta2, epsilon; slot0 = m_v)
OptCall shard_opt_call(int optimizer, const float* hp) {
  switch (optimizer) {
    case OPT_ADAM_V4: case OPT_ADAM_V3:
      return group_adam_call(optimizer == OPT_ADAM_V4 ? 4 : 3, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7], hp[8]);
    case OPT_ADAGRAD: return adagrad_call(hp[0], hp[1] != 0.f);
    case OPT_FTRL: return sparse_group_ftrl_call(hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]);
    case OPT_FTRL_V2: case OPT_GROUP_FTRL_V2: return ftrl_v2_call(optimizer, hp[0], hp[1], hp[2], hp[3], hp[4]);
    case OPT_GROUP_RADAM:
      return group_radam_call(hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7], hp[8], hp[9], hp[10] != 0.f, hp[11] != 0.f,
                              hp[12] != 0.f);
    case OPT_ADAM: return adam_call(hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]);
    default: return OptCall{};
  }
}

// One table (s1: the linear table of the FTRL family).  The reference's single-table ops check, in this order: the handles,
// the optimizer itself (GroupAdam version), the tables' initialisation, the hyperparameters, the shapes.  So c.status is
// reported at its place in that order (nothing calls fail() before it unless it returns).  The batched ops report it first.
int apply_one(const OptCall& c, kv_table* v, kv_table* s0, kv_table* s1, const float* grad, const void* ids, int64_t n,
              kv_batch_token_t token, kv_stream_t stream, bool unique, const SelfSegment* self, const DevCount* counted) {
  int rc;
  const bool two = two_slots(c.opt);
  if ((rc = check_table(v)) || (rc = check_table(s0)) || (two && (rc = check_table(s1)))) return rc;
  if (c.status && c.opt < 0) return c.status;
  const WideSlotWords ww = wide_slot_words(c.opt);
  if (wide_slot(c.opt)) {   // order and wording of training_ops.cc:7001-7103 (group RectifiedAdam: :6714-6721)
    if ((rc = require_initialized(v, "var")) || (rc = require_initialized(s0, ww.slot))) return rc;
  } else if (!two) {
    if (!v->initialized || !s0->initialized)
      return fail(KV_FAILED_PRECONDITION, "Attempting to use uninitialized variables: %s", !v->initialized ? "var" : "accum");
  } else if ((rc = require_initialized(v, nullptr)) || (rc = require_initialized(s0, nullptr)) || (rc = require_initialized(s1, nullptr))) {
    return rc;
  }
  if (c.status) return c.status;
  if (wide_slot(c.opt)) {
    // (group RectifiedAdam: the reference's shape check (:6790-6805) also lets an opt dim EQUAL to the var's through and
    // would then read four blocks past the row; here only 5x passes)
    if (ww.same_first && v == s0) return fail(KV_INVALID_ARGUMENT, "var and %s are the same table", ww.slot);
    if (s0->dim != c.slot_mult * v->dim) return fail(KV_INVALID_ARGUMENT, ww.shape, v->dim, s0->dim);
    if (v->device != s0->device) return fail(KV_INVALID_ARGUMENT, "var and slot live on different devices");
    if (v == s0) return fail(KV_INVALID_ARGUMENT, "var and %s are the same table", ww.slot);
  } else if (!two) {
    if (s0->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "var and accum do not have the same shape [%d] [%d]", v->dim, s0->dim);
    if (v->device != s0->device || v == s0) return fail(KV_INVALID_ARGUMENT, "var and accum must be distinct tables on one device");
  } else {
    if (s0->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "kv_varaible and accum do not have the same shape [%d] [%d]", v->dim, s0->dim);
    if (s1->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "kv_variable and linear do not have the same shape [%d] [%d]", v->dim, s1->dim);
    if (v->device != s0->device || v->device != s1->device || v == s0 || v == s1 || s0 == s1)
      return fail(KV_INVALID_ARGUMENT, "var, accum and linear must be distinct tables on one device");
  }
  if (counted) {   // what only the batch pipeline serves needs a host count: refused before anything is queued
    if (!fused_ok(v->dim))
      return fail(KV_UNIMPLEMENTED, "kv_apply_unique_counted: embedding dim %d (multiples of 4 up to 256; other dims take the batch "
                                    "pipeline, which needs the count on the host: kv_apply_*_unique)", v->dim);
    DeviceGuard dgc(v->device);
    if (stream_is_capturing((hipStream_t)stream))
      return fail(KV_UNIMPLEMENTED, "kv_apply_unique_counted under stream capture: the duplicate guard's launch serial lives on "
                                    "the host (kv_apply_*_unique takes the batch pipeline there)");
  }
  if (n == 0) return KV_OK;
  DeviceGuard dg(v->device);
  MultiLock lk({v, s0, two ? s1 : s0});
  // GroupAdam / Adagrad: apply_common decides whether this apply works on the mirrors (mirror_decide); the FTRL family reads
  // and writes the slot tables' own records: its entry ends the tables' epochs
  auto keep = [&](const kv_table* t) -> unsigned { return two ? KEEP_NONE : (t == v ? KEEP_VAR : KEEP_NONE) | (t == s0 ? KEEP_SLOT : KEEP_NONE); };
  hipStream_t s = (hipStream_t)stream;
  if ((rc = lk.enter(s, keep, v->batch.holds(token, n) ? v : nullptr))) return rc;
  OptArgs a = c.a;
  a.l21_norm = a.l21 * std::sqrt((float)v->dim);   // training_ops.cc:728
  return with_opt(c.opt, [&](auto o) { return apply_common<decltype(o)::value>(v, s0, two ? s1 : nullptr, grad, ids, n, a, token, s, unique, self, counted); });
}

// Many tables.  After the parser's verdict the ops refuse a missing first table (and linears) — all but Adagrad, whose op
// leaves that to multi_common — and multi_apply_common checks the tables, their initialisation included.
int multi_apply(const OptCall& c, int num_tables, const kv_handle_t* vars, const kv_handle_t* slots0,
                const kv_handle_t* slots1, const float* const* grads, const void* const* ids, const int64_t* ns,
                const kv_batch_token_t* tokens, kv_stream_t stream, bool unique, bool require_reuse,
                const SelfSegment* selfs) {
  if (c.status) return c.status;
  const bool two = two_slots(c.opt);
  if (c.opt != OPT_ADAGRAD && (num_tables < 1 || !vars || !vars[0] || (two && !slots1)))
    return fail(KV_INVALID_ARGUMENT, "N must be >= 1");
  return with_opt(c.opt, [&](auto o) {
    return multi_apply_common<decltype(o)::value>(num_tables, vars, slots0, two ? slots1 : nullptr, c.slot_mult, grads, ids, ns,
                                                  c.a, stream, tokens, unique, require_reuse, selfs);
  });
}
}  // namespace kvhip_internal

extern "C" {

// ---- the entry points: plain / _tok / _unique, single table and batched ------------------------------------------------
// The _unique forms carry the caller's promise that `ids` holds no id twice — what the reference's ops receive in an
// unchanged TF graph (TF-core de-duplicates the IndexedSlices in front of them, variable_scope.py:1096-1106): kv_uapply.h
int kv_apply_group_adam(kv_handle_t v, kv_handle_t mvl, const float* grad, const void* ids, int64_t n, float lr, float b1p,
                        float b2p, float b1, float b2, float eps, float l1, float l2, float l21, int version, kv_stream_t stream) {
  return apply_one(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), v, mvl, nullptr, grad, ids, n, 0, stream, false);
}
int kv_apply_group_adam_tok(kv_handle_t v, kv_handle_t mvl, const float* grad, const void* ids, int64_t n, float lr, float b1p,
                            float b2p, float b1, float b2, float eps, float l1, float l2, float l21, int version,
                            kv_batch_token_t token, kv_stream_t stream) {
  return apply_one(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), v, mvl, nullptr, grad, ids, n, token, stream,
                   false);
}
int kv_apply_group_adam_unique(kv_handle_t v, kv_handle_t mvl, const float* grad, const void* ids, int64_t n, float lr,
                               float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21, int version,
                               kv_stream_t stream) {
  return apply_one(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), v, mvl, nullptr, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_group_adam(int num_tables, const kv_handle_t* vars, const kv_handle_t* slots, const float* const* grads,
                              const void* const* ids, const int64_t* ns, float lr, float b1p, float b2p, float b1, float b2,
                              float eps, float l1, float l2, float l21, int version, kv_stream_t stream) {
  return multi_apply(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), num_tables, vars, slots, nullptr, grads,
                     ids, ns, nullptr, stream, false);
}
int kv_multi_apply_group_adam_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* slots, const float* const* grads,
                                  const void* const* ids, const int64_t* ns, float lr, float b1p, float b2p, float b1, float b2,
                                  float eps, float l1, float l2, float l21, int version, const kv_batch_token_t* tokens,
                                  kv_stream_t stream) {
  return multi_apply(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), num_tables, vars, slots, nullptr, grads,
                     ids, ns, tokens, stream, false);
}
int kv_multi_apply_group_adam_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* slots,
                                     const float* const* grads, const void* const* ids, const int64_t* ns, float lr,
                                     float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21,
                                     int version, kv_stream_t stream) {
  return multi_apply(group_adam_call(version, lr, b1p, b2p, b1, b2, eps, l1, l2, l21), num_tables, vars, slots, nullptr, grads,
                     ids, ns, nullptr, stream, true);
}

int kv_apply_group_rectified_adam(kv_handle_t v, kv_handle_t opt, const float* grad, const void* ids, int64_t n, float lr,
                                  float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21, float r_t,
                                  int tractable, int amsgrad, int use_nesterov, kv_stream_t stream) {
  return apply_one(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), v, opt, nullptr,
                   grad, ids, n, 0, stream, false);
}
int kv_apply_group_rectified_adam_tok(kv_handle_t v, kv_handle_t opt, const float* grad, const void* ids, int64_t n, float lr,
                                      float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21,
                                      float r_t, int tractable, int amsgrad, int use_nesterov, kv_batch_token_t token,
                                      kv_stream_t stream) {
  return apply_one(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), v, opt, nullptr,
                   grad, ids, n, token, stream, false);
}
int kv_apply_group_rectified_adam_unique(kv_handle_t v, kv_handle_t opt, const float* grad, const void* ids, int64_t n, float lr,
                                         float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21,
                                         float r_t, int tractable, int amsgrad, int use_nesterov, kv_stream_t stream) {
  return apply_one(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), v, opt, nullptr,
                   grad, ids, n, 0, stream, true);
}
int kv_multi_apply_group_rectified_adam(int num_tables, const kv_handle_t* vars, const kv_handle_t* opts,
                                        const float* const* grads, const void* const* ids, const int64_t* ns, float lr, float b1p,
                                        float b2p, float b1, float b2, float eps, float l1, float l2, float l21, float r_t,
                                        int tractable, int amsgrad, int use_nesterov, kv_stream_t stream) {
  return multi_apply(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), num_tables,
                     vars, opts, nullptr, grads, ids, ns, nullptr, stream, false);
}
int kv_multi_apply_group_rectified_adam_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* opts,
                                            const float* const* grads, const void* const* ids, const int64_t* ns, float lr,
                                            float b1p, float b2p, float b1, float b2, float eps, float l1, float l2, float l21,
                                            float r_t, int tractable, int amsgrad, int use_nesterov,
                                            const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), num_tables,
                     vars, opts, nullptr, grads, ids, ns, tokens, stream, false);
}
int kv_multi_apply_group_rectified_adam_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* opts,
                                               const float* const* grads, const void* const* ids, const int64_t* ns, float lr,
                                               float b1p, float b2p, float b1, float b2, float eps, float l1, float l2,
                                               float l21, float r_t, int tractable, int amsgrad, int use_nesterov,
                                               kv_stream_t stream) {
  return multi_apply(group_radam_call(lr, b1p, b2p, b1, b2, eps, l1, l2, l21, r_t, tractable, amsgrad, use_nesterov), num_tables,
                     vars, opts, nullptr, grads, ids, ns, nullptr, stream, true);
}

int kv_apply_adam(kv_handle_t v, kv_handle_t mv, const float* grad, const void* ids, int64_t n, float lr, float b1p, float b2p,
                  float b1, float b2, float eps, kv_stream_t stream) {
  return apply_one(adam_call(lr, b1p, b2p, b1, b2, eps), v, mv, nullptr, grad, ids, n, 0, stream, false);
}
int kv_apply_adam_tok(kv_handle_t v, kv_handle_t mv, const float* grad, const void* ids, int64_t n, float lr, float b1p,
                      float b2p, float b1, float b2, float eps, kv_batch_token_t token, kv_stream_t stream) {
  return apply_one(adam_call(lr, b1p, b2p, b1, b2, eps), v, mv, nullptr, grad, ids, n, token, stream, false);
}
int kv_apply_adam_unique(kv_handle_t v, kv_handle_t mv, const float* grad, const void* ids, int64_t n, float lr, float b1p,
                         float b2p, float b1, float b2, float eps, kv_stream_t stream) {
  return apply_one(adam_call(lr, b1p, b2p, b1, b2, eps), v, mv, nullptr, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_adam(int num_tables, const kv_handle_t* vars, const kv_handle_t* mvs, const float* const* grads,
                        const void* const* ids, const int64_t* ns, float lr, float b1p, float b2p, float b1, float b2, float eps,
                        kv_stream_t stream) {
  return multi_apply(adam_call(lr, b1p, b2p, b1, b2, eps), num_tables, vars, mvs, nullptr, grads, ids, ns, nullptr, stream, false);
}
int kv_multi_apply_adam_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* mvs, const float* const* grads,
                            const void* const* ids, const int64_t* ns, float lr, float b1p, float b2p, float b1, float b2,
                            float eps, const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(adam_call(lr, b1p, b2p, b1, b2, eps), num_tables, vars, mvs, nullptr, grads, ids, ns, tokens, stream, false);
}
int kv_multi_apply_adam_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* mvs, const float* const* grads,
                               const void* const* ids, const int64_t* ns, float lr, float b1p, float b2p, float b1, float b2,
                               float eps, kv_stream_t stream) {
  return multi_apply(adam_call(lr, b1p, b2p, b1, b2, eps), num_tables, vars, mvs, nullptr, grads, ids, ns, nullptr, stream, true);
}

int kv_apply_adagrad(kv_handle_t v, kv_handle_t acc, float lr, const float* grad, const void* ids, int64_t n, int update_slots,
                     kv_stream_t stream) {
  return apply_one(adagrad_call(lr, update_slots), v, acc, nullptr, grad, ids, n, 0, stream, false);
}
int kv_apply_adagrad_tok(kv_handle_t v, kv_handle_t acc, float lr, const float* grad, const void* ids, int64_t n,
                         int update_slots, kv_batch_token_t token, kv_stream_t stream) {
  return apply_one(adagrad_call(lr, update_slots), v, acc, nullptr, grad, ids, n, token, stream, false);
}
int kv_apply_adagrad_unique(kv_handle_t v, kv_handle_t acc, float lr, const float* grad, const void* ids, int64_t n,
                            int update_slots, kv_stream_t stream) {
  return apply_one(adagrad_call(lr, update_slots), v, acc, nullptr, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_adagrad(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, float lr,
                           const float* const* grads, const void* const* ids, const int64_t* ns, int update_slots,
                           kv_stream_t stream) {
  return multi_apply(adagrad_call(lr, update_slots), num_tables, vars, accums, nullptr, grads, ids, ns, nullptr, stream, false);
}
int kv_multi_apply_adagrad_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, float lr,
                               const float* const* grads, const void* const* ids, const int64_t* ns, int update_slots,
                               const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(adagrad_call(lr, update_slots), num_tables, vars, accums, nullptr, grads, ids, ns, tokens, stream, false);
}
int kv_multi_apply_adagrad_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, float lr,
                                  const float* const* grads, const void* const* ids, const int64_t* ns, int update_slots,
                                  kv_stream_t stream) {
  return multi_apply(adagrad_call(lr, update_slots), num_tables, vars, accums, nullptr, grads, ids, ns, nullptr, stream, true);
}

int kv_apply_sparse_group_ftrl(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                               float lr, float l1, float l2, float l21, float l2s, float lr_power, kv_stream_t stream) {
  return apply_one(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, false);
}
int kv_apply_sparse_group_ftrl_tok(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids,
                                   int64_t n, float lr, float l1, float l2, float l21, float l2s, float lr_power,
                                   kv_batch_token_t token, kv_stream_t stream) {
  return apply_one(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), v, acc, lin, grad, ids, n, token, stream, false);
}
int kv_apply_sparse_group_ftrl_unique(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids,
                                      int64_t n, float lr, float l1, float l2, float l21, float l2s, float lr_power,
                                      kv_stream_t stream) {
  return apply_one(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_sparse_group_ftrl(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                     const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                     const int64_t* ns, float lr, float l1, float l2, float l21, float l2s, float lr_power,
                                     kv_stream_t stream) {
  return multi_apply(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     nullptr, stream, false);
}
int kv_multi_apply_sparse_group_ftrl_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                         const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                         const int64_t* ns, float lr, float l1, float l2, float l21, float l2s,
                                         float lr_power, const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     tokens, stream, false);
}
int kv_multi_apply_sparse_group_ftrl_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                            const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                            const int64_t* ns, float lr, float l1, float l2, float l21, float l2s,
                                            float lr_power, kv_stream_t stream) {
  return multi_apply(sparse_group_ftrl_call(lr, l1, l2, l21, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     nullptr, stream, true);
}

int kv_apply_ftrl_v2(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                     float lr, float l1, float l2, float l2s, float lr_power, kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, false);
}
int kv_apply_ftrl_v2_tok(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                         float lr, float l1, float l2, float l2s, float lr_power, kv_batch_token_t token, kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, token, stream, false);
}
int kv_apply_ftrl_v2_unique(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                            float lr, float l1, float l2, float l2s, float lr_power, kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_ftrl_v2(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, const kv_handle_t* linears,
                           const float* const* grads, const void* const* ids, const int64_t* ns, float lr, float l1, float l2,
                           float l2s, float lr_power, kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     nullptr, stream, false);
}
int kv_multi_apply_ftrl_v2_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, const kv_handle_t* linears,
                               const float* const* grads, const void* const* ids, const int64_t* ns, float lr, float l1,
                               float l2, float l2s, float lr_power, const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     tokens, stream, false);
}
int kv_multi_apply_ftrl_v2_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                  const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                  const int64_t* ns, float lr, float l1, float l2, float l2s, float lr_power, kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids, ns,
                     nullptr, stream, true);
}

int kv_apply_group_ftrl_v2(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                           float lr, float l1, float l2, float l2s, float lr_power, kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, false);
}
int kv_apply_group_ftrl_v2_tok(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids, int64_t n,
                               float lr, float l1, float l2, float l2s, float lr_power, kv_batch_token_t token,
                               kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, token, stream, false);
}
int kv_apply_group_ftrl_v2_unique(kv_handle_t v, kv_handle_t acc, kv_handle_t lin, const float* grad, const void* ids,
                                  int64_t n, float lr, float l1, float l2, float l2s, float lr_power, kv_stream_t stream) {
  return apply_one(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), v, acc, lin, grad, ids, n, 0, stream, true);
}
int kv_multi_apply_group_ftrl_v2(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums, const kv_handle_t* linears,
                                 const float* const* grads, const void* const* ids, const int64_t* ns, float lr, float l1,
                                 float l2, float l2s, float lr_power, kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids,
                     ns, nullptr, stream, false);
}
int kv_multi_apply_group_ftrl_v2_tok(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                     const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                     const int64_t* ns, float lr, float l1, float l2, float l2s, float lr_power,
                                     const kv_batch_token_t* tokens, kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids,
                     ns, tokens, stream, false);
}
int kv_multi_apply_group_ftrl_v2_unique(int num_tables, const kv_handle_t* vars, const kv_handle_t* accums,
                                        const kv_handle_t* linears, const float* const* grads, const void* const* ids,
                                        const int64_t* ns, float lr, float l1, float l2, float l2s, float lr_power,
                                        kv_stream_t stream) {
  return multi_apply(ftrl_v2_call(OPT_GROUP_FTRL_V2, lr, l1, l2, l2s, lr_power), num_tables, vars, accums, linears, grads, ids,
                     ns, nullptr, stream, true);
}

// the _unique op of optimizer code `optimizer` (shard_opt_call) with the id count on the device: kv_uapply.h k_uapply_counted
int kv_apply_unique_counted(kv_handle_t v, int optimizer, kv_handle_t slot0, kv_handle_t slot1, const float* hp, const float* grad,
                            const void* ids, int ids_dtype, int64_t n_max, const int64_t* n_dev, kv_stream_t stream) {
  if (!hp) return fail(KV_INVALID_ARGUMENT, "kv_apply_unique_counted: hp is null");
  if (ids_dtype != KV_DT_INT64 && ids_dtype != KV_DT_INT32)
    return fail(KV_INVALID_ARGUMENT, "kv_apply_unique_counted: ids_dtype %d (KV_DT_INT64 or KV_DT_INT32)", ids_dtype);
  if (!n_dev) return fail(KV_INVALID_ARGUMENT, "kv_apply_unique_counted: n_dev is null");
  const OptCall c = shard_opt_call(optimizer, hp);
  if (c.opt < 0) return fail(KV_INVALID_ARGUMENT, "kv_apply_unique_counted: optimizer %d", optimizer);
  DevCount dc;
  dc.n_dev = reinterpret_cast<const long long*>(n_dev);
  dc.ids32 = ids_dtype == KV_DT_INT32 ? 1 : 0;
  return apply_one(c, v, slot0, slot1, grad, ids, n_max, 0, stream, true, nullptr, &dc);
}

int kv_attach_slot(kv_handle_t v, kv_handle_t sl, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(v)) || (rc = check_table(sl))) return rc;
  if (v == sl || v->device != sl->device || v->key_dtype != sl->key_dtype)
    return fail(KV_INVALID_ARGUMENT, "kv_attach_slot: var and slot must be distinct tables on one device with one key dtype");
  DeviceGuard dg(v->device);
  MultiLock lk({v, sl});
  hipStream_t s = (hipStream_t)stream;
  if ((rc = lk.enter(s))) return rc;
  unsigned nrows = 1;
  if ((rc = stats(v, s, nullptr, &nrows))) return rc;
  if (v->slot_uid != 0 && (v->slot_uid != sl->uid || v->slot_gen != sl->gen))
    launch_clear_hints(v, s);
  v->slot_uid = sl->uid;
  v->slot_gen = sl->gen;
  v->batch.drop();
  // (the entry above ended any running epoch of either table; a pair of single-chunk tables gets its mirrors filled here)
  launch_link_hints(v, sl, nrows, s);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

}  // extern "C"
