// kv_host.h — the table core's internal interface: what the three units on top of kvhip.hip — kv_ops.hip (the table ops),
// kv_apply.hip (the optimizer layer) and kv_shard.hip (the sharded layer) — use of a table: its types and the functions
// below, nothing else.  Everything sits in the hidden namespace of kv_types.h, so none of it is exported; `struct kv_table`
// is the ABI's opaque handle and therefore global.  The functions are defined, and explained, in kvhip.hip unless a section
// names another unit.
//
// The boundary: no unit other than kvhip.hip names a pair_*, mirror_*, pend_wd or pend_pa member of kv_table, or a MirrorPair
// — the slot mirrors and the pending partition pass are reached through mirror_decide, set_pending_part, take_pending_part,
// flush_part and launch_link_hints — and only kvhip.hip compiles the pipelines' kernels (kv_kernels.h, kv_fused.h, kv_papply.h), which the
// other units reach through the launch_* functions.  The descriptors of a batched launch go to the device through
// Staged<Desc> alone (the staging ring: acquire, fill, upload, busy until the stream has read them).
//
// What the entry points share: TableOp (device, lock and stream of a single-table op), require_initialized (the one
// precondition message), with_id_type (a kernel's id-type template argument from a run-time value; the row-width ones come
// from kv_row_geom.h, the one statement of the row geometry: with_lanes, with_row_geom), self_part_args (the PartArgs of an
// op on a table's own rows) and ensure_pos_ent (Workspace::pos_ent).
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/kvhip.h"
#include "kv_batch_index.h"
#include "kv_launch.h"
#include "kv_mirror_epoch.h"

namespace __attribute__((visibility("hidden"))) kvhip_internal {

int fail(int code, const char* fmt, ...);   // records the calling thread's message (kv_last_error), returns `code`

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(_e == hipErrorOutOfMemory ? KV_RESOURCE_EXHAUSTED : KV_INTERNAL,            \
                  "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

struct Workspace {
  long long cap_n = 0;       // ids (multiple of TILE)
  unsigned capP = 0;         // partitions toff was sized for
  long long* ent_key = nullptr;
  unsigned* ent_a = nullptr;
  unsigned* ent_b = nullptr;
  unsigned* ent_base = nullptr;
  unsigned* ent_rec = nullptr;
  unsigned* toff = nullptr;
  unsigned* slot_rank = nullptr;
  unsigned* order = nullptr;
  uint4* coldlist = nullptr;   // [cap_n][2]
  uint4* hotlist = nullptr;    // [cap_n][2]
  uint4* litem = nullptr;      // [cap_n]
  uint4* items = nullptr;      // [cap_n]
  uint4* pmeta = nullptr;      // [capP]
  float* hpart = nullptr;      // [chunk_cap(cap_n)][dim]
  long long hpart_elems = 0;
  unsigned* ctr = nullptr;
  unsigned* mcount = nullptr;  // entry-list pipeline: [cap_n / TILE]
  unsigned short* pos_ent = nullptr;   // [pos_cap] sharded route: every position's entry number in its tile
  long long pos_cap = 0;
  float* epart = nullptr;      // [cap_n / 2][dim] tile sums
  long long epart_elems = 0;
  long long* scat_keys = nullptr;  // kv_scatter_update on repeated ids: de-duplicated ids and combined updates
  float* scat_sum = nullptr;
  long long scat_cap = 0;          // rows
  unsigned* seg_off = nullptr;   // kv_lookup_sparse and its backward: CSR offsets [seg_cap + 1]
  long long seg_cap = 0;
  float* seg_den = nullptr;      // kv_lookup_sparse_grad: the segments' denominators [den_cap]
  long long den_cap = 0;
  int* pseg = nullptr;           // sharded sparse apply (a route table): every position's clamped segment [prec_cap]
  float* pscale = nullptr;       // ... and its scale [prec_cap]
  long long prec_cap = 0;
  unsigned long long* dbg = nullptr;
};

// The slot mirrors of one (var, slot) pair (kv_device.h SlotMirror; kvhip.hip "slot mirrors: the host side"): ONE record that
// the two tables share, each through a reference of its own (kv_table::pair_var / pair_slot), either of which may go first.
// Everything in it is read and written under `mu` alone — the innermost lock: taken with one or both table locks held, never
// the other way round.
struct MirrorPair {
  std::mutex mu;
  MirrorEpoch epoch;
  // the pair's device views as the last lean apply (or the pairing) saw them.  What a dirty copy names — a var row and a
  // slot row of the chunk-0 slabs — is inside these views whatever happened to the tables since: an epoch end launches
  // through them and never reads the other table's host state (whose owner may be growing it on another thread)
  TableDev view_var{}, view_slot{};
  bool dissolved = false;        // a table has left: no epoch, no copies any more; the other one drops its reference when it next looks
  hipEvent_t flushed = nullptr;  // recorded behind the last write-back, on the stream that ran it
  ~MirrorPair() { if (flushed) hipEventDestroy(flushed); }
};

}  // namespace kvhip_internal

using namespace kvhip_internal;   // (as every unit says: the handle's members name the internal types)

struct kv_table {
  // every op that may change which rows exist (or what the delta lists hold) advances op_serial; the two-phase
  // calls (count, then fill into buffers the caller sized from the counts) refuse to fill once it has moved on
  uint64_t op_serial = 1, export_serial = 0, delta_serial = 0, expire_serial = 0;
  int device = 0;
  int key_dtype = KV_DT_INT64;
  int dim = 0;
  unsigned enter_threshold = 0;
  unsigned long long seed = 0;
  int fixed_day = -1;
  // index
  Entry* entries = nullptr;
  unsigned long long cap = 0;
  // slab
  int chunk_bits = 16;
  std::vector<Chunk> chunks;
  Chunk* d_chunks = nullptr;
  unsigned* d_counters = nullptr;  // [0] next_row [1] error [2] rows on the free list
  unsigned* free_rows = nullptr;   // rows released by Delete (device stack, rows_cap entries)
  unsigned long long free_cap = 0;
  long long free_known = 0;        // free-list length at the last sync (> 0: inserts pop from it)
  unsigned long long idx_ub = 0;   // upper bound of claimed index entries (live keys + tombstones)
  // exact claimed entries at a sync = idx_base + (next_row - bump_base) + free-list pops since the
  // last index rebuild, pops = pushes_since - (free_now - free_base)   (revivals make it an upper bound)
  unsigned long long idx_base = 0, bump_base = 1, pushes_since = 0;
  long long free_base = 0;
  unsigned long long rows_cap = 0;  // chunks.size() << chunk_bits
  unsigned long long rows_ub = 1;   // upper bound of next_row
  // stream capture (kvhip.hip ensure_capacity): kv_prepare_capture was called; a call on the table was recorded into a
  // capture since — replays move the device's counters without the host, so rows_ub / idx_ub are refreshed by every call
  // outside a capture from then on
  bool capture_prepared = false, captured_calls = false;
  // init table
  float* init_table = nullptr;
  long long init_rows = 0;
  bool initialized = false;
  bool init_placeholder = false;   // init_table is the zero row an import put there, not a real init table
  Workspace ws;
  // the index of the table's last batch, as far as the workspace still holds it, and whether that lookup's partition pass
  // is still pending: one record, written only through its transitions (kv_batch_index.h states the invariants)
  BatchIndex batch;
  long long batch_n_prev = 0;      // ids of the previous entry-list index pass (choose_partitions: the distinct-count hint belongs to that size)
  // A training lookup that hands out a batch token returns when its rows are written; its partition pass (frequency
  // words, rows of new keys, the batch's key records and entry list) is PENDING (batch.part_pending()): the optimizer apply
  // of that batch runs it in front of its own kernels, any other op on the table runs it first thing (settle).  Same stream
  // order as before, the rows just do not wait for it.  The pass's arguments, as byte images (their types are the device's):
  unsigned char pend_wd[sizeof(WsDev)], pend_pa[sizeof(PartArgs)];
  // Slot mirrors: the table's references to the pair records it is half of — as a var (its rows hold the copies) and as a slot
  // table (another table's rows hold copies of its records); a table can be both.  Read and written under the table's own
  // `mu`, never by the partner.  The rest are the table's own facts, under `mu` like everything else.
  std::shared_ptr<MirrorPair> pair_var, pair_slot;
  unsigned mirror_next = 1u;       // var side: the first epoch of its next pair — where the last pair it left stopped
  long long stat_mirror_applies = 0, stat_mirror_epochs = 0;   // kv_get_stat (epochs: ended in the pairs it has left as their var)
  bool mirror_banned = false;      // either side: the table is used under stream capture (kv_prepare_capture): no mirrors, ever
  bool mirror_shared = false;      // slot side: a second var attached it — no mirrors for this table any more
  unsigned uniq_serial = 0;        // stamp of the table's last kv_apply_*_unique launch (kv_uapply.h; wraps at 65535: stamps cleared)
  bool deterministic = false;      // kv_set_deterministic
  bool occurrence_order = false;   // kv_set_deterministic(h, 2): a repeated id's gradient rows are added one by one in input order
                                   // (the sorted-position pipeline with one chain per key; implies deterministic)
  std::atomic<int> shard_refs{0};  // kv_shard handles built on this table
  bool fast_math = false;          // kv_set_fast_math: the optimizers' sqrt / division on v_sqrt_f32 / v_rcp_f32 (1 ulp) —
                                   // never in deterministic mode, which keeps the IEEE sequences
  uint64_t uid = 0;                // unique over the process: names the attached slot table safely
  uint64_t slot_uid = 0;           // uid of the slot table the index entries' hints refer to (0 = none)
  uint64_t slot_gen = 0;           // that table's `gen` when the hints were valid
  uint64_t gen = 0;                // bumped when the table is cleared (import): hints into it die
  unsigned* err_host = nullptr;    // pinned: the device error flag, copied back after every batch op
  unsigned* cnt_host = nullptr;    // pinned: where the synchronous ops (kv_dedup_segment_sum, kv_unique) read their count back
  hipStream_t last_stream = nullptr;  // stream of the table's last op; a different stream first waits for it
  bool has_last = false;
  hipEvent_t last_done = nullptr;
  // delta lists (SUPPORT_DELTA_EXPORT / SUPPORT_PREDICTION_DELTA_EXPORT, kv_variable.h:100-111): live keys
  // carry a byte in their RowMeta; keys recorded by Delete have no row and wait here
  bool track_delta = false, track_pred = false;
  std::vector<long long> del_train, del_pred;
  unsigned long long* d_stat = nullptr;  // [4]
  std::mutex mu;
  unsigned* route_hist = nullptr;  // kv_bucket_by_owner scratch
  size_t route_hist_cap = 0;
  // optional per-kernel timing (kv_profile_*): event pairs recorded on the op's stream
  bool prof = false;
  unsigned prof_mask = 0xFFFFFFFFu;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_kind;
  size_t ev_used = 0;
  int prof_every = 1;                // bracket every prof_every-th launch of a kind (kv_profile_sample)
  unsigned prof_seq[KV_PROF_KINDS] = {};
};

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// ---- small helpers -----------------------------------------------------------------------------------------------------
inline unsigned long long pow2ceil(unsigned long long x) {
  unsigned long long p = 1;
  while (p < x) p <<= 1;
  return p;
}

inline int ilog2(unsigned long long x) {
  int l = 0;
  while ((1ull << l) < x) ++l;
  return l;
}

inline int nblocks(long long work, int per_block, int cap = 4096) {
  long long b = (work + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int d) { hipGetDevice(&prev); if (prev != d) hipSetDevice(d); cur = d; }
  ~DeviceGuard() { if (prev != cur) hipSetDevice(prev); }
  int cur;
};

inline int check_table(kv_handle_t h) {
  if (!h) return fail(KV_INVALID_ARGUMENT, "null table handle");
  return KV_OK;
}

// CheckInitializedInternal (kv_variable.h:242).  what: the words behind the colon (the optimizer ops name the table;
// nullptr: none).  Each op calls it where the reference checks, between its own argument checks.
inline int require_initialized(const kv_table* t, const char* what = "KvVariable init table not set") {
  if (t->initialized) return KV_OK;
  return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables%s%s", what ? ": " : "", what ? what : "");
}

// A single-table op from here to scope exit: the table's device current, its mutex held, s the op's stream.  Entering the
// table stays the op's own call, because the ops differ in it: enter_op with its KEEP_* roles, hand_over, join_side, none.
struct TableOp {
  DeviceGuard dg;
  std::lock_guard<std::mutex> lock;
  hipStream_t s;
  TableOp(kv_table* t, kv_stream_t stream) : dg(t->device), lock(t->mu), s((hipStream_t)stream) {}
};

// f(IdT{}) with the id type of a kernel: int or long long
template <class F>
auto with_id_type(bool int32_ids, F&& f) {
  if (int32_ids) return f(int{});
  return f((long long)0);
}

// ---- the entry-list pipeline (kv_fused.h) ----
// ids per index pass: positions and epart rows are 30-bit fields of the entry list's words, a partition block takes
// up to 65535 entries; 2^23 ids (4096 tiles) stay well inside both
constexpr long long FUSED_MAX_N = 1ll << 23;   // (the dims it serves: fused_ok, kv_row_geom.h)

// (re)allocation that leaves the old buffer in place when the new one cannot be had
template <typename T>
int regrow(T** p, size_t count) {
  T* q = nullptr;
  HIP_TRY(hipMalloc(&q, count * sizeof(T)));
  if (*p) hipFree(*p);
  *p = q;
  return KV_OK;
}

bool stream_is_capturing(hipStream_t s);
int ws_sync(hipStream_t s);
int ensure_capacity(kv_table* t, long long extra, hipStream_t s);
int ensure_free_list(kv_table* t, hipStream_t s);   // the free-list stack holds every row of the slab (before a kernel that releases rows)
int ensure_workspace(kv_table* t, long long n, bool need_part, hipStream_t s);
int ensure_pos_ent(kv_table* t, long long n, hipStream_t s);
int ensure_pos_records(kv_table* t, long long n, hipStream_t s);   // Workspace::pseg / pscale hold n positions
// kv_ops.hip: Workspace::seg_off holds num_segments + 1 offsets and, need_den, Workspace::seg_den num_segments denominators
int ensure_seg(kv_table* t, long long num_segments, bool need_den, hipStream_t s);
// kv_ops.hip: the position records of the sharded sparse apply (kv_types.h SegDesc; kv_lookup_sparse_grad's offsets,
// denominators and scales, per position instead of per values row).  m tables; m > 1: `dev` is the staged copy of `host`.
// At most 3 launches whatever m is.
int launch_pos_records(int m, const SegDesc* host, const SegDesc* dev, int seg32, int combiner, hipStream_t s);
unsigned fused_default_P(long long n);
size_t chunk_cap(long long n);

// ---- what a table's settings mean to an op -----------------------------------------------------------------------------
bool fast_math_on(const kv_table* t);
int det_mode(const kv_table* t);
unsigned today(const kv_table* t);
bool fused_tab(const kv_table* t);
bool dim_supported(int D);

// ---- views -------------------------------------------------------------------------------------------------------------
TableDev dev_view(const kv_table* t);

// The sharded owner ops read a rank's OWN exchange segment where it was written: records [lo, lo + len) of the buffers the
// op reads come from `ids` / `grad` (the send buffers) instead.  Passed by kv_shard_lookup_serve / kv_shard_apply_serve and
// the grouped serve blocks of kv_multi_shard_lookup / kv_multi_shard_apply (shard_self; one per table in the batched ones)
// down to the ws_view of the lookup or apply that serves them; every other op passes none.  The default is "no segment".
struct SelfSegment { unsigned lo = 0, len = 0; const void* ids = nullptr; const float* grad = nullptr; };

WsDev ws_view(kv_table* t, long long n, const SelfSegment* self = nullptr);

// the PartArgs of an op of n ids on a table's own rows: its slot tables are the table itself
inline PartArgs self_part_args(const kv_table* t, long long n) {
  PartArgs pa{};
  pa.tv = dev_view(t); pa.ts0 = pa.tv; pa.ts1 = pa.tv;
  pa.det = det_mode(t);
  pa.n = n;
  return pa;
}

// brackets one kernel launch with a pair of events when profiling is on
struct ProfScope {
  kv_table* t;
  hipStream_t s;
  bool on;
  ProfScope(kv_table* t_, int kind, hipStream_t s_) : t(t_), s(s_), on(false) {
    if (t->prof && ((t->prof_mask >> kind) & 1u) && t->ev_used + 2 <= t->ev.size() &&
        (t->prof_every <= 1 || (t->prof_seq[kind]++ % (unsigned)t->prof_every) == 0u)) {
      on = true;
      t->ev_kind[t->ev_used / 2] = kind;
      hipEventRecord(t->ev[t->ev_used], s);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(t->ev[t->ev_used + 1], s);
      t->ev_used += 2;
    }
  }
};

// ---- kernel launchers (the pipelines' kernels are compiled into kvhip.hip alone) -----------------------------------------
// the templated ones are instantiated in kvhip.hip for the arguments named here
template <bool FIRST>   // false, true
void launch_tile(kv_table* t, const WsDev& wd, const void* ids, const int* counts, long long n, hipStream_t s,
                 int ids_kind = -1, const MultiDesc* md = nullptr, int ntab = 0, unsigned gx = 0);
template <int MODE>     // MODE_LOOKUP, MODE_APPLYIDX, MODE_UNIQUE, MODE_SCATTER, MODE_MARK
void launch_part_keys(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0);
void launch_gather(const TableDev& td, const WsDev& wd, float* op, long long m, hipStream_t s,
                   const MultiDesc* md = nullptr, int ntab = 0, bool order = false);
void launch_order(const TableDev& td, const WsDev& wd, long long n, hipStream_t s,
                  const MultiDesc* md = nullptr, int ntab = 0);
void launch_ltile(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, const int* counts, long long n, float* out,
                  hipStream_t s, int ids_kind = -1, const MultiDesc* md = nullptr, int ntab = 0, bool multi_rows = false);
void launch_part2(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0);
int launch_occ_sum(const WsDev& wd, const PartArgs& pa, int fop, long long nmax, hipStream_t s);
void launch_fill_entries(kv_table* t, hipStream_t s);
void launch_clear_hints(kv_table* v, hipStream_t s);
void launch_clear_stamps(kv_table* v, hipStream_t s);
void launch_link_hints(kv_table* v, kv_table* sl, unsigned nrows, hipStream_t s);
void launch_ltile_notable(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, long long n, hipStream_t s,
                          const int* counts = nullptr, bool int32_ids = false);
void launch_ltile_multi_notable(const WsDev& wmax, int ntab, const MultiDesc* md, hipStream_t s);

// ---- entering a table --------------------------------------------------------------------------------------------------
// the mirror role(s) an op keeps a table in where it enters it (kvhip.hip: slot mirrors, the host side)
enum : unsigned {
  KEEP_NONE = 0u,
  KEEP_VAR = 1u,    // the table's own epoch (it is a pair's var) goes on
  KEEP_SLOT = 2u,   // the epoch of the var this table is the slot table of goes on
};

int hand_over(kv_table* t, hipStream_t s, unsigned keep = KEEP_NONE, bool settle = true, bool mutates = true);
int enter_op(kv_table* t, hipStream_t s, unsigned keep = KEEP_NONE, bool settle = true, bool mutates = true);
int join_side(kv_table* t, hipStream_t s);
int settle_pending(kv_table* t);
int stats(kv_handle_t t, hipStream_t s, unsigned long long out[2], unsigned* nrows_out);

// ---- the pending partition pass and the slot mirrors, as the ops see them ------------------------------------------------
// a training lookup leaves its partition pass (wd, pa) pending on the table (BatchIndex::defer_part)
void set_pending_part(kv_table* t, const WsDev& wd, const PartArgs& pa);
// the optimizer apply of that batch takes it over: no longer pending; the lookup's own day stamp and counting rule come out
void take_pending_part(kv_table* t, PartArgs* lookup);
int flush_part(kv_table* t, hipStream_t s);
// lean: the launch is k_papply / k_uapply AND the optimizer has one slot table (!two_slots(OPT))
int mirror_decide(kv_table* v, kv_table* s0, PartArgs& pa, bool lean, hipStream_t s);

// locks tables in address order like MaybeLockVariableInputMutexesInOrder (training_ops.cc:96-184)
struct MultiLock {
  std::vector<kv_table*> ts;
  kv_table* one = nullptr;   // the single-table form: one mutex, nothing allocated (ts stays empty)
  explicit MultiLock(kv_table* t) : one(t) { t->mu.lock(); }
  explicit MultiLock(std::initializer_list<kv_table*> l) : MultiLock(std::vector<kv_table*>(l)) {}
  explicit MultiLock(std::vector<kv_table*> l) : ts(std::move(l)) {
    std::sort(ts.begin(), ts.end());
    ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
    for (auto* t : ts) t->mu.lock();
  }
  ~MultiLock() {
    for (auto it = ts.rbegin(); it != ts.rend(); ++it) (*it)->mu.unlock();
    if (one) one->mu.unlock();
  }
  // keep(t): the mirror role(s) table t is kept in (KEEP_*)
  // later: this table's pending partition pass is taken over by the caller (the optimizer apply of that batch)
  template <class Keep>
  int enter(hipStream_t s, Keep keep, kv_table* later = nullptr) {
    int rc;
    for (auto* t : ts)
      if ((rc = enter_op(t, s, keep(t), t != later))) return rc;
    return one ? enter_op(one, s, keep(one), one != later) : KV_OK;
  }
  int enter(hipStream_t s) { return enter(s, [](const kv_table*) { return (unsigned)KEEP_NONE; }); }
};

void retire_stream(hipStream_t dead);

// ---- index passes ------------------------------------------------------------------------------------------------------
extern std::atomic<uint64_t> g_serial;   // batch tokens
void choose_partitions(kv_table* t, WsDev& wd, long long n);   // wd.P, wd.pshift: whoever publishes the index hands P on
template <int MODE>   // MODE_LOOKUP, MODE_APPLYIDX, MODE_UNIQUE
void index_pass(kv_table* t, const WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                int ids_kind, float* out, hipStream_t s, bool file_order = true);
int fused_lookup_pass(kv_table* t, WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                      int ids_kind, float* out, hipStream_t s, bool defer_part);
// segmented fold over the sorted positions + fused update (k_apply_sorted), then the keys that cross chunk
// boundaries (k_apply_span).  pa.n = ids of the batch (multi: nmax = the largest table's batch).  A host template that
// launches through kv_launch.h and launch_occ_sum: kv_apply.hip uses it per OPT, kv_ops.hip for MODE_DEDUP.
template <int MODE, int OPT>
int launch_apply(kv_table* prof_t, const WsDev& wd, const PartArgs& pa, long long nmax, hipStream_t s,
                 const MultiDesc* md = nullptr, int ntab = 0, bool skip_fin = false) {
  const int D = pa.tv.dim;
  // waves stride over the items (hot chunks, then cold batches of 64 / LPR keys); 8 blocks of 4 waves per CU
  // is everything the chip holds at once, fewer for small batches
  constexpr int gmax = 2048;
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(gmax, (nmax / 2 + chunk_cap(nmax)) / 4 + 1));
  const unsigned gfin = (unsigned)std::max<long long>(1, std::min<long long>(256, nmax / 4096 + 1));   // each block reads its share of the items at once
  auto launch = [&](unsigned nchunks, int span) {
    if constexpr (MODE == MODE_DEDUP) return launch_dedup_fold(wd, pa, s, md, ntab, nchunks, span);
    else return launch_sorted_apply<OPT>(wd, pa, s, md, ntab, nchunks, span);
  };
  int rc;
  if (pa.det == 2 && !md) {
    // occurrence order: the hot keys' chains first (k_occ_sum: one block per key, the sums to hpart), k_apply reads them
    const int fop = MODE == MODE_APPLY ? KV_SCATTER_ADD : pa.fold_op;
    if ((rc = launch_occ_sum(wd, pa, fop, nmax, s))) return rc;
  }
  {
    ProfScope ps(prof_t, KV_PROF_APPLY_SORTED, s);
    rc = launch(grid, 0);
  }
  if (rc == KV_OK && !skip_fin) {
    ProfScope ps(prof_t, KV_PROF_APPLY_SPAN, s);
    rc = launch(gfin, 1);
  }
  if (rc == KV_UNIMPLEMENTED)
    return md ? fail(KV_UNIMPLEMENTED, "batched launch: embedding dim %d (multiples of 4 only)", D)
              : fail(KV_UNIMPLEMENTED, "embedding dim %d not supported by the fused kernels "
                     "(multiples of 4 up to 1024, any dim up to 256)", D);
  if (rc)   // (today the one such step is k_apply_fin's request for its LDS, dims 576 and up: launch_apply_t)
    return fail(rc, "sorted-position apply at embedding dim %d: setting up a kernel launch failed (code %d)", D, rc);
  return KV_OK;
}

// ---- descriptor staging for the batched launches -----------------------------------------------------------------------
struct StageSlot {
  char* host = nullptr;   // pinned
  char* dev = nullptr;
  size_t cap = 0;
  hipEvent_t consumed = nullptr;
  // where `consumed` was recorded, and whether the stream may not have got there yet (retire_stream clears it for a stream
  // that was drained and is about to go away: an event is not waited on once its stream is gone)
  hipStream_t last = nullptr;
  bool busy = false;
};
struct BatchStage {       // a small ring, so the host can prepare call k+1 while call k still runs
  std::mutex mu;
  StageSlot slot[4];
  unsigned cursor = 0;
};
extern BatchStage g_stage[64][3];   // [device][0 = inference gather, 1 = training ops, 2 = the sparse lookups' own descriptors]
int stage_take(BatchStage& st, size_t bytes, StageSlot** out);   // the ring's next slot; st.mu is HELD where it succeeds
// Under a stream capture the upload is RECORDED: every replay copies whatever the host buffer holds then into a device
// buffer that later calls write too, and a ring slot is handed out again four calls on — a replayed batched op would run on
// another call's descriptors.  A captured batched call therefore takes the host and device bytes of its descriptors from an
// arena whose bytes are handed out once and never again (graphs may be replayed for as long as the process lives).  The arena
// grows outside captures only: kv_prepare_capture tops it up to CAPTURE_STAGE_ROOM free bytes (capture_stage_reserve);
// capture_stage_take refuses with KV_FAILED_PRECONDITION where it has no room.
constexpr size_t CAPTURE_STAGE_ROOM = 256 * 1024;
int capture_stage_reserve(int device);
int capture_stage_take(int device, size_t bytes, char** host, char** dev);
// `count` descriptors of a batched launch on g_stage[device][ring]: zeroed host descriptors by index, then ONE upload,
// which is the only way to the device pointer — so a slot a kernel may still read is always marked busy.  The ring stays
// locked until scope exit.  Check rc before anything else.
template <class Desc>   // MultiDesc, FinishDesc, BatchGatherDesc, SparseDesc, SegDesc
class Staged {
  BatchStage& st;
  StageSlot* sl = nullptr;
  const size_t bytes;
  hipStream_t s = nullptr;
  bool launched = false;
  const int device;
 public:
  int rc;
  Staged(int device, int ring, int count) : st(g_stage[device][ring]), bytes((size_t)count * sizeof(Desc)), device(device) {
    if (!(rc = stage_take(st, bytes, &sl))) std::memset(sl->host, 0, bytes);
  }
  Staged(const Staged&) = delete;
  ~Staged() {   // the slot is busy until the stream gets there
    if (launched) { hipEventRecord(sl->consumed, s); sl->last = s; sl->busy = true; }
    if (sl) st.mu.unlock();
  }
  Desc& operator[](int i) { return reinterpret_cast<Desc*>(sl->host)[i]; }
  int upload(hipStream_t stream, const Desc** dev) {
    if (stream_is_capturing(stream)) {   // bytes of its own, for every replay (the ring slot never reaches the stream: not busy)
      char *h, *d;
      const int rc_take = capture_stage_take(device, bytes, &h, &d);
      if (rc_take) return rc_take;
      std::memcpy(h, sl->host, bytes);
      HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream));
      *dev = reinterpret_cast<const Desc*>(d);
      return KV_OK;
    }
    HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, bytes, hipMemcpyHostToDevice, stream));
    launched = true; s = stream;
    *dev = reinterpret_cast<const Desc*>(sl->dev);
    return KV_OK;
  }
};
// a batched launch's grid covers its largest table
inline void widen(WsDev& wmax, const WsDev& w) { wmax.ntiles = std::max(wmax.ntiles, w.ntiles); wmax.P = std::max(wmax.P, w.P); }
inline void use_partitions(WsDev& w, unsigned P) { w.P = P; w.pshift = 64 - ilog2(P); }
int check_same_shape(int num_tables, const kv_handle_t* tables, const char* what);

// ---- kv_ops.hip: the argument checks the batched lookups and the batched optimizer ops share ---------------------------
int multi_common(int num_tables, const kv_handle_t* tables, const void* const* ids, const int64_t* ns);

// ---- the ops the owner side of a sharded op runs (kv_ops.hip the lookups, kv_apply.hip the optimizer ops) --------------
int gather_or_insert_impl(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, float* out,
                          kv_stream_t stream, int pairs, kv_batch_token_t* token, unsigned seg_cap = 0,
                          const SelfSegment* self = nullptr);
int multi_lookup_impl(int num_tables, const kv_handle_t* tables, const void* const* ids,
                      const int32_t* const* counts, const int64_t* ns, float* const* outs,
                      kv_batch_token_t* tokens, kv_stream_t stream, int ids_kind, const unsigned* seg_caps,
                      const SelfSegment* selfs);

// An optimizer op as the pipelines see it: which kernels (opt, an OPT_*), with which arguments, on slot tables of which
// shape.  One parser per optimizer family fills it from the op's arguments; every entry point below is a parser and one of
// two bodies: apply_one (one table) or multi_apply (many tables, one launch per stage).
struct OptCall {
  int opt = -1;          // OPT_*; -1: not known (a GroupAdam version other than 3 or 4, a sharded optimizer code)
  OptArgs a{};           // without l21_norm, which the bodies derive from the var's dim
  int slot_mult = 1;     // first slot table's dim / var dim; a second slot table (linear) iff two_slots(opt)
  int status = KV_OK;    // the parser's verdict on the op's arguments; its message is the one fail() recorded last
};

OptCall shard_opt_call(int optimizer, const float* hp);
// kv_apply_unique_counted: the unique apply whose id count is a device word (n of apply_one is then the most ids the call
// may hold) and whose ids have a dtype of their own
struct DevCount { const long long* n_dev = nullptr; int ids32 = 0; };
int apply_one(const OptCall& c, kv_table* v, kv_table* s0, kv_table* s1, const float* grad, const void* ids, int64_t n,
              kv_batch_token_t token, kv_stream_t stream, bool unique, const SelfSegment* self = nullptr,
              const DevCount* counted = nullptr);
int multi_apply(const OptCall& c, int num_tables, const kv_handle_t* vars, const kv_handle_t* slots0,
                const kv_handle_t* slots1, const float* const* grads, const void* const* ids, const int64_t* ns,
                const kv_batch_token_t* tokens, kv_stream_t stream, bool unique, bool require_reuse = false,
                const SelfSegment* selfs = nullptr);

}  // namespace kvhip_internal
