// kvhip.hip — MI355X (gfx950) KvVariable, the table core: HBM hash table + row slab, growth, the per-batch workspace,
// slot mirrors, stream hand-over, the pipelines' kernels with their launchers and index passes, and the lifecycle /
// settings part of the C ABI of include/kvhip.h.  The only unit that compiles the pipelines' kernels.  The units on top
// reach it through kv_host.h: kv_ops.hip (the table ops), kv_apply.hip (the optimizer ops), kv_shard.hip (sharded tables).
//
// Layout in HBM (per table):
//   index    Entry[cap+1]   16 B {int64 key, u32 row, u32 slot-row hint}, open addressing, linear
//                           probing, cap = 2^k >= 2 * rows (load <= 0.5).  Entry[cap] is the
//                           home of the one key that equals the EMPTY sentinel.
//   chunks   row slab in chunks of 2^cb rows: rows[r][dim] fp32 and one 32-byte record unit per row: RowMeta 16 B
//            {int64 key, u32 freq = (day << 16) | saturating u16 frequency, u8 flags (bit0 blacklist, bit1
//            under_threshold, bit2 under_threshold stale, bit3 released by Delete), u8 delta-list bits,
//            u16 stamp (serial of the last unique-ids apply that updated the row)} + SlotMirror 16 B (var tables of
//            a (var, slot) pair: a write-back copy of the slot row's frequency word and flags; mirror_* below).  Row ids are
//            dense (bump allocated; rows released by Delete are recycled from a device free
//            list), row 0 is a permanent all-zero row (misses / nothing).
//   workspace per-batch index (ent_key / ent_a / ent_b / ent_base / ent_rec, toff, mrow, epart, order; the
//            sorted-position kernels' lists in the same buffers): plain stores only, rewritten by every
//            op — nothing to clean.
//
// Kernel pipelines (DESIGN.md section 3 has the byte accounting):
//   entry-list kernels (kv_fused.h, kv_papply.h, kv_uapply.h; dims that are multiples of 4 up to 256):
//     lookup : k_ltile            tile pass (LDS dedup, winner probes / inserts, entries by hash partition) + output rows
//              k_part2            the lookup's bookkeeping alone (deferred when a batch token is handed out)
//     apply  : k_tsum + k_papply  tile sums, then partition pass + bookkeeping + fused update in one launch
//              k_ltsum + k_papply the same for ids the table has not indexed (no token)
//              k_uapply           ids promised unique + pre-summed rows: one launch
//   sorted-position kernels (kv_kernels.h; every other dim, kv_unique / dedup / scatter / marks / sparse lookup):
//     k_tile, k_part_keys<MODE>, k_gather<ORDER> / k_order, k_apply<OPT>, k_apply_fin<OPT>
//   the ops' own small kernels (kv_op_kernels.h, kv_ops.hip): point queries, delete, export, inference gathers, combiners
//   sharded (kv_shard.hip, on this unit through kv_host.h): kv_comm_*, kv_shard_* (route / serve / finish phases)
//   many tables in one launch: the *_multi entry points (grid.y = table)
//
// Reference semantics restated per function with file:line (relative to the tfplus tree).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <vector>
#include <unordered_set>

// the core's interface; the kernels of the instantiation units (one per optimizer, one for the sums) are reached through
// kv_launch.h, which it includes
#include "kv_host.h"

using namespace kvhip_internal;

namespace {

#include "kv_device.h"
#include "kv_key_update.h"
#include "kv_kernels.h"
#include "kv_fused.h"
#include "kv_papply.h"

// ------------------------------------------------------------------------------------------
// maintenance kernels
// ------------------------------------------------------------------------------------------
__global__ void k_fill_entries(Entry* e, unsigned long long count) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    Entry v; v.key = EMPTY_KEY; v.row = 0; v.hint = 0;
    *reinterpret_cast<uint4*>(&e[i]) = *reinterpret_cast<uint4*>(&v);
  }
}

// re-insert rows [1, next_row) into a fresh index; the slot-row hints travel from the old index (told)
__global__ void k_rehash(TableDev t, TableDev told, unsigned nrows) {
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    if (*flags_ptr(t, r) & FLAG_FREE) continue;  // released by Delete: no index entry
    const long long key = *key_ptr(t, r);
    unsigned hint = 0;
    if (told.entries) { const Entry* oe = table_entry_of(told, key); if (oe) hint = oe->hint; }
    if (key == EMPTY_KEY) {
      Entry* s = &t.entries[t.mask + 1];
      s->key = 0; s->row = r; s->hint = hint;
      continue;
    }
    unsigned long long p = mix64((unsigned long long)key) & t.mask;
    for (;;) {
      unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&t.entries[p].key),
                                         (unsigned long long)EMPTY_KEY, (unsigned long long)key);
      if (old == (unsigned long long)EMPTY_KEY) { t.entries[p].row = r; t.entries[p].hint = hint; break; }
      p = (p + 1) & t.mask;
    }
  }
}
// A batch the partition pass refused (device error 2) after the entry-list tile pass (kv_fused.h tile_insert) had inserted
// its new keys: their index entries are {key, row, HINT_NEW} and their rows have no record yet (no key, no frequency word,
// no contents — the partition pass writes all three).  Every reader that walks the rows (k_stats, k_export, k_rehash,
// k_delete_by_time) would take such a row for a live key 0.  So the report of the error takes them out again: the entry
// becomes a tombstone (probe chains through it stay intact; the same key revives it), the row goes back to the free list.
// One thread per index entry, the sentinel key's entry[mask + 1] included; a row is named by one entry, so it is pushed once.
__global__ void k_rollback_new(TableDev t, unsigned* free_rows, unsigned long long* cnt) {
  const unsigned long long count = t.mask + 2ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    Entry* s = &t.entries[i];
    const Entry e = load_entry(s);
    if (e.key == EMPTY_KEY || e.hint != HINT_NEW) continue;
    s->hint = 0u;
    s->row = ROW_TOMB;
    if (e.row == 0u || e.row == ROW_TOMB || e.row >= t.max_rows) continue;   // (claimed, but the slab was full: no row)
    *flags_ptr(t, e.row) = (unsigned char)FLAG_FREE;
    free_rows[atomicAdd(&t.counters[2], 1u)] = e.row;
    atomicAdd(&cnt[0], 1ull);
  }
}
// kv_uapply.h: the 16-bit launch serial wrapped — every row's stamp back to "none"
__global__ void k_clear_stamps(TableDev t, unsigned nrows) {
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) meta_ptr(t, r)->stamp = 0;
}
// forget every slot-row hint (the attached slot table changed or was cleared)
__global__ void k_clear_hints(Entry* e, unsigned long long count) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (unsigned long long)gridDim.x * blockDim.x) e[i].hint = 0;
}
// kv_attach_slot: every key of the var learns its row in the slot table (one pass over the var's rows) and, mirrors != 0,
// takes a clean copy of that row's frequency word and flags into its own record line (kv_device.h SlotMirror)
__global__ void k_link_hints(TableDev tv, TableDev ts, unsigned nrows, unsigned epoch, int mirrors) {
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    if (mirrors) mirror_ptr(tv, r)->state = (unsigned char)MIRROR_INVALID;
    if (*flags_ptr(tv, r) & FLAG_FREE) continue;
    const long long key = *key_ptr(tv, r);
    const unsigned sr = table_find(ts, key);
    if (!sr) continue;
    Entry* e = table_entry_of(tv, key);
    if (e && load_entry(e).row == r) {
      e->hint = sr;
      if (mirrors) {
        const uint2 sm = load_freq_flags(ts, sr);
        SlotMirror nm;
        nm.srow = sr; nm.freq = sm.x; nm.flags = (unsigned char)(sm.y & 0xFFu); nm.state = (unsigned char)MIRROR_CLEAN;
        nm.epoch = (unsigned short)epoch; nm.pad = 0u;
        *mirror_ptr(tv, r) = nm;
      }
    }
  }
}
// the end of a mirror epoch: what the lean applies wrote into the var rows' mirrors goes back into the slot table's own
// records (a dirty mirror of THIS epoch names a live slot row: nothing else has touched the slot table since it was made)
__global__ void k_flush_mirrors(TableDev tv, TableDev ts, unsigned epoch) {
  const unsigned nrows = min(tv.counters[0], tv.max_rows);
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    SlotMirror* mp = mirror_ptr(tv, r);
    const SlotMirror m = *mp;
    if (m.state != MIRROR_DIRTY || m.epoch != (unsigned short)epoch || m.srow == 0u || m.srow >= ts.max_rows) continue;
    RowMeta* sm = meta_ptr(ts, m.srow);
    sm->freq = m.freq;
    sm->flags = m.flags;
    mp->state = (unsigned char)MIRROR_CLEAN;
  }
}
// the 16-bit epoch wrapped: every mirror back to "none"
__global__ void k_clear_mirrors(TableDev tv) {
  const unsigned nrows = min(tv.counters[0], tv.max_rows);
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x)
    mirror_ptr(tv, r)->state = (unsigned char)MIRROR_INVALID;
}

// size() / sum_freq() kv_variable.h:139-175 ; out[0] = size, out[1] = sum_freq
__global__ void k_stats(TableDev t, unsigned nrows, unsigned long long* out) {
  unsigned long long c = 0, f = 0;
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    const unsigned fl = *flags_ptr(t, r);
    const unsigned fr = *freq_ptr(t, r) & 0xFFFFu;
    if (!(fl & (FLAG_BLACK | FLAG_FREE)) && fr >= t.enter_threshold) { c += 1; f += fr; }
  }
  for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o); f += __shfl_xor(f, o); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], c); atomicAdd(&out[1], f); }
}

}  // namespace

namespace __attribute__((visibility("hidden"))) kvhip_internal {
// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

TableDev dev_view(const kv_table* t) {
  TableDev d;
  d.c0 = t->chunks.empty() ? Chunk{} : t->chunks[0];
  d.entries = t->entries;
  d.mask = t->cap - 1;
  d.chunks = t->d_chunks;
  d.chunk_bits = t->chunk_bits;
  d.counters = t->d_counters;
  d.free_rows = t->free_known > 0 ? t->free_rows : nullptr;
  d.max_rows = (unsigned)std::min<unsigned long long>(t->rows_cap, 0x7FFFFFFFull);
  d.init_table = t->init_table;
  d.init_rows = (unsigned)t->init_rows;
  d.dim = t->dim;
  d.enter_threshold = t->enter_threshold;
  d.seed = t->seed;
  d.track_delta = t->track_delta ? 1u : 0u;
  d.err_host = t->err_host;   // hipHostMallocMapped: the same address on the device
  d.single = t->chunks.size() <= 1 ? 1u : 0u;
  return d;
}

int add_chunk(kv_table* t, hipStream_t s) {
  if (t->chunks.size() >= (size_t)MAX_CHUNKS) return fail(KV_RESOURCE_EXHAUSTED, "row slab: too many chunks");
  const size_t R = (size_t)1 << t->chunk_bits;
  Chunk c{};
  HIP_TRY(hipMalloc(&c.rows, R * t->dim * sizeof(float)));
  HIP_TRY(hipMalloc(&c.meta, R * META_STRIDE * sizeof(RowMeta)));   // (record + slot mirror per row: kv_device.h)
  // every mirror unit starts INVALID (state 0): k_flush_mirrors walks all rows below next_row, also those no apply has met
  HIP_TRY(hipMemsetAsync(c.meta, 0, R * META_STRIDE * sizeof(RowMeta), s));
  if (t->chunks.empty()) {
    // row 0: the permanent zero row
    HIP_TRY(hipMemsetAsync(c.rows, 0, (size_t)t->dim * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c.meta, 0, META_STRIDE * sizeof(RowMeta), s));
  }
  t->chunks.push_back(c);
  HIP_TRY(hipMemcpyAsync(t->d_chunks + (t->chunks.size() - 1), &t->chunks.back(), sizeof(Chunk),
                         hipMemcpyHostToDevice, s));
  t->rows_cap = (unsigned long long)t->chunks.size() << t->chunk_bits;
  return KV_OK;
}

int build_index(kv_table* t, unsigned long long newcap, unsigned nrows, hipStream_t s) {
  Entry* ne = nullptr;
  HIP_TRY(hipMalloc(&ne, (newcap + 1) * sizeof(Entry)));
  k_fill_entries<<<nblocks((long long)newcap + 1, TB, 8192), TB, 0, s>>>(ne, newcap + 1);
  Entry* old = t->entries;
  TableDev told = dev_view(t);   // the old index: its slot-row hints are carried over
  if (!old) told.entries = nullptr;
  t->entries = ne;
  t->cap = newcap;
  if (nrows > 1) {
    k_rehash<<<nblocks(nrows, TB), TB, 0, s>>>(dev_view(t), told, nrows);
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (old) HIP_TRY(hipFree(old));
  return KV_OK;
}

// the free-list stack must hold every row of the slab
int ensure_free_list(kv_table* t, hipStream_t s) {
  if (t->free_cap >= t->rows_cap) return KV_OK;
  unsigned* nf = nullptr;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMalloc(&nf, (size_t)t->rows_cap * sizeof(unsigned)));
  if (t->free_rows) {
    HIP_TRY(hipMemcpy(nf, t->free_rows, (size_t)t->free_cap * sizeof(unsigned), hipMemcpyDeviceToDevice));
    hipFree(t->free_rows);
  }
  t->free_rows = nf;
  t->free_cap = t->rows_cap;
  return KV_OK;
}

static int hop_behind_last(kv_table* t, hipStream_t s);

// The report of a refused batch (code 2) takes the keys its tile pass inserted out of the table again (k_rollback_new).
// A LATER lookup's partition pass may still be pending (the refusal was raised while that lookup's entry settled the
// refused batch's pass): its new keys carry HINT_NEW too and are its own, so it runs first — and if it refuses its batch
// as well, that one's keys go with the same sweep and the flag is cleared once more.
static int rollback_refused(kv_table* t, hipStream_t s) {
  int rc;
  if ((rc = hop_behind_last(t, s)) || (rc = flush_part(t, s)) || (rc = ensure_free_list(t, s))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  k_rollback_new<<<nblocks((long long)t->cap + 1, TB, 8192), TB, 0, s>>>(dev_view(t), t->free_rows, t->d_stat);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(t->d_counters + 1, 0, sizeof(unsigned), s));
  unsigned c[3];
  unsigned long long n = 0;
  HIP_TRY(hipMemcpyAsync(&n, t->d_stat, sizeof n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(c, t->d_counters, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t->pushes_since += n;   // (as after a Delete: kv_ops.hip after_release)
  t->free_known = std::max(0, (int)c[2]);
  t->rows_ub = c[0];
  return KV_OK;
}

// the device error flag was found set at a synchronous point: report once, then clear it so the table
// stays usable (the batch that raised it had no effect beyond rows it may have inserted; a refused batch's — code 2 —
// are taken out again)
int flagged_error(kv_table* t, unsigned code, hipStream_t s) {
  hipMemsetAsync(t->d_counters + 1, 0, sizeof(unsigned), s);
  if (code == 2) {
    const int rc = rollback_refused(t, s);
    if (rc) return rc;
  }
  hipStreamSynchronize(s);
  if (t->err_host) *reinterpret_cast<volatile unsigned*>(t->err_host) = 0u;
  t->batch.drop();   // (from report_deferred_error: ahead of the settle — a pending pass stays for the table's next op; code 2 has run it)
  if (code == 4)
    return fail(KV_INVALID_ARGUMENT, "kv_apply_*_unique: the ids of an earlier call were NOT unique (an id was listed twice): that "
                                     "batch was not applied as the reference applies repeated ids; pass such batches to "
                                     "kv_apply_* (which sums repeated ids) instead");
  if (code == 5)
    return fail(KV_INVALID_ARGUMENT, "kv_apply_unique_counted: the device count of an earlier call was negative or above its n_max: "
                                     "that batch was not applied (the count is not clamped)");
  return fail(KV_INTERNAL, code == 2 ? "an earlier batch was refused: one hash partition received more than 65535 entries, or more "
                                       "distinct keys than a partition block holds that no sub-hash separates (a key set crafted "
                                       "against the hash); those keys were not applied and the ones the batch had inserted were removed again "
                                       "(other keys of that batch may have been: include/kvhip.h, The refused batch)"
                                     : "row slab overflow detected on device");
}

// make room for `extra` more keys (worst case: every id of the batch is new).  rows_ub bounds the
// bump allocator, idx_ub the claimed index entries (a key inserted into a row taken from the free
// list claims a new entry while the deleted key's tombstone stays until the next rebuild).
//
// Stream capture.  A captured call takes its ids from the bounds once, at the capture; every replay inserts on the device
// again, without the host.  From the first captured call on (captured_calls: set here, behind kv_prepare_capture, and
// never cleared — a graph can be replayed at any time) the device may be ahead of both bounds by whatever the replays
// inserted, so every call outside a capture refreshes them from the device before it decides anything: a bound that lags
// would let the device reach the end of the slab first (table_find_or_insert's trap) or fill the index past one half.
// A captured call that finds no room left within the bounds cannot refresh or grow (both synchronise): it is refused
// before anything is queued, as ws_sync refuses a workspace that would have to grow, and the capture stays valid.
int ensure_capacity(kv_table* t, long long extra, hipStream_t s) {
  const bool capturing = t->capture_prepared && stream_is_capturing(s);
  if (capturing) t->captured_calls = true;
  unsigned long long need = t->rows_ub + (unsigned long long)extra;
  unsigned long long need_idx = t->idx_ub + (unsigned long long)extra;
  if ((t->captured_calls && !capturing) || need > t->rows_cap || need_idx * 2 > t->cap) {
    if (capturing || stream_is_capturing(s))
      return fail(KV_FAILED_PRECONDITION, "the table has no room left for the %lld ids of this call within what kv_prepare_capture "
                                          "settled (making room synchronises the stream and may move the table): call "
                                          "kv_prepare_capture outside the stream capture with max_new_ids covering every captured "
                                          "call and every replay", extra);
    // refresh the exact counts before deciding to grow
    unsigned c[3];
    HIP_TRY(hipMemcpyAsync(c, t->d_counters, sizeof c, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (c[1]) return flagged_error(t, c[1], s);
    const long long freed = std::max(0, (int)c[2]);
    t->rows_ub = c[0];
    t->free_known = freed;
    t->idx_ub = t->idx_base + (c[0] - t->bump_base) +
                (unsigned long long)std::max<long long>(0, (long long)t->pushes_since - (freed - t->free_base));
    need = t->rows_ub + (unsigned long long)extra;
    need_idx = t->idx_ub + (unsigned long long)extra;
    if (need >= 0x7FFFFFFFull) return fail(KV_RESOURCE_EXHAUSTED, "more than 2^31 rows in one table");
    while (need > t->rows_cap) {
      int rc = add_chunk(t, s);
      if (rc) return rc;
    }
    if (need_idx * 2 > t->cap) {
      // rebuild from the live rows: tombstones vanish, so the live count decides the size
      const unsigned long long live = t->rows_ub - 1 - (unsigned long long)freed;
      unsigned long long nc = pow2ceil(std::max<unsigned long long>((live + (unsigned long long)extra) * 2, 1024));
      if (nc < t->cap && (live + (unsigned long long)extra) * 4 > t->cap) nc = t->cap;  // no shrink thrash
      int rc = build_index(t, nc, (unsigned)t->rows_ub, s);
      if (rc) return rc;
      t->idx_ub = t->idx_base = live;
      t->bump_base = t->rows_ub;
      t->free_base = freed;
      t->pushes_since = 0;
    }
  }
  t->rows_ub += (unsigned long long)extra;
  t->idx_ub += (unsigned long long)extra;
  return KV_OK;
}

// partitions for a batch of n ids: a power of two <= MAX_P.  Up to 1 M ids: min(1024, n / 32) —
// small batches are cut fine (~32 ids per block) so a 2048-id op still spreads over 64 CUs, large ones
// get 1024 blocks = one resident wave of blocks.  Above 1 M ids: ~1024 ids per partition (2 M ids ->
// 2048 blocks in two waves; with 1024 the hot partitions overflow the LDS entry lists and split:
// measured 331 us vs 2 x 70)
// `many_distinct`: the table's recent batches held mostly distinct ids (err_host[1], below): twice the partitions,
// so that a partition's distinct keys still fit the partition block's LDS hash in one round (1 M nearly distinct ids
// over 1024 partitions are ~960 keys each against 768 slots: every block split its keys and read its entries three
// times)
unsigned pick_partitions(long long n, bool many_distinct = false) {
  if (many_distinct && n >= (1ll << 18)) {
    const unsigned P0 = pick_partitions(n, false);
    return P0 < (unsigned)MAX_P ? P0 * 2u : P0;
  }
  unsigned long long want = std::min<unsigned long long>(1024, (unsigned long long)((n + 31) / 32));
  want = std::max<unsigned long long>(want, (unsigned long long)((n + 1023) / 1024));
  unsigned P = 1;
  while (P < want && P < (unsigned)MAX_P) P <<= 1;
  return P;
}

// the entry-list pipeline's partition count when nothing is known about the batch: about 384 ids per partition block
// (k_part2 works on a tile's distinct keys, not on positions: fewer, fatter partitions than the sorted-position
// pipeline wants), 64 .. 1024; never more than pick_partitions(n), so the workspace of either rule holds it
unsigned fused_default_P(long long n) {
  unsigned P = 64;
  while ((long long)P * 384 < n && P < 1024u) P <<= 1;
  return std::min(P, pick_partitions(n, false));
}

// upper bounds of a batch of n ids: hot keys (more than LCOLD occurrences each) and their chunks
size_t chunk_cap(long long n) { return (size_t)(n / HC + n / (LCOLD + 1) + 4); }

bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
// the workspace grows behind a stream synchronisation: under a stream capture that is refused BEFORE anything is queued
// (a failed synchronisation would invalidate the caller's capture)
int ws_sync(hipStream_t s) {
  if (stream_is_capturing(s))
    return fail(KV_FAILED_PRECONDITION, "the table's batch workspace has to grow for this call, which needs a stream synchronisation: "
                                        "run the op once with this batch length outside the stream capture first");
  HIP_TRY(hipStreamSynchronize(s));
  return KV_OK;
}
int ensure_workspace(kv_table* t, long long n, bool need_part, hipStream_t s) {
  Workspace& w = t->ws;
  const unsigned P = pick_partitions(n, true);
  int rc;
  if (n > w.cap_n || P > w.capP) {
    if ((rc = ws_sync(s))) return rc;
    long long cap = std::max<long long>(n, TILE);
    if (w.cap_n) cap = std::max<long long>(cap, std::min<long long>(w.cap_n * 2, 1ll << 30));
    cap = (cap + TILE - 1) / TILE * TILE;
    const unsigned capP = std::max(pick_partitions(cap, true), P);
    const size_t nt = (size_t)(cap / TILE);
    // every buffer is replaced only once its successor exists; a failure leaves the old sizes in force
    w.cap_n = 0; w.capP = 0; w.hpart_elems = 0; w.epart_elems = 0;
    t->batch.drop();
    if ((rc = regrow(&w.ent_key, (size_t)cap)) || (rc = regrow(&w.ent_a, (size_t)cap)) ||
        (rc = regrow(&w.ent_b, (size_t)cap)) || (rc = regrow(&w.ent_base, (size_t)cap)) || (rc = regrow(&w.ent_rec, (size_t)cap)) ||
        (rc = regrow(&w.toff, nt * (capP + 1))) || (rc = regrow(&w.slot_rank, (size_t)cap)) ||
        (rc = regrow(&w.order, (size_t)cap + 1)) || (rc = regrow(&w.coldlist, 2 * (size_t)cap)) ||
        (rc = regrow(&w.hotlist, 2 * (size_t)cap)) || (rc = regrow(&w.litem, (size_t)cap)) ||
        (rc = regrow(&w.items, (size_t)cap)) || (rc = regrow(&w.pmeta, (size_t)capP + 1)) ||
        (rc = regrow(&w.mcount, nt + 1)))
      return rc;
    if (!w.ctr) {   // zeroed: the first tile pass publishes ctr[5] (the previous pass's distinct keys) as a hint
      HIP_TRY(hipMalloc(&w.ctr, 8 * sizeof(unsigned)));
      HIP_TRY(hipMemset(w.ctr, 0, 8 * sizeof(unsigned)));
    }
#ifdef KV_STAMPS
    if ((rc = regrow(&w.dbg, (size_t)16384 * 16))) return rc;
    hipMemset(w.dbg, 0, (size_t)16384 * 16 * 8);
#endif
    w.cap_n = cap;
    w.capP = capP;
  }
  const long long pe = (long long)chunk_cap(w.cap_n) * (long long)t->dim;
  if (need_part && w.hpart_elems < pe) {
    if ((rc = ws_sync(s))) return rc;
    w.hpart_elems = 0;
    if ((rc = regrow(&w.hpart, (size_t)pe))) return rc;
    w.hpart_elems = pe;
  }
  // the tile sums: [tiles of THIS batch][TILE / 2][dim] — sized by the batch, not by the workspace's doubled capacity
  // (half a row per id: 512 MB for a 1 M-id batch at dim 256), grown by half when a longer batch comes
  const long long ee = ((n + TILE - 1) / TILE) * (long long)(TILE / 2) * (long long)t->dim;
  if (need_part && w.epart_elems < ee) {
    if ((rc = ws_sync(s))) return rc;
    const long long want = std::max(ee, std::min((w.cap_n / 2) * (long long)t->dim, w.epart_elems + w.epart_elems / 2));
    w.epart_elems = 0;
    if ((rc = regrow(&w.epart, (size_t)want))) return rc;
    w.epart_elems = want;
  }
  return KV_OK;
}

// Workspace::pos_ent holds n positions (every position's entry number in its tile: the table-less tile pass of the
// distinct-id ops and the sharded route, kv_lookup_sparse's combiner)
int ensure_pos_ent(kv_table* t, long long n, hipStream_t s) {
  Workspace& w = t->ws;
  if (w.pos_cap >= n) return KV_OK;
  int rc;
  if ((rc = ws_sync(s))) return rc;
  const long long cap = std::max<long long>(n, w.cap_n);
  w.pos_cap = 0;
  if ((rc = regrow(&w.pos_ent, (size_t)cap))) return rc;
  w.pos_cap = cap;
  return KV_OK;
}

// Workspace::pseg / pscale hold n positions (the sharded sparse apply's position records, on the route table)
int ensure_pos_records(kv_table* t, long long n, hipStream_t s) {
  Workspace& w = t->ws;
  if (w.prec_cap >= n) return KV_OK;
  int rc;
  if ((rc = ws_sync(s))) return rc;
  const long long cap = std::max<long long>(n, w.cap_n);
  w.prec_cap = 0;
  if ((rc = regrow(&w.pseg, (size_t)cap)) || (rc = regrow(&w.pscale, (size_t)cap))) return rc;
  w.prec_cap = cap;
  return KV_OK;
}

WsDev ws_view(kv_table* t, long long n, const SelfSegment* self) {
  Workspace& w = t->ws;
  WsDev d;
  d.ent_key = w.ent_key; d.ent_a = w.ent_a; d.ent_b = w.ent_b; d.ent_base = w.ent_base; d.ent_rec = w.ent_rec;
  d.toff = w.toff;
  d.slot_rank = w.slot_rank;
  d.order = w.order;
  d.coldlist = w.coldlist;
  d.hotlist = w.hotlist;
  d.litem = w.litem;
  d.items = w.items;
  d.pmeta = w.pmeta;
  d.hpart = w.hpart;
  d.ctr = w.ctr;
  d.ntiles = (unsigned)((n + TILE - 1) / TILE);
  use_partitions(d, pick_partitions(n));
  d.seg_cap = 0;
  d.zero_counts = nullptr;
  d.dbg = w.dbg;
  // entry-list pipeline: mrow lives in slot_rank's storage
  d.mrow = w.slot_rank;
  d.mcount = w.mcount;
  d.epart = w.epart;
  d.pos_ent = nullptr;
  d.self_lo = d.self_len = 0; d.ids_self = nullptr; d.grad_self = nullptr;
  if (self) { d.self_lo = self->lo; d.self_len = self->len; d.ids_self = self->ids; d.grad_self = self->grad; }
  return d;
}


// the optimizers' row math on the hardware's 1-ulp sqrt / reciprocal (kv_device.h kv_sqrt / kv_div)?
bool fast_math_on(const kv_table* t) { return t->fast_math && !t->deterministic; }
// PartArgs::det: 0 arrival order, 1 an order fixed by the input positions, 2 occurrence order (one chain per key; kv_kernels.h)
int det_mode(const kv_table* t) { return t->occurrence_order ? 2 : t->deterministic ? 1 : 0; }

unsigned today(const kv_table* t) {
  if (t->fixed_day >= 0) return (unsigned)t->fixed_day & 0xFFFFu;
  return (unsigned)(std::time(nullptr) / (3600 * 24)) & 0xFFFFu;  // utility.cc:38-40
}

// tile pass.  FIRST: scatter / mark flavour (one input position per key instead of the counts).
// ids_kind: -1 = the table's key dtype, 0 int64, 1 int32, 2 (id, count) int64 pairs (lookups only).
// md != nullptr: the same launch over `ntab` tables (grid.y), arguments from the descriptor array
// md, grid.x = gx (the largest table's tile count)
template <bool FIRST>
void launch_tile(kv_table* t, const WsDev& wd, const void* ids, const int* counts, long long n, hipStream_t s,
                 int ids_kind, const MultiDesc* md, int ntab, unsigned gx) {
  if (ids_kind < 0) ids_kind = t->key_dtype == KV_DT_INT32 ? 1 : 0;
  const int grid = (int)wd.ntiles;
  const size_t sh = tile_smem_bytes(FIRST);
  const int det = det_mode(t);
#define KV_TILE(IDT)                                                                     \
  do {                                                                                   \
    if (md) k_tile_multi<FIRST, IDT><<<dim3(gx, (unsigned)ntab), TBT, sh, s>>>(md);       \
    else k_tile<FIRST, IDT><<<grid, TBT, sh, s>>>(wd, (const IDT*)ids, counts, n, det);  \
  } while (0)
  if (ids_kind == 2) {
    if constexpr (!FIRST) KV_TILE(IdCount);
  } else if (ids_kind == 1) KV_TILE(int);
  else KV_TILE(long long);
#undef KV_TILE
}

// out[i] = rows[row of ids[i]] after the lookup index passes; md: many tables in one launch.
// order: the same kernel also builds the sorted position list (the training lookup's third and last kernel)
void launch_gather(const TableDev& td, const WsDev& wd, float* op, long long m, hipStream_t s,
                   const MultiDesc* md, int ntab, bool order) {
  const int D = td.dim;
  const int q = pow2_vectors(D, TB);   // a lane group per row; 0: the generic body, one thread per element
  constexpr int gcap = 8192;  // one 64-row step per wave at 1M rows: residency, not a loop, hides the hops
  const int grid = q ? nblocks(m, q <= 64 ? TB : TB / q, gcap) : nblocks(m * D, TB, 4096);   // (q > 64: TB / q rows per block)
  auto launch = [&](auto vq) {
    constexpr int VQ = decltype(vq)::value;
    if (md) k_gather_multi<VQ><<<dim3((unsigned)grid, (unsigned)ntab), TB, 0, s>>>(md);
    else if (order) k_gather<VQ, true><<<grid + ITEM_BLOCKS, TB, 0, s>>>(td, wd, op, m);
    else k_gather<VQ, false><<<grid, TB, 0, s>>>(td, wd, op, m);
  };
  if (q) with_lanes<TB>(q, launch);
  else launch(std::integral_constant<int, 0>{});
}

// partition pass.  multi (md != nullptr): wd carries the LARGEST ntiles / P of the batch of tables (LDS
// sizing, grid.x); instantiated for MODE_LOOKUP and MODE_APPLYIDX
template <int MODE>
void launch_part_keys(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab) {
  const int grid = (int)wd.P;
  const size_t sh = (size_t)wd.ntiles * 4 + 32;
  if constexpr (MODE == MODE_LOOKUP || MODE == MODE_APPLYIDX) {
    if (md) {
      k_part_keys_multi<MODE><<<dim3((unsigned)grid, (unsigned)ntab), TBK, sh, s>>>(md);
      return;
    }
  }
  k_part_keys<MODE><<<grid, TBK, sh, s>>>(wd, pa);
}
// sorted position list of the batch (the training lookup builds it in its gather kernel instead)
void launch_order(const TableDev& td, const WsDev& wd, long long n, hipStream_t s,
                  const MultiDesc* md, int ntab) {
  const int grid = nblocks(n, TB, 4096) + ITEM_BLOCKS;   // ITEM_BLOCKS blocks in front build the item directory only
  if (md) k_order_multi<<<dim3((unsigned)grid, (unsigned)ntab), TB, 0, s>>>(md);
  else k_order<<<grid, TB, 0, s>>>(td, wd, n);
}
// ... and tables: one in occurrence-order mode takes the sorted-position pipeline for every op, like a dim the entry-list
// kernels do not serve (its sums are one chain per key there; the entry lists sum tile by tile)
bool fused_tab(const kv_table* t) { return fused_ok(t->dim) && !t->occurrence_order; }
// tile pass: dedup, index probes / inserts, entries, tile-local order and (out != nullptr) the output rows
// md != nullptr: `ntab` tables in one launch (grid.y), arguments from the descriptor array; multi_rows: with rows
void launch_ltile(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, const int* counts, long long n, float* out,
                  hipStream_t s, int ids_kind, const MultiDesc* md, int ntab, bool multi_rows) {
  if (ids_kind < 0) ids_kind = t->key_dtype == KV_DT_INT32 ? 1 : 0;
  const int grid = (int)wd.ntiles;
  const size_t sh = ltile_smem_bytes();
  const int det = det_mode(t);
  auto launch = [&](auto id) {
    using IDT = decltype(id);
    with_lanes(row_lanes(td.dim), [&](auto vq) {
      constexpr int VQ = decltype(vq)::value;
      if (md && multi_rows) k_ltile_multi<IDT, VQ, true><<<dim3((unsigned)grid, (unsigned)ntab), TBT, sh, s>>>(md);
      else if (md) k_ltile_multi<IDT, 1, false><<<dim3((unsigned)grid, (unsigned)ntab), TBT, sh, s>>>(md);
      else if (out) k_ltile<IDT, VQ, true><<<grid, TBT, sh, s>>>(td, wd, (const IDT*)ids, counts, n, det, out);
      else k_ltile<IDT, 1, false><<<grid, TBT, sh, s>>>(td, wd, (const IDT*)ids, counts, n, det, nullptr);
    });
  };
  if (ids_kind == 2) launch(IdCount{});
  else if (ids_kind == 1) launch(int{});
  else launch((long long)0);
}
// the table-less tile pass of the sharded route (int64 ids): entries, mrow, every position's entry number
void launch_ltile_notable(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, long long n, hipStream_t s,
                          const int* counts, bool int32_ids) {
  with_id_type(int32_ids, [&](auto id) {
    using IDT = decltype(id);
    k_ltile<IDT, 1, false, true><<<(int)wd.ntiles, TBT, ltile_smem_bytes(), s>>>(td, wd, (const IDT*)ids, counts, n, det_mode(t), nullptr);
  });
}
// ... of `ntab` sharded routes in one launch (wmax: the largest ntiles of the batch of tables)
void launch_ltile_multi_notable(const WsDev& wmax, int ntab, const MultiDesc* md, hipStream_t s) {
  k_ltile_multi_notable<<<dim3(wmax.ntiles, (unsigned)ntab), TBT, ltile_smem_bytes(), s>>>(md);
}
// the bookkeeping of a training lookup that no apply takes over (k_part2); md: `ntab` tables in one launch
void launch_part2(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md, int ntab) {
  if (md) k_part2_multi<<<dim3(wd.P, (unsigned)ntab), TBK, (size_t)wd.ntiles * 4 + 32, s>>>(md);
  else k_part2<<<(int)wd.P, TBK, (size_t)wd.ntiles * 4 + 32, s>>>(wd, pa);
}

// occurrence order (pa.det == 2): the hot keys' chains, one block per key, the sums to hpart; k_apply reads them
// (launch_apply, kv_host.h).  nmax: ids of the batch
int launch_occ_sum(const WsDev& wd, const PartArgs& pa, int fop, long long nmax, hipStream_t s) {
  const int D = pa.tv.dim;
  const unsigned og = (unsigned)std::max<long long>(1, std::min<long long>(2048, nmax / 256 + 1));
  const int nc = (D + 63) / 64;
  // (two stages + positions: above the 64 KB a launch gets without asking — per device, so asked at every launch)
#define KV_OCC(NC_)                                                                                                          \
  do {                                                                                                                       \
    HIP_TRY(hipFuncSetAttribute((const void*)k_occ_sum<NC_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)occ_smem_bytes())); \
    k_occ_sum<NC_><<<og, OCC_TB, occ_smem_bytes(), s>>>(wd, pa, fop);                                                        \
  } while (0)
  if (nc <= 1) KV_OCC(1);
  else if (nc <= 2) KV_OCC(2);
  else if (nc <= 4) KV_OCC(4);
  else if (nc <= 8) KV_OCC(8);
  else KV_OCC(16);
#undef KV_OCC
  return KV_OK;
}

bool dim_supported(int D) { return (D & 3) == 0 ? D <= 1024 : D <= 256; }

// A batch the index pass gave up on (a hash partition with more than 65535 entries, or keys that no
// sub-hash separates) raises the device flag AND this pinned host word; every later kernel of that op saw
// the flag and did nothing.  The next call on the table reports it — no synchronisation on the good path.
int report_deferred_error(kv_table* t, hipStream_t s) {
  if (!t->err_host || *reinterpret_cast<volatile unsigned*>(t->err_host) == 0u) return KV_OK;
  const unsigned code = *reinterpret_cast<volatile unsigned*>(t->err_host);
  hipStreamSynchronize(s);
  return flagged_error(t, code, s);
}

// a lookup's partition pass (wd, pa) stays pending on the table (BatchIndex::defer_part)
void set_pending_part(kv_table* t, const WsDev& wd, const PartArgs& pa) {
  std::memcpy(t->pend_wd, &wd, sizeof wd);
  std::memcpy(t->pend_pa, &pa, sizeof pa);
  t->batch.defer_part();
}
// ... and is taken over by the optimizer apply of that batch (k_papply PA_LOOKUP completes it): not pending any more;
// *lookup = the pending lookup's own arguments (the apply wants its day stamp and counting rule)
void take_pending_part(kv_table* t, PartArgs* lookup) {
  std::memcpy(lookup, t->pend_pa, sizeof *lookup);
  t->batch.part_taken();
}
// launches a lookup's pending partition pass (BatchIndex::defer_part) on stream s
int flush_part(kv_table* t, hipStream_t s) {
  if (!t->batch.part_pending()) return KV_OK;
  t->batch.part_flushed();
  WsDev wd; PartArgs pa;
  std::memcpy(&wd, t->pend_wd, sizeof wd);
  std::memcpy(&pa, t->pend_pa, sizeof pa);
  ProfScope ps(t, KV_PROF_LOOKUP_PART, s);
  // (k_part2 reads the tiles' entries alone — also behind a sharded owner lookup whose own segment stayed in the send
  //  buffers; an apply that still comes with the batch's token runs k_papply PA_NONE over the same entries)
  launch_part2(wd, pa, s);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// ---- slot mirrors: the host side -------------------------------------------------------------------------------------
// Invariant: the slot table's own records are up to date for every key whose var-row mirror is not (valid in the current
// epoch AND dirty).  Mirrors are written only by the lean apply of (var, slot) — k_papply / k_uapply with use_mirror — and
// read only by it.  EVERY other op that enters either table first ends the epoch (flush the dirty copies, one kernel over
// the var's rows, then epoch + 1 — which invalidates every copy at once), so it sees, and may change, the authoritative
// records; the keys' next lean apply finds no valid mirror, takes the general path once and leaves a fresh clean copy
// (finish_key).  An op that keeps the epoch says so where it enters the table, with the role(s) it keeps the table in
// (KEEP_*, kv_host.h).  A role, not a table, is kept: a var entered as KEEP_VAR that is also another var's slot table still
// ends that other pair's epoch.
// The locks: a pair is ONE record (MirrorPair, kv_host.h).  A table's reference to it (pair_var, pair_slot) is read and
// written under that table's own mu, never by the partner.  What is in the record is read and written under the record's
// mu, the innermost lock: mirror_visit and the lean apply (mirror_decide) take it once and are the transitions.

// ends p's epoch (p.mu held) on s: the write-back with the number the dirty copies carry, the clearing on wrap.  The event
// stands behind the last write-back; a call that launched none (the pair's other side may just have, on its own stream)
// waits for it before its op reads a slot record.  write_back == false: the slot table is going, its records with it
static void pair_end_epoch(MirrorPair& p, hipStream_t s, bool write_back) {
  const MirrorEpoch::End e = p.epoch.end();
  const long long rows = (long long)p.view_var.max_rows + 1;
  const bool flush = e.flush && write_back;
  if (flush) k_flush_mirrors<<<nblocks(rows, TB, 8192), TB, 0, s>>>(p.view_var, p.view_slot, e.flush_epoch16);
  if (e.clear_all) k_clear_mirrors<<<nblocks(rows, TB, 8192), TB, 0, s>>>(p.view_var);
  if (flush || e.clear_all) hipEventRecord(p.flushed, s);
  else hipStreamWaitEvent(s, p.flushed, 0);
}
// What table t (t->mu held) does to the pair behind `ref`, one of its own two references, on stream s.  A table that leaves
// dissolves the pair (the dirty copies go back); its partner, whose lock the leaver need not hold, finds the record
// dissolved whatever it came for, and leaves too, behind the leaver's write-back.  A var that leaves keeps the record's next
// epoch: its rows still hold the copies, and only a number none of them carries makes them void in its next pair.
// Under a stream capture the flush would be RECORDED, not run, and a replay would carry the epoch of its capture: a table
// that is captured gives up its mirrors beforehand (kv_prepare_capture); an op that would end an epoch in a capture is refused.
enum MirrorVisit { LOOK, END_EPOCH, LEAVE, LEAVE_NO_FLUSH };
static int mirror_visit(kv_table* t, std::shared_ptr<MirrorPair>& ref, hipStream_t s, MirrorVisit what) {
  if (!ref) return KV_OK;
  {
    std::lock_guard<std::mutex> l(ref->mu);
    if (!ref->dissolved) {
      if (what == LOOK) return KV_OK;
      if (what == END_EPOCH && stream_is_capturing(s))
        return fail(KV_FAILED_PRECONDITION, "this table is half of a (var, slot) pair whose optimizer applies keep the slot records' "
                                            "frequency words in the var's rows between ops; call kv_prepare_capture on it (outside the "
                                            "capture) before capturing ops on it");
      pair_end_epoch(*ref, s, what != LEAVE_NO_FLUSH);
      if (what == END_EPOCH) return KV_OK;
      ref->dissolved = true;
    } else if (!stream_is_capturing(s)) hipStreamWaitEvent(s, ref->flushed, 0);
    if (&ref == &t->pair_var) { t->mirror_next = ref->epoch.epoch16(); t->stat_mirror_epochs = ref->epoch.ended(); }
  }
  ref.reset();
  return KV_OK;
}
// ... LOOK: is there a live pair behind ref?
static bool mirror_live(kv_table* t, std::shared_ptr<MirrorPair>& ref, hipStream_t s) { mirror_visit(t, ref, s, LOOK); return ref != nullptr; }
// the entry hook of hand_over / join_side: a role the op does not keep the table in ends its pair's epoch
int mirror_on_entry(kv_table* t, hipStream_t s, unsigned keep) {
  int rc = KV_OK;
  if (!(keep & KEEP_SLOT)) rc = mirror_visit(t, t->pair_slot, s, END_EPOCH);         // its records are about to be read or written
  if (!rc && !(keep & KEEP_VAR)) rc = mirror_visit(t, t->pair_var, s, END_EPOCH);    // its rows may be released, moved or read back
  return rc;
}
// kv_prepare_capture: no host code runs at a replay, so nothing could flush or re-validate a mirror: no pair, now or ever
void mirror_ban(kv_table* t, hipStream_t s) {
  mirror_visit(t, t->pair_var, s, LEAVE);
  mirror_visit(t, t->pair_slot, s, LEAVE);
  t->mirror_banned = true;
}
// (var, slot) become a mirror pair — or stay / become unpaired when the slot table already serves another var (both locks held)
bool mirror_pair(kv_table* v, kv_table* sl, hipStream_t s) {
  if (sl->mirror_shared || v->mirror_banned || sl->mirror_banned) return false;
  // (one record in both tables' hands is live: whoever dissolves it holds one of the two locks and drops its reference at once)
  if (v->pair_var && v->pair_var == sl->pair_slot) return true;
  if (mirror_live(sl, sl->pair_slot, s)) {   // a second var on one slot table: no mirrors for it at all
    mirror_visit(sl, sl->pair_slot, s, LEAVE);
    sl->mirror_shared = true;
    return false;
  }
  mirror_visit(v, v->pair_var, s, LEAVE);   // a change of slot table
  auto p = std::make_shared<MirrorPair>();
  if (hipEventCreateWithFlags(&p->flushed, hipEventDisableTiming) != hipSuccess) return false;
  p->epoch = MirrorEpoch(v->mirror_next, v->stat_mirror_epochs);
  p->view_var = dev_view(v); p->view_slot = dev_view(sl);
  v->pair_var = sl->pair_slot = p;
  mirror_visit(v, v->pair_var, s, END_EPOCH);   // a fresh epoch: whatever bytes the rows' mirror units hold are void
  return true;
}

// Does this apply of (v, s0) work on the var rows' slot mirrors?  lean: the launch is k_papply / k_uapply (their lean
// update is the only code that reads or writes a mirror).  Otherwise the apply reads and writes the slot table's own
// records: the epoch ends first (the caller entered the var as KEEP_VAR and the slot as KEEP_SLOT, so nothing has ended it yet).
// (lean is false for an optimizer with two slot tables: the caller passes lean && !two_slots(OPT))
int mirror_decide(kv_table* v, kv_table* s0, PartArgs& pa, bool lean, hipStream_t s) {
  pa.use_mirror = 0; pa.mirror_epoch = 0u;
  // (a captured apply of a pair that still has mirrors: their flush would be recorded, not run — see mirror_visit)
  if ((v->pair_var || s0->pair_slot) && stream_is_capturing(s) && (mirror_live(v, v->pair_var, s) || mirror_live(s0, s0->pair_slot, s)))
    return fail(KV_FAILED_PRECONDITION, "optimizer apply under stream capture on a (var, slot) pair with live slot mirrors: call "
                                        "kv_prepare_capture on both tables (outside the capture) first");
  const bool eligible = lean && pa.use_hints != 0 && pa.tv.single != 0u && pa.ts0.single != 0u &&
                        !v->track_delta && !s0->track_delta && !stream_is_capturing(s) && mirror_pair(v, s0, s);
  if (eligible) {
    MirrorPair& p = *v->pair_var;
    std::lock_guard<std::mutex> l(p.mu);
    p.view_var = dev_view(v); p.view_slot = dev_view(s0);   // what this apply's dirty copies name is inside these views
    pa.use_mirror = 1;
    pa.mirror_epoch = p.epoch.lean_apply();
    ++v->stat_mirror_applies;
    return KV_OK;
  }
  int rc = mirror_visit(v, v->pair_var, s, END_EPOCH);
  if (!rc && s0->pair_slot != v->pair_var) rc = mirror_visit(s0, s0->pair_slot, s, END_EPOCH);
  return rc;
}

// Ops of one table run in the order they were issued, whatever their streams: the per-table workspace
// and the table itself are shared by every op (the reference's table locks cover execution, not just
// enqueue, training_ops.cc:96-184).  Same stream as the last op: nothing to do.  Another stream: it first
// waits for everything the previous stream had been given, and is the table's last stream from there on.
static int hop_behind_last(kv_table* t, hipStream_t s) {
  if (!t->has_last || t->last_stream == s) return KV_OK;
  HIP_TRY(hipEventRecord(t->last_done, t->last_stream));
  HIP_TRY(hipStreamWaitEvent(s, t->last_done, 0));
  t->last_stream = s;
  return KV_OK;
}

// keep: the mirror role(s) the op keeps the table in (KEEP_*; mirror_on_entry)
// settle == false: the caller is the optimizer apply that takes the table's pending partition pass over
// mutates == false: a read-only op (the inference gathers): ordered like any other op of the table — behind the table's
// last op whatever its stream, and the next op behind it — but it does not move op_serial (a two-phase export may go on)
int hand_over(kv_table* t, hipStream_t s, unsigned keep, bool settle, bool mutates) {
  int rc;
  if (t->batch.part_pending() && settle) {   // (an apply that takes the batch over runs it itself, behind the stream hand-over below)
    if ((rc = hop_behind_last(t, s)) || (rc = flush_part(t, s))) return rc;
  }
  if ((rc = hop_behind_last(t, s))) return rc;
  t->last_stream = s;
  t->has_last = true;
  if (mutates) ++t->op_serial;
  return mirror_on_entry(t, s, keep);
}

// ops that read a table without the full hand_over (no workspace, no row-set change): the last lookup's pending
// partition pass (it may still have rows to initialise) is settled first.  None of them keeps a mirror epoch.
int join_side(kv_table* t, hipStream_t s) {
  int rc;
  if (t->batch.part_pending()) {
    if ((rc = hop_behind_last(t, s)) || (rc = flush_part(t, s))) return rc;
  }
  // An epoch of slot mirrors that ends here flushes copies the last lean apply wrote — on the stream of t's last op (an apply
  // enters both tables; anything later on t has ended the epoch already): the flush must run behind it.  (A flush that
  // overtook the apply would miss its copies, and the epoch number that ends with it would orphan them for good.)
  if ((t->pair_var || t->pair_slot) && (rc = hop_behind_last(t, s))) return rc;
  return mirror_on_entry(t, s, KEEP_NONE);
}

// How an op enters a table it holds the lock of: the deferred error of the table's last batch, then the hand-over.
int enter_op(kv_table* t, hipStream_t s, unsigned keep, bool settle, bool mutates) {
  int rc;
  if ((rc = report_deferred_error(t, s))) return rc;
  return hand_over(t, s, keep, settle, mutates);
}

// The index of a batch (kv_kernels.h): tile pass, partition pass, sorted position list.
//   MODE_LOOKUP   with out != nullptr: the training lookup (rows copied by the kernel that builds the list)
//   MODE_APPLYIDX the optimizer meets the ids first (FindOrInsertUnsafe on the var table)
//   MODE_UNIQUE   no table: dense unique indices (pa.out_keys / direct_rows)
template <int MODE>
void index_pass(kv_table* t, const WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                int ids_kind, float* out, hipStream_t s, bool file_order) {
  {
    ProfScope ps(t, MODE == MODE_LOOKUP ? KV_PROF_LOOKUP_TILE : KV_PROF_INDEX, s);
    launch_tile<false>(t, wd, ids, counts, n, s, ids_kind);
  }
  {
    ProfScope ps(t, MODE == MODE_LOOKUP ? KV_PROF_LOOKUP_PART : KV_PROF_INDEX, s);
    launch_part_keys<MODE>(wd, pa, s);
  }
  ProfScope ps(t, MODE == MODE_LOOKUP ? KV_PROF_LOOKUP_ORDER : KV_PROF_INDEX, s);
  // file_order == false: a lookup nobody will follow with an apply of the same batch (no token asked for): the
  // plain gather, 36 instead of 48 us at configs[1]
  if (MODE == MODE_LOOKUP && out) launch_gather(pa.tv, wd, out, n, s, nullptr, 0, file_order);
  else launch_order(pa.tv, wd, n, s);
}

// partitions of an entry-list index pass over n ids (wd.P, wd.pshift; whoever publishes the index hands P to BatchIndex::publish)
void choose_partitions(kv_table* t, WsDev& wd, long long n) {
  {
    // the distinct ids of the batch before the last one (the tile pass hands the partition pass's count to the host
    // through a pinned word, no synchronisation): mostly distinct ids -> twice the partitions
    const unsigned u_prev = t->err_host ? reinterpret_cast<volatile unsigned*>(t->err_host)[1] : 0u;
    // (not in deterministic mode: the partitioning decides the order of a tile's entries, hence of the additions —
    // there it depends on the batch alone)
    const bool hinted = !t->deterministic && t->batch_n_prev == n && u_prev > 0u;
    t->batch_n_prev = n;
    if (hinted) {
      // about 384 distinct keys per partition block (the LDS hash of k_part2 holds 768 before a partition splits),
      // at most 2048 entries: 109 k keys of 1 M ids (Zipf 1.2) -> 512 partitions, 773 k (Zipf 0.8) -> 2048.
      // Measured at 1 M ids: 512 against 1024 partitions is -2.5 us per step at Zipf 1.2 and +40 us at Zipf 0.8.
      // With k_papply (kv_papply.h) the partition block also applies its keys' updates: two blocks of eight waves per
      // CU, about 256 keys per block (109 k keys -> 512 partitions, one resident generation: 60 us; four blocks of four
      // waves with 128 keys each 64.7 us, one block of sixteen waves with 512 keys 75 us; profiles/r04_tools_output.txt).
      // (a hint is only a hint: never more distinct keys than ids, never more partitions than the workspace was sized for)
      const unsigned long long u = std::min<unsigned long long>(u_prev, (unsigned long long)n);
      const unsigned long long per = 256ull;
      const unsigned long long want = std::max<unsigned long long>((u + per - 1ull) / per, (unsigned long long)((n + 2047) / 2048));
      const unsigned pmax = std::min<unsigned>((unsigned)MAX_P, std::max(64u, t->ws.capP));
      unsigned P = 64;
      while (P < want && P < pmax) P <<= 1;
      wd.P = P;
    } else {
      wd.P = fused_default_P(n);
    }
    wd.pshift = 64 - ilog2(wd.P);
  }
}

// The training lookup on the entry-list kernels (kv_fused.h): the tile pass with the output rows; then the lookup's
// bookkeeping (k_part2) — or, defer_part: it stays PENDING for the optimizer apply of this batch (k_papply completes it
// in the same pass as the update) or for whatever op the table sees next (flush_part)
int fused_lookup_pass(kv_table* t, WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                      int ids_kind, float* out, hipStream_t s, bool defer_part) {
  choose_partitions(t, wd, n);
  {
    ProfScope ps(t, KV_PROF_LOOKUP_TILE, s);
    launch_ltile(t, pa.tv, wd, ids, counts, n, out, s, ids_kind);
  }
  if (defer_part) {   // the rows are out: the partition pass waits for the table's next op
    set_pending_part(t, wd, pa);
    return KV_OK;
  }
  ProfScope ps(t, KV_PROF_LOOKUP_PART, s);
  launch_part2(wd, pa, s);
  return KV_OK;
}

// Every live table: a stream the LIBRARY owns (a communicator's) is retired from the tables that last ran on it before it
// is destroyed — hand_over would otherwise record an event on a dead stream at the table's next op (found in round 6:
// bench.py's sharded_world1 sub-record destroys its communicator, the next lookup on another stream crashed in
// hipEventRecord).  A stream the CALLER owns must outlive the table's next op, or the caller synchronises it first and
// calls kv_forget_stream.
std::mutex g_tables_mu;
std::unordered_set<kv_table*> g_tables;
void retire_stream(hipStream_t dead) {   // `dead` is drained (the caller synchronised it)
  {
    std::lock_guard<std::mutex> l(g_tables_mu);
    for (kv_table* t : g_tables) {
      std::lock_guard<std::mutex> lt(t->mu);
      if (t->has_last && t->last_stream == dead) { t->has_last = false; t->last_stream = nullptr; }
    }
  }
  // ... and the staging slots whose last launch ran there have been read: their events are not waited on again
  for (auto& dev : g_stage)
    for (BatchStage& st : dev) {
      std::lock_guard<std::mutex> l(st.mu);
      for (StageSlot& sl : st.slot)
        if (sl.busy && sl.last == dead) sl.busy = false;
    }
}

std::atomic<uint64_t> g_serial{0};   // batch tokens
std::atomic<uint64_t> g_uid{0};

// descriptor staging for the batched launches: one pinned host buffer + device buffer per device
// and descriptor kind; the next upload waits until the previous launch has consumed the buffer
BatchStage g_stage[64][3];   // [device][0 = inference gather, 1 = training ops, 2 = the sparse lookups' own descriptors]

// returns with st.mu HELD (released by ~Staged after `consumed` is recorded on the stream)
int stage_take(BatchStage& st, size_t bytes, StageSlot** out) {
  st.mu.lock();
  StageSlot& sl = st.slot[st.cursor++ & 3u];
  const hipError_t busy = sl.busy ? hipEventSynchronize(sl.consumed) : hipSuccess;
  if (busy != hipSuccess) {
    st.mu.unlock();
    return fail(KV_INTERNAL, "descriptor staging: event sync failed (%s)", hipGetErrorString(busy));
  }
  sl.busy = false;
  if (sl.cap < bytes) {
    if (sl.host) hipHostFree(sl.host);
    if (sl.dev) hipFree(sl.dev);
    sl.host = sl.dev = nullptr;
    sl.cap = std::max<size_t>(bytes, 64 * 1024);
    if (hipHostMalloc(&sl.host, sl.cap) != hipSuccess || hipMalloc(&sl.dev, sl.cap) != hipSuccess ||
        (!sl.consumed && hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming) != hipSuccess)) {
      sl.cap = 0;
      st.mu.unlock();
      return fail(KV_RESOURCE_EXHAUSTED, "descriptor staging: allocation failed");
    }
  }
  *out = &sl;
  return KV_OK;
}

// the descriptors of captured batched calls (kv_host.h): blocks of pinned host + device memory, filled front to back, never
// handed out twice and never freed
struct CaptureStage {
  struct Block { char* host; char* dev; size_t used; };
  std::mutex mu;
  std::vector<Block> blocks;
};
static CaptureStage g_capture_stage[64];
int capture_stage_reserve(int device) {
  if (device < 0 || device >= 64) return fail(KV_INVALID_ARGUMENT, "device index");
  CaptureStage& a = g_capture_stage[device];
  std::lock_guard<std::mutex> l(a.mu);
  if (!a.blocks.empty() && a.blocks.back().used == 0) return KV_OK;   // a whole block is free
  CaptureStage::Block b{nullptr, nullptr, 0};
  if (hipHostMalloc(&b.host, CAPTURE_STAGE_ROOM) != hipSuccess) return fail(KV_RESOURCE_EXHAUSTED, "capture staging: allocation failed");
  if (hipMalloc(&b.dev, CAPTURE_STAGE_ROOM) != hipSuccess) {
    hipHostFree(b.host);
    return fail(KV_RESOURCE_EXHAUSTED, "capture staging: allocation failed");
  }
  // (an earlier block keeps what is left of it: the next take may still fit there)
  a.blocks.push_back(b);
  return KV_OK;
}
int capture_stage_take(int device, size_t bytes, char** host, char** dev) {
  bytes = (bytes + 255) & ~(size_t)255;
  CaptureStage& a = g_capture_stage[device];
  std::lock_guard<std::mutex> l(a.mu);
  for (CaptureStage::Block& b : a.blocks)
    if (CAPTURE_STAGE_ROOM - b.used >= bytes) {
      *host = b.host + b.used;
      *dev = b.dev + b.used;
      b.used += bytes;
      return KV_OK;
    }
  return fail(KV_FAILED_PRECONDITION, "a batched call under stream capture keeps its %zu bytes of descriptors for every replay, and "
                                      "the room kv_prepare_capture sets aside for them is used up (or was never made): call "
                                      "kv_prepare_capture on a table of this device outside the stream capture first", bytes);
}

int check_same_shape(int num_tables, const kv_handle_t* tables, const char* what) {
  int rc;
  if (num_tables < 1) return fail(KV_INVALID_ARGUMENT, "N must be >= 1");
  if (!tables) return fail(KV_INVALID_ARGUMENT, "null argument array");
  for (int i = 0; i < num_tables; ++i) {
    if ((rc = check_table(tables[i]))) return rc;
    if (tables[i]->device != tables[0]->device) return fail(KV_INVALID_ARGUMENT, "%s live on different devices", what);
  }
  if (tables[0]->device < 0 || tables[0]->device >= 64) return fail(KV_INVALID_ARGUMENT, "device index");
  return KV_OK;
}

// A lookup's deferred passes hold a snapshot of the table's arrays (pend_pa): whatever moves or frees those arrays, or
// changes what the passes would compute (seed, deterministic order), first lets them run — on the stream of the
// table's last op — and waits for them.
int settle_pending(kv_table* t) {
  if (!t->batch.part_pending()) return KV_OK;
  hipStream_t s = t->has_last ? t->last_stream : nullptr;
  int rc;
  if ((rc = join_side(t, s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return KV_OK;
}

int stats(kv_handle_t t, hipStream_t s, unsigned long long out[2], unsigned* nrows_out) {
  { const int jr = join_side(t, s); if (jr) return jr; }
  unsigned c[3];
  HIP_TRY(hipMemcpyAsync(c, t->d_counters, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c[1]) return flagged_error(t, c[1], s);
  t->rows_ub = c[0];
  t->free_known = std::max(0, (int)c[2]);
  if (nrows_out) *nrows_out = c[0];
  if (out) {
    HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
    k_stats<<<nblocks(c[0], TB, 2048), TB, 0, s>>>(dev_view(t), c[0], t->d_stat);
    HIP_TRY(hipMemcpyAsync(out, t->d_stat, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return KV_OK;
}

// ---- the core's own kernels as the units on top launch them --------------------------------------------------------------
// every index entry back to EMPTY (import: the table is cleared)
void launch_fill_entries(kv_table* t, hipStream_t s) {
  k_fill_entries<<<nblocks((long long)t->cap + 1, TB, 8192), TB, 0, s>>>(t->entries, t->cap + 1);
}
void launch_clear_hints(kv_table* v, hipStream_t s) {
  k_clear_hints<<<nblocks((long long)v->cap + 1, TB, 8192), TB, 0, s>>>(v->entries, v->cap + 1);
}
// (every row in use: behind captured calls rows_ub may lag the device — ensure_capacity — so there the whole slab is cleared)
void launch_clear_stamps(kv_table* v, hipStream_t s) {
  const unsigned long long nrows = v->captured_calls ? v->rows_cap : v->rows_ub;
  k_clear_stamps<<<nblocks((long long)nrows, TB, 4096), TB, 0, s>>>(dev_view(v), (unsigned)nrows);
}
// kv_attach_slot (both locks held, any running epoch of either table ended): a pair of single-chunk tables gets its mirrors
// filled with the hints
void launch_link_hints(kv_table* v, kv_table* sl, unsigned nrows, hipStream_t s) {
  const bool mir = v->chunks.size() == 1 && sl->chunks.size() == 1 && !v->track_delta && !sl->track_delta && mirror_pair(v, sl, s);
  if (nrows <= 1) return;
  unsigned epoch = 0u;   // (the copies' stamp: not looked at without mirrors)
  if (mir) { std::lock_guard<std::mutex> l(v->pair_var->mu); epoch = v->pair_var->epoch.epoch16(); }
  k_link_hints<<<nblocks(nrows, TB, 8192), TB, 0, s>>>(dev_view(v), dev_view(sl), nrows, epoch, mir ? 1 : 0);
}

// the templated launchers, for the arguments the units on top use (kv_host.h)
template void launch_tile<false>(kv_table*, const WsDev&, const void*, const int*, long long, hipStream_t, int, const MultiDesc*, int, unsigned);
template void launch_tile<true>(kv_table*, const WsDev&, const void*, const int*, long long, hipStream_t, int, const MultiDesc*, int, unsigned);
template void launch_part_keys<MODE_LOOKUP>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int);
template void launch_part_keys<MODE_APPLYIDX>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int);
template void launch_part_keys<MODE_UNIQUE>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int);
template void launch_part_keys<MODE_SCATTER>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int);
template void launch_part_keys<MODE_MARK>(const WsDev&, const PartArgs&, hipStream_t, const MultiDesc*, int);
template void index_pass<MODE_LOOKUP>(kv_table*, const WsDev&, const PartArgs&, const void*, const int*, long long, int, float*, hipStream_t, bool);
template void index_pass<MODE_APPLYIDX>(kv_table*, const WsDev&, const PartArgs&, const void*, const int*, long long, int, float*, hipStream_t, bool);
template void index_pass<MODE_UNIQUE>(kv_table*, const WsDev&, const PartArgs&, const void*, const int*, long long, int, float*, hipStream_t, bool);
}  // namespace kvhip_internal

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* kv_last_error(void) { return g_err.c_str(); }

int kv_create(int key_dtype, int value_dtype, int dim, int enter_threshold, int64_t capacity_hint,
              int device, kv_handle_t* out) {
  if (!out) return fail(KV_INVALID_ARGUMENT, "out is null");
  if (key_dtype != KV_DT_INT64 && key_dtype != KV_DT_INT32 && key_dtype != KV_DT_UINT64)
    return fail(KV_INVALID_ARGUMENT, "key_dtype %d: only int32/int64/uint64 (kv_variable_ops.cc:149-156)", key_dtype);
  if (value_dtype != KV_DT_FLOAT)
    return fail(KV_UNIMPLEMENTED, "value_dtype %d: only float has optimizer kernels (training_ops.cc:7232)", value_dtype);
  if (dim <= 0) return fail(KV_INVALID_ARGUMENT, "Inner dimension should be greater than zero.");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(KV_INVALID_ARGUMENT, "device %d out of range (%d GPUs)", device, ndev);
  DeviceGuard dg(device);
  kv_table* t = new kv_table();
  t->device = device;
  t->key_dtype = key_dtype;
  t->dim = dim;
  t->enter_threshold = (unsigned)(unsigned short)std::min<int>(enter_threshold, 65535);  // SaturateMaxFrequency
  unsigned long long hint = capacity_hint > 0 ? (unsigned long long)capacity_hint + 1 : 0;
  t->chunk_bits = std::max(16, std::min(30, ilog2(std::max<unsigned long long>(hint, 1))));
  hipStream_t s = nullptr;
  int rc = KV_OK;
  do {
    if (hipMalloc(&t->d_chunks, MAX_CHUNKS * sizeof(Chunk)) != hipSuccess ||
        hipMalloc(&t->d_counters, 8 * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&t->d_stat, 4 * sizeof(unsigned long long)) != hipSuccess) {
      rc = fail(KV_RESOURCE_EXHAUSTED, "hipMalloc of table header failed");
      break;
    }
    if (hipHostMalloc(&t->err_host, 4 * sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipEventCreateWithFlags(&t->last_done, hipEventDisableTiming) != hipSuccess) {
      rc = fail(KV_RESOURCE_EXHAUSTED, "table header: pinned word / event");
      break;
    }
    t->err_host[0] = t->err_host[1] = t->err_host[2] = t->err_host[3] = 0;
    t->uid = ++g_uid;
    unsigned init[8] = {1, 0, 0, 0, 0, 0, 0, 0};  // next_row = 1 (row 0 is the zero row)
    if (hipMemcpy(t->d_counters, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(KV_INTERNAL, "hipMemcpy failed");
      break;
    }
    if ((rc = add_chunk(t, s))) break;
    if ((rc = build_index(t, pow2ceil(std::max<unsigned long long>(2 * t->rows_cap, 1024)), 1, s))) break;
  } while (0);
  if (rc) { kv_destroy(t); return rc; }
  { std::lock_guard<std::mutex> l(g_tables_mu); g_tables.insert(t); }
  *out = t;
  return KV_OK;
}

int kv_destroy(kv_handle_t t) {
  if (!t) return KV_OK;
  { std::lock_guard<std::mutex> l(g_tables_mu); g_tables.erase(t); }
  DeviceGuard dg(t->device);
  {   // slot mirrors: a var hands its dirty copies back before it goes — on the stream of its last op, where the lean apply
      // that wrote them was queued; a slot table's records go with it: nothing to write back
    std::lock_guard<std::mutex> l(t->mu);
    hipStream_t s = t->has_last ? t->last_stream : nullptr;
    mirror_visit(t, t->pair_var, s, LEAVE);
    mirror_visit(t, t->pair_slot, s, LEAVE_NO_FLUSH);
  }
  hipDeviceSynchronize();
  for (auto& c : t->chunks) { hipFree(c.rows); hipFree(c.meta); }
  hipFree(t->entries); hipFree(t->d_chunks); hipFree(t->d_counters); hipFree(t->d_stat); hipFree(t->free_rows);
  hipFree(t->init_table);
  hipFree(t->route_hist);
  for (auto e : t->ev) hipEventDestroy(e);
  Workspace& w = t->ws;
  hipFree(w.ent_key); hipFree(w.ent_a); hipFree(w.ent_b); hipFree(w.ent_base); hipFree(w.ent_rec); hipFree(w.toff); hipFree(w.slot_rank);
  hipFree(w.order); hipFree(w.coldlist); hipFree(w.hotlist); hipFree(w.litem); hipFree(w.items); hipFree(w.pmeta); hipFree(w.hpart);
  hipFree(w.mcount); hipFree(w.epart); hipFree(w.pos_ent);
  hipFree(w.ctr); hipFree(w.dbg); hipFree(w.scat_keys); hipFree(w.scat_sum); hipFree(w.seg_off); hipFree(w.seg_den); hipFree(w.pseg); hipFree(w.pscale);
  if (t->err_host) hipHostFree(t->err_host);
  if (t->cnt_host) hipHostFree(t->cnt_host);
  if (t->last_done) hipEventDestroy(t->last_done);
  delete t;
  return KV_OK;
}

int kv_reserve(kv_handle_t t, int64_t capacity) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = settle_pending(t))) return rc;
  unsigned long long save = t->rows_ub, save_idx = t->idx_ub;
  long long extra = capacity + 1 - (long long)t->rows_ub;
  if (extra <= 0) return KV_OK;
  rc = ensure_capacity(t, extra, nullptr);
  t->rows_ub = std::min(save, t->rows_ub);  // reserve does not consume the bounds
  t->idx_ub = std::min(save_idx, t->idx_ub);
  return rc;
}

int kv_init_table(kv_handle_t t, const float* table, int64_t rows, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!table || rows <= 0) return fail(KV_INVALID_ARGUMENT, "random_initializer must be a non-empty [rows, dim] matrix");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  // "re-initialization ignored" once a table is set (random_init_table_.NumElements() > 0, kv_variable.h:188-193);
  // the zero row an import leaves in place of a missing init table is not one
  if (t->initialized && t->init_table && !t->init_placeholder) return KV_OK;
  if ((rc = settle_pending(t))) return rc;   // (a pending pass reads the placeholder the next line frees)
  if (t->init_table) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); hipFree(t->init_table); t->init_table = nullptr; }
  HIP_TRY(hipMalloc(&t->init_table, (size_t)rows * t->dim * sizeof(float)));
  HIP_TRY(hipMemcpyAsync(t->init_table, table, (size_t)rows * t->dim * sizeof(float),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  t->init_rows = rows;
  t->init_placeholder = false;
  t->initialized = true;
  return KV_OK;
}

int kv_is_initialized(kv_handle_t t, int* out) {
  int rc;
  if ((rc = check_table(t))) return rc;
  *out = t->initialized ? 1 : 0;
  return KV_OK;
}

int kv_set_clock_days(kv_handle_t t, int day) {
  int rc;
  if ((rc = check_table(t))) return rc;
  t->fixed_day = day;
  ++t->op_serial;   // what a timed delete would release depends on the day
  return KV_OK;
}
int kv_set_seed(kv_handle_t t, uint64_t seed) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = settle_pending(t))) return rc;   // rows a pending pass initialises follow the seed the lookup answered with
  t->seed = seed;
  return KV_OK;
}

int kv_set_deterministic(kv_handle_t t, int on) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = settle_pending(t))) return rc;
  if (on < 0 || on > 2) return fail(KV_INVALID_ARGUMENT, "kv_set_deterministic: on = %d (0, 1 or 2)", on);
  if (on == 2 && t->shard_refs.load() > 0)
    return fail(KV_UNIMPLEMENTED, "kv_set_deterministic(h, 2): the table serves a kv_shard (occurrence order is a single-table notion)");
  t->deterministic = on != 0;
  t->occurrence_order = on == 2;
  t->batch.drop();   // the index a lookup left was built by the other pipeline's rules
  return KV_OK;
}

int kv_set_fast_math(kv_handle_t t, int on) {
  int rc;
  if ((rc = check_table(t))) return rc;
  std::lock_guard<std::mutex> l(t->mu);
  t->fast_math = on != 0;
  return KV_OK;
}

int kv_get_stat(kv_handle_t t, int which, int64_t* value) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!value) return fail(KV_INVALID_ARGUMENT, "kv_get_stat: null value");
  std::lock_guard<std::mutex> l(t->mu);
  if (which == KV_STAT_MIRROR_APPLIES) { *value = t->stat_mirror_applies; return KV_OK; }
  if (which == KV_STAT_MIRROR_EPOCHS) {   // (of the pairs the table has been the var of)
    *value = t->stat_mirror_epochs;
    if (t->pair_var) { std::lock_guard<std::mutex> lp(t->pair_var->mu); *value = t->pair_var->epoch.ended(); }
    return KV_OK;
  }
  return fail(KV_INVALID_ARGUMENT, "kv_get_stat: unknown counter %d", which);
}

int kv_prepare_capture(kv_handle_t t, int64_t max_new_ids, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (max_new_ids < 0) return fail(KV_INVALID_ARGUMENT, "max_new_ids < 0");
  TableOp op(t, stream);
  hipStream_t s = op.s;
  if ((rc = enter_op(t, s))) return rc;
  mirror_ban(t, s);   // (a captured apply replays without host code: no slot mirrors for this table from here on)
  t->capture_prepared = true;   // (ensure_capacity: captured calls on this table are told from the others from here on)
  if ((rc = capture_stage_reserve(t->device))) return rc;   // (the descriptors of captured batched calls: kv_host.h)
  unsigned c[3];
  HIP_TRY(hipMemcpyAsync(c, t->d_counters, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c[1]) return flagged_error(t, c[1], s);
  const long long freed = std::max(0, (int)c[2]);
  t->rows_ub = c[0];
  t->free_known = freed;
  t->idx_ub = t->idx_base + (c[0] - t->bump_base) +
              (unsigned long long)std::max<long long>(0, (long long)t->pushes_since - (freed - t->free_base));
  // make room now (this may grow the table), then give the room back: the captured calls take it piece by piece
  const unsigned long long r0 = t->rows_ub, i0 = t->idx_ub;
  if ((rc = ensure_capacity(t, max_new_ids, s))) return rc;
  t->rows_ub = r0; t->idx_ub = i0;
  HIP_TRY(hipStreamSynchronize(s));
  return KV_OK;
}

int kv_profile_enable(kv_handle_t t, int max_launches) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  for (auto e : t->ev) hipEventDestroy(e);
  t->ev.clear();
  t->ev_kind.clear();
  t->ev_used = 0;
  t->prof = max_launches > 0;
  for (int i = 0; i < 2 * max_launches; ++i) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    t->ev.push_back(e);
  }
  t->ev_kind.assign((size_t)std::max(max_launches, 0), 0);
  return KV_OK;
}

int kv_profile_select(kv_handle_t t, unsigned kind_mask) {
  int rc;
  if ((rc = check_table(t))) return rc;
  std::lock_guard<std::mutex> l(t->mu);
  t->prof_mask = kind_mask;
  return KV_OK;
}

int kv_profile_sample(kv_handle_t t, int every) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (every < 1) return fail(KV_INVALID_ARGUMENT, "kv_profile_sample: every %d", every);
  std::lock_guard<std::mutex> l(t->mu);
  t->prof_every = every;
  for (unsigned& q : t->prof_seq) q = 0;
  return KV_OK;
}

int kv_profile_read(kv_handle_t t, double* ms_sum, int64_t* launches, int n_kinds) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  for (int k = 0; k < n_kinds; ++k) { ms_sum[k] = 0; launches[k] = 0; }
  for (size_t i = 0; i + 1 < t->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(t->ev[i + 1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
    const int k = t->ev_kind[i / 2];
    if (k < n_kinds) { ms_sum[k] += ms; launches[k] += 1; }
  }
  t->ev_used = 0;
  return KV_OK;
}

#ifdef KV_STAMPS
int kv_debug_read_stamps(kv_handle_t t, unsigned long long* out, int64_t nblocks_) {
  DeviceGuard dg(t->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, t->ws.dbg, (size_t)std::min<int64_t>(nblocks_, 16384) * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return KV_OK;
}
#endif

}  // extern "C"
