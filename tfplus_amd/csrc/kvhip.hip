// kvhip.hip — MI355X (gfx950) KvVariable: HBM hash table + row slab, lookup and fused
// sparse optimizer kernels, and the C ABI of include/kvhip.h.
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
#include <iterator>
#include <ctime>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <unordered_set>

#include "../../include/kvhip.h"

// the kernels of the instantiation units (one per optimizer, one for the sums) are reached through kv_launch.h
#include "kv_launch.h"
#include "kv_host.h"

using namespace kvhip_internal;

namespace {

#include "kv_device.h"
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
__global__ void k_fill_i64(long long* p, long long v, unsigned long long count) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (unsigned long long)gridDim.x * blockDim.x) p[i] = v;
}
// int64 list -> int32 list in place (one block: element i is read before any thread can overwrite
// it, because writes land at half the byte offset and the loop is barrier-stepped)
__global__ void k_narrow_keys(long long* keys, long long n) {
  int* out = reinterpret_cast<int*>(keys);
  for (long long base = 0; base < n; base += blockDim.x) {
    const long long i = base + threadIdx.x;
    const long long v = i < n ? keys[i] : 0;
    __syncthreads();
    if (i < n) out[i] = (int)v;
    __syncthreads();
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

template <typename IdT>
__global__ void k_get_meta(TableDev t, const IdT* ids, long long n, unsigned* fw, unsigned char* fl) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const unsigned r = table_find(t, load_id(ids, (size_t)i));
    fw[i] = r ? *freq_ptr(t, r) : 0u;
    fl[i] = r ? (unsigned char)(*flags_ptr(t, r) | 0x80u) : 0;
  }
}

// GetCount kv_variable.h:503-524 (absent -> 0, else the low 16 bits) and GetTimeStamp :526-561
// (absent -> today, else the high 16 bits = day stamp of the last training lookup)
template <typename IdT>
__global__ void k_get_count_ts(TableDev t, const IdT* ids, long long n, int what, unsigned today, unsigned* out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const unsigned r = table_find(t, load_id(ids, (size_t)i));
    const unsigned fw = r ? *freq_ptr(t, r) : 0u;
    out[i] = what == 0 ? (r ? (fw & 0xFFFFu) : 0u) : (r ? (fw >> 16) : today);
  }
}

// releases one key: its index entry becomes a tombstone, its row goes to the free list
// (TableManager::DeleteKey table_manager.h:405-416: Evict + erase).  A key listed twice is
// released once (the second probe finds the tombstone).
__device__ __forceinline__ bool release_key(const TableDev& t, long long key, unsigned* free_rows) {
  Entry* slot;
  if (key == EMPTY_KEY) {
    slot = &t.entries[t.mask + 1];
    if (load_entry(slot).key != 0) return false;
  } else {
    unsigned long long p = mix64((unsigned long long)key) & t.mask;
    for (;;) {
      slot = &t.entries[p];
      const Entry e = load_entry(slot);
      if (e.key == key) break;
      if (e.key == EMPTY_KEY) return false;
      p = (p + 1) & t.mask;
    }
  }
  const unsigned r = atomicExch(&slot->row, ROW_TOMB);   // duplicates of the key race here: one wins
  if (r == ROW_TOMB || r == 0u) return false;
  *flags_ptr(t, r) = (unsigned char)FLAG_FREE;
  free_rows[atomicAdd(&t.counters[2], 1u)] = r;
  return true;
}
template <typename IdT>
__global__ void k_delete(TableDev t, const IdT* ids, long long n, unsigned* free_rows, unsigned long long* cnt) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    if (release_key(t, load_id(ids, (size_t)i), free_rows)) atomicAdd(&cnt[0], 1ull);
}
// DeleteWithTimestamp kv_variable.h:757-789: keys whose day stamp is > 0 and at least `threshold`
// days old.  fill == 0 only counts; fill == 1 releases them and lists their keys.
__global__ void k_delete_by_time(TableDev t, unsigned nrows, unsigned today, unsigned threshold, int fill,
                                 unsigned* free_rows, unsigned long long* cnt, long long* out_keys) {
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    if (*flags_ptr(t, r) & FLAG_FREE) continue;
    const unsigned kt = *freq_ptr(t, r) >> 16;
    if (kt == 0 || (int)today - (int)kt < (int)threshold) continue;
    const long long key = *key_ptr(t, r);
    if (!fill) { atomicAdd(&cnt[0], 1ull); continue; }
    if (release_key(t, key, free_rows)) out_keys[atomicAdd(&cnt[0], 1ull)] = key;
  }
}

// ExportValues dynamic_save.hpp:47-195.  cnt[0..2] = rows, blacklist, freq.  fill != 0 writes.
__global__ void k_export(TableDev t, unsigned nrows, int first_n, int fill, unsigned long long* cnt,
                         long long* keys, float* values, long long* blacklist, long long* fkeys,
                         unsigned* fvals) {
  const int D = t.dim;
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    const unsigned fl = *flags_ptr(t, r);
    const unsigned fw = *freq_ptr(t, r);
    const long long key = *key_ptr(t, r);
    if (fl & FLAG_FREE) continue;
    if (fl & FLAG_BLACK) {
      if (first_n > 3) {
        unsigned long long p = atomicAdd(&cnt[1], 1ull);
        if (fill && blacklist) blacklist[p] = key;
      }
    } else if ((first_n <= 3 || (fw & 0xFFFFu) >= t.enter_threshold) && !(fl & FLAG_UNDER)) {
      unsigned long long p = atomicAdd(&cnt[0], 1ull);
      if (fill) {
        keys[p] = key;
        const float* row = row_ptr(t, r);
        for (int e = 0; e < D; ++e) values[p * D + e] = row[e];
      }
    }
    if (first_n > 4) {
      unsigned long long p = atomicAdd(&cnt[2], 1ull);
      if (fill && fkeys) { fkeys[p] = key; fvals[p] = fw; }
    }
  }
}

// DeltaExport dynamic_save.hpp:198-451 over the rows whose delta bytes are set (train list, plus the
// prediction list when first_n <= 3).  cnt[0] = update rows, [1] = blacklisted keys, [2] = all delta rows.
// Order per key as in :231-248: low frequency -> only in the frequency list; blacklisted -> black list
// (the caller hands the delete list as `black` when first_n <= 3, :345-351); else key + row.
__global__ void k_export_delta(TableDev t, unsigned nrows, int first_n, int fill, unsigned long long* cnt,
                               long long* keys, float* values, long long* black, long long* fkeys,
                               unsigned* fvals) {
  const int D = t.dim;
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    const RowMeta m = *meta_ptr(t, r);
    if (m.flags & FLAG_FREE) continue;
    if (!((m.delta & DELTA_TRAIN) || (first_n <= 3 && (m.delta & DELTA_PRED)))) continue;
    if (first_n > 4) {  // ExportFrequencyDelta kv_variable.h:937-957: the whole 32-bit word
      unsigned long long p = atomicAdd(&cnt[2], 1ull);
      if (fill && fkeys) { fkeys[p] = m.key; fvals[p] = m.freq; }
    }
    if ((m.freq & 0xFFFFu) < t.enter_threshold) continue;
    if (m.flags & FLAG_BLACK) {
      unsigned long long p = atomicAdd(&cnt[1], 1ull);
      if (fill && black) black[p] = m.key;
      continue;
    }
    unsigned long long p = atomicAdd(&cnt[0], 1ull);
    if (fill) {
      keys[p] = m.key;
      const float* row = row_ptr(t, r);
      for (int e = 0; e < D; ++e) values[p * D + e] = row[e];
    }
  }
}
// keys recorded by Delete: one that has a row again is a live member of the list (its row carries the
// byte from here on), one without stays a "deleted" member.  which: 0 train list, 1 prediction list
__global__ void k_delta_resolve(TableDev t, const long long* keys, long long n, int which, unsigned char* present) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const unsigned r = table_find(t, keys[i]);
    present[i] = r ? 1 : 0;
    if (r) meta_ptr(t, r)->delta |= (unsigned char)(which == 0 ? DELTA_TRAIN : DELTA_PRED);
  }
}
// end of an export (dynamic_save.hpp:179-192, 432-443).  mode 0 (training export): the train list moves
// to the prediction list (if kept) and empties; mode 1 (prediction export): the prediction list empties
__global__ void k_delta_clear(TableDev t, unsigned nrows, int mode, int keep_pred) {
  for (unsigned r = 1 + blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    RowMeta* m = meta_ptr(t, r);
    const unsigned d = m->delta;
    if (mode == 1) { if (d & DELTA_PRED) m->delta = (unsigned char)(d & ~DELTA_PRED); continue; }
    if (d & DELTA_TRAIN) m->delta = (unsigned char)((d & ~DELTA_TRAIN) | (keep_pred ? DELTA_PRED : 0u));
  }
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

// the device error flag was found set at a synchronous point: report once, then clear it so the table
// stays usable (the batch that raised it had no effect beyond rows it may have inserted)
int flagged_error(kv_table* t, unsigned code, hipStream_t s) {
  hipMemsetAsync(t->d_counters + 1, 0, sizeof(unsigned), s);
  hipStreamSynchronize(s);
  if (t->err_host) *reinterpret_cast<volatile unsigned*>(t->err_host) = 0u;
  t->batch_serial = 0;
  if (code == 4)
    return fail(KV_INVALID_ARGUMENT, "kv_apply_*_unique: the ids of an earlier call were NOT unique (an id was listed twice): that "
                                     "batch was not applied as the reference applies repeated ids; pass such batches to "
                                     "kv_apply_* (which sums repeated ids) instead");
  return fail(KV_INTERNAL, code == 2 ? "a hash partition received more than 65535 entries in one batch "
                                       "(key set crafted against the partition hash); that batch was not applied"
                                     : "row slab overflow detected on device");
}

// make room for `extra` more keys (worst case: every id of the batch is new).  rows_ub bounds the
// bump allocator, idx_ub the claimed index entries (a key inserted into a row taken from the free
// list claims a new entry while the deleted key's tombstone stays until the next rebuild).
int ensure_capacity(kv_table* t, long long extra, hipStream_t s) {
  unsigned long long need = t->rows_ub + (unsigned long long)extra;
  unsigned long long need_idx = t->idx_ub + (unsigned long long)extra;
  if (need > t->rows_cap || need_idx * 2 > t->cap) {
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
static int ws_sync(hipStream_t s) {
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
    t->batch_serial = 0;
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
  d.P = pick_partitions(n);
  d.pshift = 64 - ilog2(d.P);
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
                 int ids_kind = -1, const MultiDesc* md = nullptr, int ntab = 0, unsigned gx = 0) {
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
                   const MultiDesc* md = nullptr, int ntab = 0, bool order = false) {
  const int D = td.dim;
  const int q = (D % 4 == 0) ? D / 4 : 0;
  const bool vec = q > 0 && (q & (q - 1)) == 0 && q <= TB;
  const long long rows_per_block = vec ? TB / q : 1;
  constexpr int gcap = 8192;  // one 64-row step per wave at 1M rows: residency, not a loop, hides the hops
  const int grid = vec ? nblocks(m, q <= 64 ? TB : (int)rows_per_block, gcap) : nblocks(m * D, TB, 4096);
#define KV_GATHER(VQ)                                                                        \
  do {                                                                                       \
    if (md) k_gather_multi<VQ><<<dim3((unsigned)grid, (unsigned)ntab), TB, 0, s>>>(md);       \
    else if (order) k_gather<VQ, true><<<grid + ITEM_BLOCKS, TB, 0, s>>>(td, wd, op, m);      \
    else k_gather<VQ, false><<<grid, TB, 0, s>>>(td, wd, op, m);                              \
  } while (0)
  switch (vec ? q : 0) {
    case 1: KV_GATHER(1); break;
    case 2: KV_GATHER(2); break;
    case 4: KV_GATHER(4); break;
    case 8: KV_GATHER(8); break;
    case 16: KV_GATHER(16); break;
    case 32: KV_GATHER(32); break;
    case 64: KV_GATHER(64); break;
    case 128: KV_GATHER(128); break;
    case 256: KV_GATHER(256); break;
    default: KV_GATHER(0); break;
  }
#undef KV_GATHER
}

// partition pass.  multi (md != nullptr): wd carries the LARGEST ntiles / P of the batch of tables (LDS
// sizing, grid.x); instantiated for MODE_LOOKUP and MODE_APPLYIDX
template <int MODE>
void launch_part_keys(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0) {
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
                  const MultiDesc* md = nullptr, int ntab = 0) {
  const int grid = nblocks(n, TB, 4096) + ITEM_BLOCKS;   // ITEM_BLOCKS blocks in front build the item directory only
  if (md) k_order_multi<<<dim3((unsigned)grid, (unsigned)ntab), TB, 0, s>>>(md);
  else k_order<<<grid, TB, 0, s>>>(td, wd, n);
}
// ... and tables: one in occurrence-order mode takes the sorted-position pipeline for every op, like a dim the entry-list
// kernels do not serve (its sums are one chain per key there; the entry lists sum tile by tile)
bool fused_tab(const kv_table* t) { return fused_ok(t->dim) && !t->occurrence_order; }
bool pow2_rows(int D) { return (D & 3) == 0 && row_lanes(D) == D / 4; }
// tile pass: dedup, index probes / inserts, entries, tile-local order and (out != nullptr) the output rows
// md != nullptr: `ntab` tables in one launch (grid.y), arguments from the descriptor array; multi_rows: with rows
void launch_ltile(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, const int* counts, long long n, float* out,
                  hipStream_t s, int ids_kind = -1, const MultiDesc* md = nullptr, int ntab = 0, bool multi_rows = false) {
  if (ids_kind < 0) ids_kind = t->key_dtype == KV_DT_INT32 ? 1 : 0;
  const int grid = (int)wd.ntiles;
  const size_t sh = ltile_smem_bytes();
  const int det = det_mode(t);
  const int q = row_lanes(td.dim);
#define KV_LT2(IDT, VQ)                                                                                     \
  do {                                                                                                      \
    if (md && multi_rows) k_ltile_multi<IDT, VQ, true><<<dim3((unsigned)grid, (unsigned)ntab), TBT, sh, s>>>(md); \
    else if (md) k_ltile_multi<IDT, 1, false><<<dim3((unsigned)grid, (unsigned)ntab), TBT, sh, s>>>(md);     \
    else if (out) k_ltile<IDT, VQ, true><<<grid, TBT, sh, s>>>(td, wd, (const IDT*)ids, counts, n, det, out); \
    else k_ltile<IDT, 1, false><<<grid, TBT, sh, s>>>(td, wd, (const IDT*)ids, counts, n, det, nullptr);     \
  } while (0)
#define KV_LT(IDT)                                                              \
  do {                                                                          \
    switch (q) {                                                                \
      case 1: KV_LT2(IDT, 1); break;   case 2: KV_LT2(IDT, 2); break;           \
      case 4: KV_LT2(IDT, 4); break;   case 8: KV_LT2(IDT, 8); break;           \
      case 16: KV_LT2(IDT, 16); break; case 32: KV_LT2(IDT, 32); break;         \
      default: KV_LT2(IDT, 64); break;                                          \
    }                                                                           \
  } while (0)
  if (ids_kind == 2) KV_LT(IdCount);
  else if (ids_kind == 1) KV_LT(int);
  else KV_LT(long long);
#undef KV_LT
#undef KV_LT2
}
// the table-less tile pass of the sharded route (int64 ids): entries, mrow, every position's entry number
void launch_ltile_notable(kv_table* t, const TableDev& td, const WsDev& wd, const void* ids, long long n, hipStream_t s,
                          const int* counts, bool int32_ids) {
  const int det = det_mode(t);
  if (int32_ids) k_ltile<int, 1, false, true><<<(int)wd.ntiles, TBT, ltile_smem_bytes(), s>>>(td, wd, (const int*)ids, counts, n, det, nullptr);
  else k_ltile<long long, 1, false, true><<<(int)wd.ntiles, TBT, ltile_smem_bytes(), s>>>(td, wd, (const long long*)ids, counts, n, det, nullptr);
}
// ... of `ntab` sharded routes in one launch (wmax: the largest ntiles of the batch of tables)
void launch_ltile_multi_notable(const WsDev& wmax, int ntab, const MultiDesc* md, hipStream_t s) {
  k_ltile_multi_notable<<<dim3(wmax.ntiles, (unsigned)ntab), TBT, ltile_smem_bytes(), s>>>(md);
}
// the bookkeeping of a training lookup that no apply takes over (k_part2); md: `ntab` tables in one launch
void launch_part2(const WsDev& wd, const PartArgs& pa, hipStream_t s, const MultiDesc* md = nullptr, int ntab = 0) {
  if (md) k_part2_multi<<<dim3(wd.P, (unsigned)ntab), TBK, (size_t)wd.ntiles * 4 + 32, s>>>(md);
  else k_part2<<<(int)wd.P, TBK, (size_t)wd.ntiles * 4 + 32, s>>>(wd, pa);
}

// segmented fold over the sorted positions + fused update (k_apply_sorted), then the keys that cross chunk
// boundaries (k_apply_span).  pa.n = ids of the batch (multi: nmax = the largest table's batch)
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

// launches a lookup's pending partition pass (see kv_table::part_pending) on stream s
int flush_part(kv_table* t, hipStream_t s) {
  if (!t->part_pending) return KV_OK;
  t->part_pending = false;
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
// read only by it.  EVERY other op that enters either table first ends the epoch (mirror_end_epoch: flush the dirty
// copies, one kernel over the var's rows, then epoch + 1 — which invalidates every copy at once), so it sees, and may
// change, the authoritative records; the keys' next lean apply finds no valid mirror, takes the general path once and
// leaves a fresh clean copy (finish_key).  An op that keeps the epoch says so where it enters the table (enter_op,
// hand_over, MultiLock::enter), with the role(s) it keeps the table in; KEEP_NONE, the default, ends it.  The
// keepers: the training / inference lookups on the var (they touch var records and rows only), the GroupAdam and Adagrad
// applies on (var, slot), single and batched, and the ops that only borrow a table's workspace.  A role, not a table, is
// kept: a var entered as KEEP_VAR that is also another var's slot table still ends that other pair's epoch.
// held: the table of the pair whose lock the caller holds (the var itself, or its slot table): the views come from there
void mirror_end_epoch(kv_table* var, hipStream_t s, const kv_table* held) {
  if (!var->mirror_slot) return;
  var->stat_mirror_epochs.fetch_add(1);
  const TableDev& tv = held->mview_var;
  const long long rows = (long long)tv.max_rows + 1;
  if (var->mirror_dirty.exchange(false))
    k_flush_mirrors<<<nblocks(rows, TB, 8192), TB, 0, s>>>(tv, held->mview_slot, var->mirror_epoch.load() & 0xFFFFu);
  if ((var->mirror_epoch.fetch_add(1) + 1u) > 0xFFFFu) {
    k_clear_mirrors<<<nblocks(rows, TB, 8192), TB, 0, s>>>(tv);
    var->mirror_epoch.store(1);
  }
}
void mirror_unpair(kv_table* var, hipStream_t s, const kv_table* held) {
  if (!var->mirror_slot) return;
  mirror_end_epoch(var, s, held);
  var->mirror_slot->mirror_var = nullptr;
  var->mirror_slot = nullptr;
}
// (both locks held)
static void mirror_snapshot(kv_table* v, kv_table* sl) {
  v->mview_var = sl->mview_var = dev_view(v);
  v->mview_slot = sl->mview_slot = dev_view(sl);
}
// the entry hook of hand_over / join_side.  Under a stream capture the flush would be RECORDED, not run, and a replay would
// carry the epoch of its capture: a table that is captured gives up its mirrors beforehand (kv_prepare_capture ->
// mirror_ban); an op that would have to end an epoch inside a capture is refused.
int mirror_on_entry(kv_table* t, hipStream_t s, unsigned keep) {
  if (!t->mirror_var && !t->mirror_slot) return KV_OK;
  const bool end_slot = t->mirror_var && !(keep & KEEP_SLOT), end_var = t->mirror_slot && !(keep & KEEP_VAR);
  if ((end_slot || end_var) && stream_is_capturing(s))
    return fail(KV_FAILED_PRECONDITION, "this table is half of a (var, slot) pair whose optimizer applies keep the slot records' "
                                        "frequency words in the var's rows between ops; call kv_prepare_capture on it (outside the "
                                        "capture) before capturing ops on it");
  if (end_slot) mirror_end_epoch(t->mirror_var, s, t);   // t is a slot table: its records are about to be read or written
  if (end_var) mirror_end_epoch(t, s, t);                // t is a var: its rows may be released, moved or read back
  return KV_OK;
}
// kv_prepare_capture: the table's ops are about to be captured and replayed — no host code runs at a replay, so nothing
// could flush or re-validate a mirror: the pair is dissolved now (the dirty copies go back) and never forms again
void mirror_ban(kv_table* t, hipStream_t s) {
  if (t->mirror_slot) mirror_unpair(t, s, t);
  if (t->mirror_var) mirror_unpair(t->mirror_var, s, t);
  t->mirror_banned = true;
}
// (var, slot) become a mirror pair — or stay / become unpaired when the slot table already serves another var
bool mirror_pair(kv_table* v, kv_table* sl, hipStream_t s) {
  if (sl->mirror_shared || v->mirror_banned || sl->mirror_banned) return false;
  if (v->mirror_slot == sl && sl->mirror_var == v) return true;
  if (sl->mirror_var && sl->mirror_var != v) {   // a second var on one slot table: no mirrors for it at all
    mirror_unpair(sl->mirror_var, s, sl);
    sl->mirror_shared = true;
    return false;
  }
  if (v->mirror_slot && v->mirror_slot != sl) mirror_unpair(v, s, v);
  v->mirror_slot = sl;
  sl->mirror_var = v;
  mirror_snapshot(v, sl);
  mirror_end_epoch(v, s, v);   // a fresh epoch: whatever bytes the rows' mirror units hold are void
  return true;
}

// Does this apply of (v, s0) work on the var rows' slot mirrors?  lean: the launch is k_papply / k_uapply (their lean
// update is the only code that reads or writes a mirror).  Otherwise the apply reads and writes the slot table's own
// records: the epoch ends first (the caller entered the var as KEEP_VAR and the slot as KEEP_SLOT, so nothing has ended it yet).
template <int OPT>
static int mirror_decide(kv_table* v, kv_table* s0, PartArgs& pa, bool lean, hipStream_t s) {
  pa.use_mirror = 0; pa.mirror_epoch = 0u;
  // (a captured apply of a pair that still has mirrors: their flush would be recorded, not run — see mirror_on_entry)
  if ((v->mirror_slot || s0->mirror_var) && stream_is_capturing(s))
    return fail(KV_FAILED_PRECONDITION, "optimizer apply under stream capture on a (var, slot) pair with live slot mirrors: call "
                                        "kv_prepare_capture on both tables (outside the capture) first");
  const bool eligible = !two_slots(OPT) && lean && pa.use_hints != 0 && pa.tv.single != 0u && pa.ts0.single != 0u &&
                        !v->track_delta && !s0->track_delta && !stream_is_capturing(s) && mirror_pair(v, s0, s);
  if (eligible) {
    pa.use_mirror = 1;
    pa.mirror_epoch = v->mirror_epoch.load() & 0xFFFFu;
    mirror_snapshot(v, s0);   // what this apply's dirty copies name is inside these views
    v->mirror_dirty.store(true);
    ++v->stat_mirror_applies;
  } else {
    if (v->mirror_slot) mirror_end_epoch(v, s, v);
    if (s0->mirror_var && s0->mirror_var != v) mirror_end_epoch(s0->mirror_var, s, s0);
  }
  return KV_OK;
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
  if (t->part_pending && settle) {   // (an apply that takes the batch over runs it itself, behind the stream hand-over below)
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
  if (t->part_pending) {
    if ((rc = hop_behind_last(t, s)) || (rc = flush_part(t, s))) return rc;
  }
  // An epoch of slot mirrors that ends here flushes copies the last lean apply wrote — on the stream of t's last op (an apply
  // enters both tables; anything later on t has ended the epoch already): the flush must run behind it.  (A flush that
  // overtook the apply would miss its copies, and the epoch number that ends with it would orphan them for good.)
  if ((t->mirror_var || t->mirror_slot) && (rc = hop_behind_last(t, s))) return rc;
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
                int ids_kind, float* out, hipStream_t s, bool file_order = true) {
  t->fused_index = false;
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

// partitions of an entry-list index pass over n ids (wd.P, wd.pshift; remembered in t->index_P)
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
    t->index_P = wd.P;
  }
}

// The training lookup on the entry-list kernels (kv_fused.h): the tile pass with the output rows; then the lookup's
// bookkeeping (k_part2) — or, defer_part: it stays PENDING for the optimizer apply of this batch (k_papply completes it
// in the same pass as the update) or for whatever op the table sees next (flush_part)
int fused_lookup_pass(kv_table* t, WsDev& wd, const PartArgs& pa, const void* ids, const int* counts, long long n,
                      int ids_kind, float* out, hipStream_t s, bool defer_part) {
  t->fused_index = true;
  choose_partitions(t, wd, n);
  {
    ProfScope ps(t, KV_PROF_LOOKUP_TILE, s);
    launch_ltile(t, pa.tv, wd, ids, counts, n, out, s, ids_kind);
  }
  if (defer_part) {   // the rows are out: the partition pass waits for the table's next op
    std::memcpy(t->pend_wd, &wd, sizeof wd);
    std::memcpy(t->pend_pa, &pa, sizeof pa);
    t->part_pending = true;
    return KV_OK;
  }
  ProfScope ps(t, KV_PROF_LOOKUP_PART, s);
  launch_part2(wd, pa, s);
  return KV_OK;
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

// Every live table: a stream the LIBRARY owns (a communicator's) is retired from the tables that last ran on it before it
// is destroyed — hand_over would otherwise record an event on a dead stream at the table's next op (found in round 6:
// bench.py's sharded_world1 sub-record destroys its communicator, the next lookup on another stream crashed in
// hipEventRecord).  A stream the CALLER owns must outlive the table's next op, or the caller synchronises it first and
// calls kv_forget_stream.
std::mutex g_tables_mu;
std::unordered_set<kv_table*> g_tables;
void retire_stream(hipStream_t dead) {   // `dead` is drained (the caller synchronised it)
  std::lock_guard<std::mutex> l(g_tables_mu);
  for (kv_table* t : g_tables) {
    std::lock_guard<std::mutex> lt(t->mu);
    if (t->has_last && t->last_stream == dead) { t->has_last = false; t->last_stream = nullptr; }
  }
}

std::atomic<uint64_t> g_serial{0};   // batch tokens
std::atomic<uint64_t> g_uid{0};

}  // namespace kvhip_internal

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
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
  {   // slot mirrors: a var hands its dirty copies back before it goes; a slot table takes its var's pairing with it
    DeviceGuard dgm(t->device);
    if (t->mirror_slot) mirror_unpair(t, nullptr, t);
    if (t->mirror_var) { t->mirror_var->mirror_dirty.store(false); t->mirror_var->mirror_slot = nullptr; t->mirror_var = nullptr; }
  }
  DeviceGuard dg(t->device);
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
  hipFree(w.ctr); hipFree(w.dbg); hipFree(w.scat_keys); hipFree(w.scat_sum); hipFree(w.seg_off);
  if (t->err_host) hipHostFree(t->err_host);
  if (t->cnt_host) hipHostFree(t->cnt_host);
  if (t->last_done) hipEventDestroy(t->last_done);
  delete t;
  return KV_OK;
}

// A lookup's deferred passes hold a snapshot of the table's arrays (pend_pa): whatever moves or frees those arrays, or
// changes what the passes would compute (seed, deterministic order), first lets them run — on the stream of the
// table's last op — and waits for them.
static int settle_pending(kv_table* t) {
  if (!t->part_pending) return KV_OK;
  hipStream_t s = t->has_last ? t->last_stream : nullptr;
  int rc;
  if ((rc = join_side(t, s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
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

static int stats(kv_handle_t t, hipStream_t s, unsigned long long out[2], unsigned* nrows_out) {
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

int kv_size(kv_handle_t t, int64_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  unsigned long long o[2];
  if ((rc = stats(t, (hipStream_t)stream, o, nullptr))) return rc;
  *out = (int64_t)o[0];
  return KV_OK;
}
int kv_sum_freq(kv_handle_t t, int64_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  unsigned long long o[2];
  if ((rc = stats(t, (hipStream_t)stream, o, nullptr))) return rc;
  *out = (int64_t)o[1];
  return KV_OK;
}
int kv_map_size(kv_handle_t t, int64_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  unsigned nrows = 1;
  if ((rc = stats(t, (hipStream_t)stream, nullptr, &nrows))) return rc;
  *out = (int64_t)nrows - 1 - t->free_known;
  return KV_OK;
}

int kv_get_meta(kv_handle_t t, const int64_t* ids, int64_t n, uint32_t* fw, uint8_t* fl, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n <= 0) return KV_OK;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = join_side(t, (hipStream_t)stream))) return rc;
  k_get_meta<long long><<<nblocks(n, TB), TB, 0, (hipStream_t)stream>>>(dev_view(t), (const long long*)ids, n, fw, fl);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

}  // extern "C"

namespace __attribute__((visibility("hidden"))) kvhip_internal {
// seg_cap + self: the (id, count) records of a sharded owner lookup, in fixed-capacity segments (kv_shard_lookup_serve)
int gather_or_insert_impl(kv_handle_t t, const void* ids, const int32_t* counts, int64_t n, float* out,
                          kv_stream_t stream, int pairs, kv_batch_token_t* token, unsigned seg_cap,
                          const SelfSegment* self) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n == 0) return KV_OK;  // kv_variable_ops.cc:530-532
  if (n < 0 || n > (1ll << 30)) return fail(KV_INVALID_ARGUMENT, "indices: bad length %lld", (long long)n);
  if (!ids || !out) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = enter_op(t, s, KEEP_VAR))) return rc;   // a training lookup touches the var's rows and records, never a slot record or a mirror
  // any batch length: chunks of 2^21 ids are looked up one after another (same semantics as one
  // pass: the frequency adds saturate identically and rows are inserted by the first chunk)
  // the entry-list pipeline indexes a batch of up to FUSED_MAX_N ids in one pass; the sorted-position one 2^21
  const long long CHK = fused_tab(t) ? FUSED_MAX_N : (1ll << 21);
  const size_t idsz = pairs ? 16 : (t->key_dtype == KV_DT_INT32 ? 4 : 8);
  t->batch_serial = 0;
  for (long long off = 0; off < n; off += CHK) {
    const long long m = std::min(CHK, (long long)n - off);
    const void* idp = (const char*)ids + (size_t)off * idsz;
    const int32_t* cp = counts ? counts + off : nullptr;
    float* op = out + (size_t)off * t->dim;
    if ((rc = ensure_capacity(t, m, s))) return rc;
    if ((rc = ensure_workspace(t, m, false, s))) return rc;
    const TableDev td = dev_view(t);
    WsDev wd = ws_view(t, m, self);
    wd.seg_cap = seg_cap;
    PartArgs pa{};
    pa.tv = td; pa.ts0 = td; pa.ts1 = td;
    pa.day = today(t);
    pa.det = det_mode(t);
    pa.n = m;
    const bool defer_part = token != nullptr && n <= CHK;   // a token is asked for: an apply of this batch follows
    if (fused_tab(t)) { if ((rc = fused_lookup_pass(t, wd, pa, idp, cp, m, pairs ? 2 : -1, op, s, defer_part))) return rc; }
    else index_pass<MODE_LOOKUP>(t, wd, pa, idp, cp, m, pairs ? 2 : -1, op, s, token != nullptr && n <= CHK);
  }
  HIP_TRY(hipGetLastError());
  if (token && n <= CHK) {   // the workspace now holds the index of exactly this batch, positions filed
    t->batch_serial = ++g_serial;
    t->batch_n = n;
    if (token) *token = t->batch_serial;
  }
  return KV_OK;
}
}  // namespace kvhip_internal

extern "C" {

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
  if (combiner < KV_COMBINER_SUM || combiner > KV_COMBINER_SQRTN)
    return fail(KV_INVALID_ARGUMENT, "combiner must be one of 'mean', 'sqrtn' or 'sum'");  // embedding_ops.py:345
  if (segment_dtype != KV_DT_INT32 && segment_dtype != KV_DT_INT64)
    return fail(KV_INVALID_ARGUMENT, "segment ids must be int32 or int64");
  const bool fused = fused_tab(t);   // (dim is fixed at creation: readable without the lock)
  if (n < 0 || n > (fused ? FUSED_MAX_N : (1ll << 21)))
    return fail(KV_INVALID_ARGUMENT, "sp_ids: %lld values (at most 2^%d per call)", (long long)n, fused ? 23 : 21);
  if (num_segments < 0 || num_segments > (1ll << 31) - 2) return fail(KV_INVALID_ARGUMENT, "bad num_segments");
  if (num_segments == 0) return KV_OK;
  if (!out || (n > 0 && (!ids || !segment_ids))) return fail(KV_INVALID_ARGUMENT, "ids / segment ids / output pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = enter_op(t, s, KEEP_VAR))) return rc;   // the table's own rows and records only
  const int D = t->dim;
  if (n == 0) {  // every segment is empty
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_segments * D * sizeof(float), s));
    return KV_OK;
  }
  if ((rc = ensure_capacity(t, n, s))) return rc;
  if ((rc = ensure_workspace(t, n, false, s))) return rc;
  Workspace& ws = t->ws;
  if (ws.seg_cap < num_segments) {
    if ((rc = ws_sync(s))) return rc;
    const long long want = std::max<long long>(num_segments, ws.seg_cap * 2);
    ws.seg_cap = 0;
    if ((rc = regrow(&ws.seg_off, (size_t)(want + 1)))) return rc;
    ws.seg_cap = want;
  }
  if (fused && ws.pos_cap < n) {   // every position's entry in its tile (k_ltile files it for the combiner)
    if ((rc = ws_sync(s))) return rc;
    ws.pos_cap = 0;
    if ((rc = regrow(&ws.pos_ent, (size_t)std::max<long long>(n, ws.cap_n)))) return rc;
    ws.pos_cap = std::max<long long>(n, ws.cap_n);
  }
  const TableDev td = dev_view(t);
  WsDev wd = ws_view(t, n);
  PartArgs pa{};
  pa.tv = td; pa.ts0 = td; pa.ts1 = td;
  pa.day = today(t);
  pa.count_once = count_occurrences ? 0 : 1;
  pa.det = det_mode(t);
  pa.n = n;
  t->batch_serial = 0;
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
  if (segment_dtype == KV_DT_INT32)
    k_seg_offsets<int><<<nblocks(n + 1, TB, 2048), TB, 0, s>>>((const int*)segment_ids, n, num_segments, ws.seg_off);
  else
    k_seg_offsets<long long><<<nblocks(n + 1, TB, 2048), TB, 0, s>>>((const long long*)segment_ids, n, num_segments, ws.seg_off);
  if (fused) {
    const int ql = row_lanes(D);
    const int grid = nblocks(num_segments * ql, TB, 8192);
#define KV_SCE(VQ) k_seg_combine_e<VQ><<<grid, TB, 0, s>>>(td, ws.pos_ent, wd.ent_b, wd.ent_key, ws.seg_off, weights, num_segments, combiner, out)
    switch (ql) {
      case 1: KV_SCE(1); break;   case 2: KV_SCE(2); break;   case 4: KV_SCE(4); break;   case 8: KV_SCE(8); break;
      case 16: KV_SCE(16); break; case 32: KV_SCE(32); break; default: KV_SCE(64); break;
    }
#undef KV_SCE
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  const int q = (D % 4 == 0) ? D / 4 : 0;
  const bool vec = q > 0 && (q & (q - 1)) == 0 && q <= 64;
  const int grid = nblocks(num_segments * (vec ? q : 1), TB, 8192);
  switch (vec ? q : 0) {
    case 1: k_seg_combine<1><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 2: k_seg_combine<2><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 4: k_seg_combine<4><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 8: k_seg_combine<8><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 16: k_seg_combine<16><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 32: k_seg_combine<32><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    case 64: k_seg_combine<64><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
    default: k_seg_combine<0><<<grid, TB, 0, s>>>(td, wd, ws.seg_off, weights, num_segments, combiner, out); break;
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_gather_or_zeros(kv_handle_t t, const void* ids, int64_t n, float* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!t->initialized)   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  if (n == 0) return KV_OK;
  if (n < 0 || !ids || !out) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  // a read: behind the table's last op on whatever stream, no serial bump.  It reads rows and flags of THIS table: as a var
  // it leaves the mirrors alone.  (hand_over, not enter_op: unlike kv_batch_gather_or_zeros this op does not report the
  // deferred error of the table's last batch — the next op that does will)
  if ((rc = hand_over(t, s, KEEP_VAR, true, false))) return rc;
  const TableDev td = dev_view(t);
  const int q = t->dim / 4;
  const bool wave_shaped = (t->dim & 3) == 0 && q >= 1 && q <= 64 && (q & (q - 1)) == 0;
  const int gw = nblocks(n, TB, 8192);  // a 64-id step per wave at 1 M ids: residency hides the hops
#define KV_GOZ(IDT, VQ) k_gather_or_zeros_w<IDT, VQ><<<gw, TB, 0, s>>>(td, (const IDT*)ids, out, n)
#define KV_GOZ_ALL(IDT)                                                                        \
  switch (q) {                                                                                 \
    case 1: KV_GOZ(IDT, 1); break;   case 2: KV_GOZ(IDT, 2); break;   case 4: KV_GOZ(IDT, 4); break;    \
    case 8: KV_GOZ(IDT, 8); break;   case 16: KV_GOZ(IDT, 16); break; case 32: KV_GOZ(IDT, 32); break;  \
    default: KV_GOZ(IDT, 64); break;                                                           \
  }
  if (wave_shaped) {
    if (t->key_dtype == KV_DT_INT32) { KV_GOZ_ALL(int) } else { KV_GOZ_ALL(long long) }
  } else if (t->key_dtype == KV_DT_INT32) {
    k_gather_or_zeros<int><<<nblocks(n, TB / 8, 8192), TB, 0, s>>>(td, (const int*)ids, out, n);
  } else {
    k_gather_or_zeros<long long><<<nblocks(n, TB / 8, 8192), TB, 0, s>>>(td, (const long long*)ids, out, n);
  }
#undef KV_GOZ_ALL
#undef KV_GOZ
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

}  // extern "C"
// descriptor staging for the batched launches: one pinned host buffer + device buffer per device
// and descriptor kind; the next upload waits until the previous launch has consumed the buffer
namespace __attribute__((visibility("hidden"))) kvhip_internal {
BatchStage g_stage[64][2];   // [device][0 = inference gather, 1 = training ops]

// returns with st.mu HELD (released by StageRelease after `consumed` is recorded on the stream)
int stage_acquire(BatchStage& st, size_t bytes, StageSlot** out) {
  st.mu.lock();
  StageSlot& sl = st.slot[st.cursor++ & 3u];
  if (sl.consumed && hipEventSynchronize(sl.consumed) != hipSuccess) {
    st.mu.unlock();
    return fail(KV_INTERNAL, "descriptor staging: event sync failed");
  }
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
}  // namespace kvhip_internal

extern "C" {

int kv_batch_gather_or_zeros(int num_tables, const kv_handle_t* tables, const void* const* ids,
                             const int64_t* ns, float* const* outs, kv_stream_t stream) {
  int rc;
  if ((rc = check_same_shape(num_tables, tables, "tables"))) return rc;  // Attr("N: int >= 1")
  if (!ids || !ns || !outs) return fail(KV_INVALID_ARGUMENT, "null argument array");
  for (int i = 0; i < num_tables; ++i) {
    if (ns[i] < 0 || (ns[i] > 0 && (!ids[i] || !outs[i]))) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
    if (!tables[i]->initialized)   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
      return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  }
  const int device = tables[0]->device;
  DeviceGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  MultiLock lock(std::vector<kv_table*>(tables, tables + num_tables));
  // every table is read on the op's stream: behind whatever its own last op queued on another stream (an optimizer
  // apply that has not finished), and its next op behind this read (rows and flags only: as vars they keep their mirrors)
  for (kv_table* tb : lock.ts)
    if ((rc = enter_op(tb, s, KEEP_VAR, true, false))) return rc;
  BatchStage& st = g_stage[device][0];
  StageSlot* sl = nullptr;
  if ((rc = stage_acquire(st, (size_t)num_tables * sizeof(BatchGatherDesc), &sl))) return rc;
  StageRelease rel{st, sl, s};
  BatchGatherDesc* hd = reinterpret_cast<BatchGatherDesc*>(sl->host);
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
  HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, (size_t)num_tables * sizeof(BatchGatherDesc), hipMemcpyHostToDevice, s));
  rel.launched = true;
  dim3 grid((unsigned)nblocks(nmax, TB / 8, 2048), (unsigned)num_tables);
  k_batch_gather_or_zeros<<<grid, TB, 0, s>>>(reinterpret_cast<const BatchGatherDesc*>(sl->dev));
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// ---- many tables, one launch per pipeline stage (26-feature CTR step: 5 launches, not 130) ------
// All tables: same device, same dim, same key dtype; each batch <= 2^21 ids.
static int multi_common(int num_tables, const kv_handle_t* tables, const void* const* ids, const int64_t* ns) {
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
    if (!tables[i]->initialized)
      return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
    for (int j = 0; j < i; ++j)
      if (tables[j] == tables[i]) return fail(KV_INVALID_ARGUMENT, "batched op: table listed twice");
  }
  return KV_OK;
}

}  // extern "C"

namespace __attribute__((visibility("hidden"))) kvhip_internal {
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
    tables[i]->batch_serial = 0;
    if (ns[i] > 0 && !outs[i]) return fail(KV_INVALID_ARGUMENT, "output pointer is null");
    if ((rc = ensure_capacity(tables[i], ns[i], s))) return rc;
    if ((rc = ensure_workspace(tables[i], std::max<long long>(ns[i], 1), false, s))) return rc;
    nmax = std::max<long long>(nmax, ns[i]);
  }
  if (nmax == 0) return KV_OK;
  BatchStage& st = g_stage[device][1];
  StageSlot* sl = nullptr;
  if ((rc = stage_acquire(st, (size_t)num_tables * sizeof(MultiDesc), &sl))) return rc;
  StageRelease rel{st, sl, s};
  MultiDesc* hd = reinterpret_cast<MultiDesc*>(sl->host);
  WsDev wmax{};
  for (int i = 0; i < num_tables; ++i) {
    MultiDesc& d = hd[i];
    std::memset(&d, 0, sizeof d);
    d.w = ws_view(tables[i], std::max<long long>(ns[i], 1), selfs ? &selfs[i] : nullptr);
    if (seg_caps) d.w.seg_cap = seg_caps[i];
    if (fused_tab(tables[i])) { d.w.P = fused_default_P(std::max<long long>(ns[i], 1)); d.w.pshift = 64 - ilog2(d.w.P); }
    d.a.tv = dev_view(tables[i]); d.a.ts0 = d.a.tv; d.a.ts1 = d.a.tv;
    d.a.day = today(tables[i]);
    d.a.det = tables[i]->deterministic ? 1 : 0;
    d.a.n = ns[i];
    d.ids = ids[i];
    d.counts = counts ? counts[i] : nullptr;
    d.out = outs[i];
    d.n = ns[i];
    if (ns[i] == 0) d.w.ntiles = 0;
    wmax.ntiles = std::max(wmax.ntiles, d.w.ntiles);
    wmax.P = std::max(wmax.P, d.w.P);
  }
  HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, (size_t)num_tables * sizeof(MultiDesc), hipMemcpyHostToDevice, s));
  rel.launched = true;
  const MultiDesc* md = reinterpret_cast<const MultiDesc*>(sl->dev);
  kv_table* t0 = tables[0];
  if (fused_tab(t0)) {
    for (int i = 0; i < num_tables; ++i) tables[i]->fused_index = true;
    launch_ltile(t0, hd[0].a.tv, wmax, nullptr, nullptr, nmax, nullptr, s, ids_kind, md, num_tables, true);
    // tokens asked for: an optimizer apply of these batches follows — every table's partition pass stays pending
    // (kv_multi_apply_*_tok completes it inside k_papply_multi; any other op on a table settles that table first)
    const bool defer = tokens != nullptr;
    if (!defer) launch_part2(wmax, hd[0].a, s, md, num_tables);
    if (tokens)   // every table's workspace now holds the index of exactly its batch (kv_multi_apply_*_tok takes it over)
      for (int i = 0; i < num_tables; ++i) {
        if (ns[i] <= 0) continue;
        tables[i]->batch_serial = ++g_serial;
        tables[i]->batch_n = ns[i];
        tables[i]->index_P = hd[i].w.P;
        tokens[i] = tables[i]->batch_serial;
        if (defer) {
          std::memcpy(tables[i]->pend_wd, &hd[i].w, sizeof(WsDev));
          std::memcpy(tables[i]->pend_pa, &hd[i].a, sizeof(PartArgs));
          tables[i]->part_pending = true;
        }
      }
  } else {
    for (int i = 0; i < num_tables; ++i) tables[i]->fused_index = false;
    launch_tile<false>(t0, wmax, nullptr, nullptr, nmax, s, -1, md, num_tables, wmax.ntiles);
    launch_part_keys<MODE_LOOKUP>(wmax, hd[0].a, s, md, num_tables);
    launch_gather(hd[0].a.tv, wmax, nullptr, nmax, s, md, num_tables);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}
}  // namespace kvhip_internal

extern "C" {
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

}  // extern "C"

// The slot table whose rows the var's index entries remember (Entry::hint): the first slot-0 table an
// optimizer uses with the var, or the one kv_attach_slot names.  Hints of a table that was cleared since
// (import) mean nothing any more and are forgotten; another table simply goes without hints.
static bool claim_slot(kv_table* v, kv_table* sl, hipStream_t s) {
  if (v->slot_uid == sl->uid && v->slot_gen == sl->gen) return true;
  if (v->slot_uid != 0 && v->slot_uid != sl->uid) return false;
  if (v->slot_uid == sl->uid)   // same table, cleared since
    k_clear_hints<<<nblocks((long long)v->cap + 1, TB, 8192), TB, 0, s>>>(v->entries, v->cap + 1);
  v->slot_uid = sl->uid;
  v->slot_gen = sl->gen;
  return true;
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
      if (!sl[i]->initialized) return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: optimizer slot");
      if (sl[i]->dim != slot_mult * D || sl[i]->device != vars[0]->device || sl[i]->key_dtype != vars[0]->key_dtype)
        return fail(KV_INVALID_ARGUMENT, "var and slot do not have matching shapes (slot dim must be %d x var dim, same device / key dtype)", slot_mult);
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
    BatchStage& st = g_stage[device][1];
    StageSlot* sl = nullptr;
    if ((rc = stage_acquire(st, (size_t)num_tables * sizeof(MultiDesc), &sl))) return rc;
    StageRelease rel{st, sl, s};
    MultiDesc* hd = reinterpret_cast<MultiDesc*>(sl->host);
    for (int i = 0; i < num_tables; ++i) {
      kv_table* v = vars[i];
      if (v->uniq_serial >= 65535u) {   // the 16-bit stamp wraps: every row back to "none"
        k_clear_stamps<<<nblocks((long long)v->rows_ub, TB, 4096), TB, 0, s>>>(dev_view(v), (unsigned)v->rows_ub);
        v->uniq_serial = 0;
      }
      MultiDesc& d = hd[i];
      std::memset(&d, 0, sizeof d);
      d.a.tv = dev_view(v); d.a.ts0 = dev_view(slots0[i]); d.a.ts1 = slots1 ? dev_view(slots1[i]) : d.a.ts0;
      d.a.opt = a; d.a.grad = grads[i]; d.a.day = today(v);
      d.a.opt.fast = fast_math_on(v) ? 1 : 0;
      d.a.n = ns[i];
      d.a.use_hints = claim_slot(v, slots0[i], s) ? 1 : 0;
      if ((rc = mirror_decide<OPT>(v, slots0[i], d.a, true, s))) return rc;
      d.a.uniq_serial = ns[i] > 0 ? ++v->uniq_serial : 0u;
      d.ids = ids[i];
      d.n = ns[i];
    }
    HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, (size_t)num_tables * sizeof(MultiDesc), hipMemcpyHostToDevice, s));
    rel.launched = true;
    const int ids32 = vars[0]->key_dtype == KV_DT_INT32 ? 1 : 0;
    ProfScope ps(vars[0], KV_PROF_APPLY_UNIQUE, s);
    rc = launch_uapply<OPT>(hd[0].a, nullptr, ids32, nmax, s, reinterpret_cast<const MultiDesc*>(sl->dev), num_tables);
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
      const bool held = tokens[i] != 0 && tokens[i] == vars[i]->batch_serial && ns[i] == vars[i]->batch_n && vars[i]->fused_index;
      if (!held) reuse = false;
      if (!held || !vars[i]->part_pending) pa_reuse = false;
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
    if (!reuse) vars[i]->batch_serial = 0;
    if (!reuse && (rc = ensure_capacity(vars[i], ns[i], s))) return rc;
    if ((rc = ensure_capacity(slots0[i], ns[i], s))) return rc;
    if (slots1 && (rc = ensure_capacity(slots1[i], ns[i], s))) return rc;
    if ((rc = ensure_workspace(vars[i], std::max<long long>(ns[i], 1), true, s))) return rc;
    nmax = std::max<long long>(nmax, ns[i]);
  }
  if (nmax == 0) return KV_OK;
  BatchStage& st = g_stage[device][1];
  StageSlot* sl = nullptr;
  if ((rc = stage_acquire(st, (size_t)num_tables * sizeof(MultiDesc), &sl))) return rc;
  StageRelease rel{st, sl, s};
  MultiDesc* hd = reinterpret_cast<MultiDesc*>(sl->host);
  WsDev wmax{};
  for (int i = 0; i < num_tables; ++i) {
    MultiDesc& d = hd[i];
    std::memset(&d, 0, sizeof d);
    d.w = ws_view(vars[i], std::max<long long>(ns[i], 1), selfs ? &selfs[i] : nullptr);
    d.a.tv = dev_view(vars[i]); d.a.ts0 = dev_view(slots0[i]); d.a.ts1 = slots1 ? dev_view(slots1[i]) : d.a.ts0;
    if (fz) { d.a.epart = d.w.epart; d.w.P = fused_default_P(std::max<long long>(ns[i], 1)); d.w.pshift = 64 - ilog2(d.w.P); }
    d.a.opt = a; d.a.grad = grads[i]; d.a.day = today(vars[i]);
    d.a.opt.fast = fast_math_on(vars[i]) ? 1 : 0;
    d.a.det = vars[i]->deterministic ? 1 : 0;
    d.a.n = ns[i];
    d.a.use_hints = claim_slot(vars[i], slots0[i], s) ? 1 : 0;
    if ((rc = mirror_decide<OPT>(vars[i], slots0[i], d.a, fz, s))) return rc;   // (fz: k_papply_multi; else the sorted-position kernels, no mirrors)
    d.ids = ids[i];
    d.n = ns[i];
    if (ns[i] == 0) d.w.ntiles = 0;
    if (reuse && ns[i] > 0 && vars[i]->index_P) { d.w.P = vars[i]->index_P; d.w.pshift = 64 - ilog2(d.w.P); }   // the lookup's partitioning
    d.a.day_lk = d.a.day;
    if (pa_reuse && ns[i] > 0) {   // the pending lookup's own day stamp and counting rule
      PartArgs pend;
      std::memcpy(&pend, vars[i]->pend_pa, sizeof pend);
      d.a.day_lk = pend.day; d.a.count_once = pend.count_once;
      vars[i]->part_pending = false;
    }
    wmax.ntiles = std::max(wmax.ntiles, d.w.ntiles);
    wmax.P = std::max(wmax.P, d.w.P);
  }
  HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, (size_t)num_tables * sizeof(MultiDesc), hipMemcpyHostToDevice, s));
  rel.launched = true;
  const MultiDesc* md = reinterpret_cast<const MultiDesc*>(sl->dev);
  if (fz) {
    // partition pass + update in one launch (k_papply_multi) behind the tile sums; an optimizer that meets the ids first
    // runs the tile pass of all tables in front (PA_APPLYIDX)
    int pa_mode = pa_reuse ? PA_LOOKUP : PA_NONE;
    if (!reuse) {
      for (int i = 0; i < num_tables; ++i) vars[i]->fused_index = true;
      launch_ltile(vars[0], hd[0].a.tv, wmax, nullptr, nullptr, nmax, nullptr, s, -1, md, num_tables, false);
      pa_mode = PA_APPLYIDX;
      for (int i = 0; i < num_tables; ++i)
        if (ns[i] > 0) { vars[i]->batch_serial = ++g_serial; vars[i]->batch_n = ns[i]; vars[i]->index_P = hd[i].w.P; }
    }
    if ((rc = launch_tsum(hd[0].a.tv, wmax, nullptr, s, md, num_tables)))
      return fail(rc, "tile sums: no kernel for dim %d", D);
    rc = launch_papply<OPT>(wmax, hd[0].a, pa_mode, s, md, num_tables);
    if (rc) return fail(rc, "partition + apply pass: no kernel for dim %d", D);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  for (int i = 0; i < num_tables; ++i) vars[i]->fused_index = false;
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
// The caller holds the locks.  self: kv_shard_apply_serve's own segment, read in place.
template <int OPT>
static int apply_common(kv_table* v, kv_table* s0, kv_table* s1, const float* grad, const void* ids, int64_t n,
                        const OptArgs& a, kv_batch_token_t token, hipStream_t s, bool unique, const SelfSegment* self) {
  const long long nmax = fused_tab(v) ? FUSED_MAX_N : (1ll << 21);
  if (n < 0 || n > nmax)
    return fail(n < 0 ? KV_INVALID_ARGUMENT : KV_UNIMPLEMENTED,
                "indices: %lld ids in one optimizer call (limit %lld for this embedding dim; split the batch)", (long long)n, nmax);
  if (n > 0 && (!grad || !ids)) return fail(KV_INVALID_ARGUMENT, "grad / indices pointer is null");
  if (!dim_supported(v->dim))
    return fail(KV_UNIMPLEMENTED, "embedding dim %d not supported by the fused kernels", v->dim);
  int rc;
  if (unique && fused_ok(v->dim) && !stream_is_capturing(s)) {
    // The caller promises unique ids (kv_apply_*_unique; kv_uapply.h): one launch, one lane group per id.  A pending
    // partition pass was settled by the caller's hand_over (no token is given).  Dims the kernel does not serve take the
    // batch pipeline below, which needs no promise.
    if ((rc = ensure_capacity(v, n, s)) || (rc = ensure_capacity(s0, n, s)) || (s1 && (rc = ensure_capacity(s1, n, s)))) return rc;
    if (v->uniq_serial >= 65535u) {   // the 16-bit stamp wraps: every row back to "none" (once per 65535 launches)
      k_clear_stamps<<<nblocks((long long)v->rows_ub, TB, 4096), TB, 0, s>>>(dev_view(v), (unsigned)v->rows_ub);
      v->uniq_serial = 0;
    }
    PartArgs pa{};
    pa.tv = dev_view(v); pa.ts0 = dev_view(s0); pa.ts1 = s1 ? dev_view(s1) : pa.ts0;
    pa.opt = a; pa.grad = grad; pa.day = today(v);
    pa.opt.fast = fast_math_on(v) ? 1 : 0;
    pa.n = n;
    pa.use_hints = claim_slot(v, s0, s) ? 1 : 0;
    if ((rc = mirror_decide<OPT>(v, s0, pa, true, s))) return rc;
    pa.uniq_serial = ++v->uniq_serial;
    ProfScope ps(v, KV_PROF_APPLY_UNIQUE, s);
    rc = launch_uapply<OPT>(pa, ids, v->key_dtype == KV_DT_INT32 ? 1 : 0, n, s);
    if (rc) return fail(rc, "unique apply: no kernel for dim %d", v->dim);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  const bool reuse = token != 0 && token == v->batch_serial && n == v->batch_n;
  // The entry-list kernels serve this dim (pa_route): the tile sums, then k_papply — the partition pass and the update in
  // one launch — in the mode the batch's state asks for:
  //   PA_LOOKUP    the token names the lookup whose partition pass is still pending: k_papply completes its bookkeeping too
  //   PA_NONE      the token names a batch whose bookkeeping is done (a second optimizer on the token; a pass another op settled)
  //   PA_APPLYIDX  no (valid) token: the optimizer meets the ids first — the tile pass runs with the tile sums (k_ltsum)
  const bool pa_route = fused_tab(v);
  int pa_mode = -1;
  PartArgs pend{};
  const void* tile_ids = nullptr;   // != nullptr: the batch's tile pass runs in front of the apply (k_ltsum)
  if (v->part_pending) {
    if (reuse && pa_route && v->fused_index) {
      std::memcpy(&pend, v->pend_pa, sizeof pend);
      v->part_pending = false;
      pa_mode = PA_LOOKUP;
    } else if ((rc = flush_part(v, s))) {
      return rc;
    }
  }
  if (!reuse && (rc = ensure_capacity(v, n, s))) return rc;
  if ((rc = ensure_capacity(s0, n, s))) return rc;
  if (s1 && (rc = ensure_capacity(s1, n, s))) return rc;
  if ((rc = ensure_workspace(v, n, true, s))) return rc;
  WsDev wd = ws_view(v, n, self);
  PartArgs pa{};
  pa.tv = dev_view(v); pa.ts0 = dev_view(s0); pa.ts1 = s1 ? dev_view(s1) : pa.ts0;
  pa.opt = a; pa.grad = grad; pa.day = today(v);
  pa.opt.fast = fast_math_on(v) ? 1 : 0;
  pa.det = det_mode(v);
  pa.n = n;
  pa.use_hints = claim_slot(v, s0, s) ? 1 : 0;
  pa.day_lk = pa.day;
  if (pa_mode == PA_LOOKUP) { pa.day_lk = pend.day; pa.count_once = pend.count_once; }
  if (!reuse) {
    v->batch_serial = 0;
    if (pa_route) {   // tile pass + tile sums in one launch, then partition pass + update in one launch
      v->fused_index = true;
      choose_partitions(v, wd, n);
      tile_ids = ids;
      pa_mode = PA_APPLYIDX;
    } else {
      index_pass<MODE_APPLYIDX>(v, wd, pa, ids, nullptr, n, -1, nullptr, s);
    }
    v->batch_serial = ++g_serial;   // the index stays valid for this batch (e.g. a second optimizer on the same ids)
    v->batch_n = n;
  } else if (pa_mode < 0 && v->fused_index) {
    pa_mode = PA_NONE;   // the tiles' entries of a batch whose bookkeeping is done
  }
  if (v->fused_index && reuse && v->index_P) { wd.P = v->index_P; wd.pshift = 64 - ilog2(wd.P); }   // the lookup's partitioning
  if ((rc = mirror_decide<OPT>(v, s0, pa, v->fused_index, s))) return rc;
  if (v->fused_index) rc = fused_apply<OPT>(v, wd, pa, n, s, pa_mode, tile_ids);
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

namespace __attribute__((visibility("hidden"))) kvhip_internal {
// The sharded ops' `optimizer` code is the OPT_* value; their hp[] layout:
// 0 GroupAdam V4, 1 GroupAdam V3 (hp = lr, beta1_power, beta2_power, beta1, beta2, epsilon, l1, l2, l21),
// 2 Adagrad (hp = lr, update_slots), 3 SparseGroupFtrl (hp = lr, l1, l2, l21, l2_shrinkage, lr_power; slot1 = linear),
// 4 FTRL-V2 / 5 group FTRL-V2 (hp = lr, l1, l2, l2_shrinkage, lr_power; slot1 = linear)
OptCall shard_opt_call(int optimizer, const float* hp) {
  switch (optimizer) {
    case OPT_ADAM_V4: case OPT_ADAM_V3:
      return group_adam_call(optimizer == OPT_ADAM_V4 ? 4 : 3, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7], hp[8]);
    case OPT_ADAGRAD: return adagrad_call(hp[0], hp[1] != 0.f);
    case OPT_FTRL: return sparse_group_ftrl_call(hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]);
    case OPT_FTRL_V2: case OPT_GROUP_FTRL_V2: return ftrl_v2_call(optimizer, hp[0], hp[1], hp[2], hp[3], hp[4]);
    default: return OptCall{};
  }
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
    default: return fail(KV_INTERNAL, "optimizer %d", opt);
  }
}

// One table (s1: the linear table of the FTRL family).  The reference's single-table ops check, in this order: the handles,
// the optimizer itself (GroupAdam version), the tables' initialisation, the hyperparameters, the shapes.  So c.status is
// reported at its place in that order (nothing calls fail() before it unless it returns).  The batched ops report it first.
int apply_one(const OptCall& c, kv_table* v, kv_table* s0, kv_table* s1, const float* grad, const void* ids, int64_t n,
              kv_batch_token_t token, kv_stream_t stream, bool unique, const SelfSegment* self) {
  int rc;
  const bool two = two_slots(c.opt);
  if ((rc = check_table(v)) || (rc = check_table(s0)) || (two && (rc = check_table(s1)))) return rc;
  if (c.status && c.opt < 0) return c.status;
  if (group_adam(c.opt)) {   // order and wording of training_ops.cc:7001-7103
    if (!v->initialized || !s0->initialized)
      return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: %s", !v->initialized ? "var" : "m_v_linear");
  } else if (!two) {
    if (!v->initialized || !s0->initialized)
      return fail(KV_FAILED_PRECONDITION, "Attempting to use uninitialized variables: %s", !v->initialized ? "var" : "accum");
  } else if (!v->initialized || !s0->initialized || !s1->initialized) {
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables");
  }
  if (c.status) return c.status;
  if (group_adam(c.opt)) {
    if (s0->dim != c.slot_mult * v->dim)
      return fail(KV_INVALID_ARGUMENT, "kv_variable and linear do not have the same shape [%d] [%d] (m_v_linear must be 3x)", v->dim, s0->dim);
    if (v->device != s0->device) return fail(KV_INVALID_ARGUMENT, "var and slot live on different devices");
    if (v == s0) return fail(KV_INVALID_ARGUMENT, "var and m_v_linear are the same table");
  } else if (!two) {
    if (s0->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "var and accum do not have the same shape [%d] [%d]", v->dim, s0->dim);
    if (v->device != s0->device || v == s0) return fail(KV_INVALID_ARGUMENT, "var and accum must be distinct tables on one device");
  } else {
    if (s0->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "kv_varaible and accum do not have the same shape [%d] [%d]", v->dim, s0->dim);
    if (s1->dim != v->dim) return fail(KV_INVALID_ARGUMENT, "kv_variable and linear do not have the same shape [%d] [%d]", v->dim, s1->dim);
    if (v->device != s0->device || v->device != s1->device || v == s0 || v == s1 || s0 == s1)
      return fail(KV_INVALID_ARGUMENT, "var, accum and linear must be distinct tables on one device");
  }
  if (n == 0) return KV_OK;
  DeviceGuard dg(v->device);
  MultiLock lk({v, s0, two ? s1 : s0});
  // GroupAdam / Adagrad: apply_common decides whether this apply works on the mirrors (mirror_decide); the FTRL family reads
  // and writes the slot tables' own records: its entry ends the tables' epochs
  auto keep = [&](const kv_table* t) -> unsigned { return two ? KEEP_NONE : (t == v ? KEEP_VAR : KEEP_NONE) | (t == s0 ? KEEP_SLOT : KEEP_NONE); };
  hipStream_t s = (hipStream_t)stream;
  if ((rc = lk.enter(s, keep, token != 0 && token == v->batch_serial ? v : nullptr))) return rc;
  OptArgs a = c.a;
  a.l21_norm = a.l21 * std::sqrt((float)v->dim);   // training_ops.cc:728
  return with_opt(c.opt, [&](auto o) { return apply_common<decltype(o)::value>(v, s0, two ? s1 : nullptr, grad, ids, n, a, token, s, unique, self); });
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
    k_clear_hints<<<nblocks((long long)v->cap + 1, TB, 8192), TB, 0, s>>>(v->entries, v->cap + 1);
  v->slot_uid = sl->uid;
  v->slot_gen = sl->gen;
  v->batch_serial = 0;
  // (the entry above ended any running epoch of either table; a pair of single-chunk tables gets its mirrors filled here)
  const bool mir = v->chunks.size() == 1 && sl->chunks.size() == 1 && !v->track_delta && !sl->track_delta && mirror_pair(v, sl, s);
  if (nrows > 1)
    k_link_hints<<<nblocks(nrows, TB, 8192), TB, 0, s>>>(dev_view(v), dev_view(sl), nrows, v->mirror_epoch.load() & 0xFFFFu, mir ? 1 : 0);
  HIP_TRY(hipGetLastError());
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
  t->batch_serial = 0;      // the index a lookup left was built by the other pipeline's rules
  t->fused_index = false;
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
  if (which == KV_STAT_MIRROR_EPOCHS) { *value = t->stat_mirror_epochs.load(); return KV_OK; }
  return fail(KV_INVALID_ARGUMENT, "kv_get_stat: unknown counter %d", which);
}

int kv_prepare_capture(kv_handle_t t, int64_t max_new_ids, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (max_new_ids < 0) return fail(KV_INVALID_ARGUMENT, "max_new_ids < 0");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = enter_op(t, s))) return rc;
  mirror_ban(t, s);   // (a captured apply replays without host code: no slot mirrors for this table from here on)
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

// inverse[i] = the dense number of position i's id: position -> its entry in its tile -> the number k_papply PA_UNIQUE gave it
__global__ void __launch_bounds__(TB) k_inverse_e(const unsigned short* __restrict__ pos_ent, const unsigned* __restrict__ ent_b,
                                                  long long n, int* __restrict__ inverse) {
  for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += (long long)gridDim.x * TB)
    inverse[i] = (int)ent_b[(size_t)(i / TILE) * TILE + pos_ent[i]];
}

// tf.unique_with_counts on the entry-list kernels (any dim: no row is touched): a table-less tile pass (entries, every
// position's entry) and k_papply PA_UNIQUE with dense numbers — uniq / uniq_counts written, every entry learns its id's
// number, the count in wd.ctr[0].  The table's mutex is held by the caller.
// the table-less tile pass of the distinct-id ops: entries, every position's entry number (pos_ent)
static int unique_tile_pass(kv_table* t, WsDev& wd, PartArgs& pa, const void* ids, const int* counts, long long n, hipStream_t s) {
  Workspace& ws = t->ws;
  int rc;
  if (ws.pos_cap < n) {
    if ((rc = ws_sync(s))) return rc;   // (refused under a stream capture before anything is queued, like ensure_workspace)
    ws.pos_cap = 0;
    if ((rc = regrow(&ws.pos_ent, (size_t)std::max<long long>(n, ws.cap_n)))) return rc;
    ws.pos_cap = std::max<long long>(n, ws.cap_n);
  }
  t->fused_index = true;
  choose_partitions(t, wd, n);
  wd.pos_ent = ws.pos_ent;
  launch_ltile_notable(t, pa.tv, wd, ids, n, s, counts, t->key_dtype == KV_DT_INT32);
  return KV_OK;
}
static int fused_unique_pass(kv_table* t, WsDev& wd, PartArgs& pa, const void* ids, const int* counts, long long n, hipStream_t s) {
  int rc;
  if ((rc = unique_tile_pass(t, wd, pa, ids, counts, n, s))) return rc;
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

// tf.unique + unsorted_segment_sum on the batch pipeline; the table's mutex is held by the caller.
// fold_op: how the rows of one id combine (KV_SCATTER_ADD = sum, MUL = product, MIN, MAX)
static int dedup_locked(kv_table* t, const void* ids, const float* grad, int64_t n, int64_t* uniq,
                        float* summed, int32_t* inverse, int64_t* num_unique, int fold_op, hipStream_t s) {
  int rc;
  if ((rc = ensure_workspace(t, n, true, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch_serial = 0;
  PartArgs pa{};
  pa.tv = dev_view(t); pa.ts0 = pa.tv; pa.ts1 = pa.tv;
  pa.grad = grad;
  pa.out_keys = (long long*)uniq;
  pa.out_sum = summed;
  pa.fold_op = fold_op;
  pa.det = det_mode(t);
  pa.n = n;
  if (fold_op == KV_SCATTER_ADD && fused_tab(t)) {
    // the entry-list kernels: distinct ids numbered (fused_unique_pass), tile sums of the rows of ids repeated inside their
    // tile (k_tsum), the per-id sums over the tiles' entries straight to summed[number] (k_papply PA_DEDUP)
    // (round 6: ONE partition pass — k_papply PA_DEDUP numbers the ids it sums, dd_number — where PA_UNIQUE's numbering pass
    //  ran in front of it: the table-less tile pass, the tile sums, the pass)
    if ((rc = unique_tile_pass(t, wd, pa, ids, nullptr, n, s))) return rc;
    pa.out_map = nullptr;
    pa.dd_number = 1;
    pa.epart = wd.epart;
    pa.day_lk = pa.day;
    if ((rc = launch_tsum(pa.tv, wd, grad, s))) return fail(rc, "tile sums: no kernel for dim %d", t->dim);
    if ((rc = launch_papply_ud(wd, pa, PA_DEDUP, s))) return fail(rc, "per-id sums: no kernel for dim %d", t->dim);
    if (inverse) k_inverse_e<<<nblocks(n, TB, 2048), TB, 0, s>>>(t->ws.pos_ent, wd.ent_b, n, inverse);
  } else {
    index_pass<MODE_UNIQUE>(t, wd, pa, ids, nullptr, n, -1, nullptr, s);
    if ((rc = launch_apply<MODE_DEDUP, OPT_ADAGRAD>(t, wd, pa, n, s))) return rc;
    if (inverse) k_dedup_inverse<<<nblocks(n, TB, 2048), TB, 0, s>>>(wd, n, inverse);
  }
  unsigned U = 0;
  if ((rc = read_count(t, wd.ctr, s, &U))) return rc;
  *num_unique = U;
  return KV_OK;
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
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, (hipStream_t)stream, KEEP_VAR | KEEP_SLOT))) return rc;
  return dedup_locked(t, ids, grad, n, uniq, summed, inverse, num_unique, KV_SCATTER_ADD, (hipStream_t)stream);
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
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, s, KEEP_VAR | KEEP_SLOT))) return rc;
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_segments * t->dim * sizeof(float), s));  // segments nobody names
  if (n == 0) return KV_OK;
  if ((rc = ensure_workspace(t, n, true, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch_serial = 0;
  PartArgs pa{};
  pa.tv = dev_view(t); pa.ts0 = pa.tv; pa.ts1 = pa.tv;
  pa.grad = data;
  pa.out_sum = out;
  pa.direct_rows = num_segments;
  pa.fold_op = KV_SCATTER_ADD;
  pa.det = det_mode(t);
  pa.n = n;
  if (fused_tab(t)) {
    // the entry-list kernels: the segment ids de-duplicated per tile (no numbering: an id IS its output row), the tile
    // sums, the per-id sums over the tiles' entries straight to out[id]
    t->fused_index = true;
    choose_partitions(t, wd, n);
    launch_ltile_notable(t, pa.tv, wd, segment_ids, n, s, nullptr, true);
    pa.epart = wd.epart;
    pa.day_lk = pa.day;
    if ((rc = launch_tsum(pa.tv, wd, data, s))) return fail(rc, "tile sums: no kernel for dim %d", t->dim);
    if ((rc = launch_papply_ud(wd, pa, PA_DEDUP, s))) return fail(rc, "segment sums: no kernel for dim %d", t->dim);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  index_pass<MODE_UNIQUE>(t, wd, pa, segment_ids, nullptr, n, 1, nullptr, s);
  if ((rc = launch_apply<MODE_DEDUP, OPT_ADAGRAD>(t, wd, pa, n, s))) return rc;
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
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  // `t` lends its workspace: neither its rows nor any record is touched
  if ((rc = enter_op(t, s, KEEP_VAR | KEEP_SLOT))) return rc;
  if ((rc = ensure_workspace(t, n, false, s))) return rc;
  WsDev wd = ws_view(t, n);
  t->batch_serial = 0;
  PartArgs pa{};
  pa.tv = dev_view(t); pa.ts0 = pa.tv; pa.ts1 = pa.tv;
  pa.out_keys = (long long*)uniq;
  pa.out_counts = uniq_counts;
  pa.det = det_mode(t);
  pa.n = n;
  // the entry-list kernels, whatever the table's dim (no row is touched)
  if ((rc = fused_unique_pass(t, wd, pa, ids, counts, n, s))) return rc;
  if (inverse) k_inverse_e<<<nblocks(n, TB, 2048), TB, 0, s>>>(t->ws.pos_ent, wd.ent_b, n, inverse);
  if (num_unique_dev) k_store_count<<<1, 1, 0, s>>>(wd.ctr, (long long*)num_unique_dev);
  HIP_TRY(hipGetLastError());
  if (num_unique) {   // synchronous form
    unsigned U = 0;
    int rc2;
    if ((rc2 = read_count(t, wd.ctr, s, &U))) return rc2;
    *num_unique = U;
  }
  return KV_OK;
}

// the free-list stack must hold every row of the slab
static int ensure_free_list(kv_table* t, hipStream_t s) {
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

static int delete_locked(kv_table* t, const void* ids, int64_t n, int64_t* num_deleted, hipStream_t s);

int kv_delete(kv_handle_t t, const void* ids, int64_t n, int64_t* num_deleted, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (num_deleted) *num_deleted = 0;
  if (n < 0 || (n > 0 && !ids)) return fail(KV_INVALID_ARGUMENT, "indices pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  if (n == 0) return KV_OK;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = record_deleted(t, ids, n, t->key_dtype == KV_DT_INT32, (hipStream_t)stream))) return rc;
  return delete_locked(t, ids, n, num_deleted, (hipStream_t)stream);
}

static int delete_locked(kv_table* t, const void* ids, int64_t n, int64_t* num_deleted, hipStream_t s) {
  int rc;
  if ((rc = enter_op(t, s))) return rc;
  t->batch_serial = 0;   // rows are released: an index of a batch that held them is void (its token goes stale)
  if ((rc = ensure_free_list(t, s))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  const TableDev td = dev_view(t);
  if (t->key_dtype == KV_DT_INT32)
    k_delete<int><<<nblocks(n, TB, 4096), TB, 0, s>>>(td, (const int*)ids, n, t->free_rows, t->d_stat);
  else
    k_delete<long long><<<nblocks(n, TB, 4096), TB, 0, s>>>(td, (const long long*)ids, n, t->free_rows, t->d_stat);
  HIP_TRY(hipGetLastError());
  unsigned long long rel = 0;
  if ((rc = after_release(t, s, &rel))) return rc;
  if (num_deleted) *num_deleted = (int64_t)rel;
  return KV_OK;
}

int kv_delete_with_timestamp(kv_handle_t t, int threshold, int dry_run, int64_t* out_keys, int64_t* count,
                             kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!count || (!dry_run && !out_keys)) return fail(KV_INVALID_ARGUMENT, "count / delete_keys pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if (!dry_run) {   // out_keys was sized by a dry run: nothing may have touched the table (or its clock) since
    if (t->expire_serial != t->op_serial)
      return fail(KV_FAILED_PRECONDITION, "the table was used between the dry run and kv_delete_with_timestamp: the key "
                                          "buffer sized from the count may be too small; count again");
    ++t->op_serial;
    t->batch_serial = 0;   // rows are released: an index of a batch that held them is void
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

static int count_or_ts(kv_handle_t t, const void* ids, int64_t n, int what, uint32_t* out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (n < 0 || (n > 0 && (!ids || !out))) return fail(KV_INVALID_ARGUMENT, "indices / output pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  if (n == 0) return KV_OK;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = join_side(t, s))) return rc;
  if (t->key_dtype == KV_DT_INT32)
    k_get_count_ts<int><<<nblocks(n, TB, 4096), TB, 0, s>>>(dev_view(t), (const int*)ids, n, what, today(t), out);
  else
    k_get_count_ts<long long><<<nblocks(n, TB, 4096), TB, 0, s>>>(dev_view(t), (const long long*)ids, n, what, today(t), out);
  HIP_TRY(hipGetLastError());
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

int kv_export_count(kv_handle_t t, int first_n, int64_t* counts, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  k_export<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, first_n, 0, t->d_stat, nullptr,
                                                   nullptr, nullptr, nullptr, nullptr);
  unsigned long long c[3];
  HIP_TRY(hipMemcpyAsync(c, t->d_stat, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t->export_serial = t->op_serial;
  counts[0] = (int64_t)c[0]; counts[1] = (int64_t)c[1]; counts[2] = (int64_t)c[2];
  return KV_OK;
}

int kv_export_fill(kv_handle_t t, int first_n, int64_t* keys, float* values, int64_t* blacklist,
                   int64_t* fkeys, uint32_t* fvals, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if (t->export_serial != t->op_serial)
    return fail(KV_FAILED_PRECONDITION, "the table was used between kv_export_count and kv_export_fill: the buffers sized "
                                        "from the counts may be too small; count again");
  ++t->op_serial;   // a fill ends the export (delta lists handed on): the next fill needs a new count
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  k_export<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, first_n, 1, t->d_stat,
                                                   (long long*)keys, values, (long long*)blacklist,
                                                   (long long*)fkeys, fvals);
  HIP_TRY(hipGetLastError());
  if (first_n > 2 && (rc = delta_after_export(t, first_n, nrows, s))) return rc;  // dynamic_save.hpp:179-192
  return KV_OK;
}

int kv_set_delta_tracking(kv_handle_t t, int support_delta_export, int support_prediction_delta_export) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = settle_pending(t))) return rc;
  t->track_delta = support_delta_export != 0;
  t->track_pred = support_prediction_delta_export != 0;
  return KV_OK;
}

int kv_export_delta_count(kv_handle_t t, int first_n, int64_t* counts, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (!counts) return fail(KV_INVALID_ARGUMENT, "counts pointer is null");
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  std::vector<long long> absent;
  if ((rc = delta_prepare(t, first_n, s, &absent))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  k_export_delta<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, first_n, 0, t->d_stat, nullptr,
                                                         nullptr, nullptr, nullptr, nullptr);
  unsigned long long c[3];
  HIP_TRY(hipMemcpyAsync(c, t->d_stat, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
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
  if (!t->initialized)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if (t->delta_serial != t->op_serial)
    return fail(KV_FAILED_PRECONDITION, "the table was used between kv_export_delta_count and kv_export_delta_fill: the "
                                        "buffers sized from the counts may be too small; count again");
  ++t->op_serial;
  unsigned nrows = 1;
  if ((rc = stats(t, s, nullptr, &nrows))) return rc;
  std::vector<long long> absent;
  if ((rc = delta_prepare(t, first_n, s, &absent))) return rc;
  HIP_TRY(hipMemsetAsync(t->d_stat, 0, 4 * sizeof(unsigned long long), s));
  // prediction exports move the blacklisted keys to the delete list (dynamic_save.hpp:345-351)
  k_export_delta<<<nblocks(nrows, TB, 2048), TB, 0, s>>>(dev_view(t), nrows, first_n, 1, t->d_stat, (long long*)keys,
                                                         values, (long long*)(first_n > 3 ? blacklist : delete_keys),
                                                         (long long*)fkeys, fvals);
  HIP_TRY(hipGetLastError());
  unsigned long long c[3];
  HIP_TRY(hipMemcpyAsync(c, t->d_stat, sizeof c, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
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

// insert / scatter / import marks: tile pass (dedup) -> partition pass on the unique keys
static int scatter_like(kv_handle_t t, const void* ids, const float* vals, int64_t n, int op,
                        int is_insert, int mark, const unsigned* fvals, hipStream_t s) {
  int rc;
  if (n == 0) return KV_OK;
  if (n < 0 || !ids || (!vals && mark < 0)) return fail(KV_INVALID_ARGUMENT, "bad arguments");
  if (!t->initialized && !is_insert && mark < 0)
    return fail(KV_FAILED_PRECONDITION, "Failed to use uninitialized variables: KvVariable init table not set");
  const long long CH = 1ll << 21;
  const size_t idsz = t->key_dtype == KV_DT_INT32 ? 4 : 8;
  for (long long off = 0; off < n; off += CH) {
    const long long m = std::min(CH, (long long)n - off);
    if ((rc = ensure_capacity(t, m, s))) return rc;
    if ((rc = ensure_workspace(t, m, false, s))) return rc;
    const WsDev wd = ws_view(t, m);
    PartArgs pa{};
    pa.tv = dev_view(t);
    if (!t->initialized) {
      // InsertOrUpdate / import never consult the init table; new rows start from the zero row
      pa.tv.init_table = t->chunks[0].rows;
      pa.tv.init_rows = 1;
    }
    pa.ts0 = pa.tv; pa.ts1 = pa.tv;
    pa.grad = vals ? vals + (size_t)off * t->dim : nullptr;
    pa.scatter_op = op; pa.is_insert = is_insert;
    pa.mark_what = mark; pa.fvals = fvals ? fvals + off : nullptr;
    t->batch_serial = 0;
    launch_tile<true>(t, wd, (const char*)ids + (size_t)off * idsz, nullptr, m, s);
    if (mark >= 0) launch_part_keys<MODE_MARK>(wd, pa, s);
    else launch_part_keys<MODE_SCATTER>(wd, pa, s);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_insert(kv_handle_t t, const void* ids, const float* values, int64_t n, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  if ((rc = enter_op(t, (hipStream_t)stream))) return rc;
  return scatter_like(t, ids, values, n, KV_SCATTER_ASSIGN, 1, -1, nullptr, (hipStream_t)stream);
}

int kv_scatter_update(kv_handle_t t, const void* ids, const float* updates, int64_t n, int op,
                      kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (op < KV_SCATTER_ASSIGN || op > KV_SCATTER_MAX) return fail(KV_INVALID_ARGUMENT, "unsupported update operation %d", op);
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
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
      HIP_TRY(hipStreamSynchronize(s));
      const long long cap = std::max<long long>(want, std::min<long long>(w.scat_cap * 2, CHK));
      w.scat_cap = 0;
      if ((rc = regrow(&w.scat_keys, (size_t)cap)) || (rc = regrow(&w.scat_sum, (size_t)cap * t->dim))) return rc;
      w.scat_cap = cap;
    }
    for (long long off = 0; off < n; off += CHK) {
      const long long m = std::min(CHK, (long long)n - off);
      int64_t U = 0;
      if ((rc = dedup_locked(t, (const char*)ids + (size_t)off * idsz, updates + (size_t)off * t->dim, m,
                             (int64_t*)w.scat_keys, w.scat_sum, nullptr, &U, fold, s)))
        return rc;
      if (t->key_dtype == KV_DT_INT32 && U > 0)   // the unique list is int64; the table's ops take its own key type
        k_narrow_keys<<<1, 1024, 0, s>>>(w.scat_keys, U);
      if ((rc = scatter_like(t, w.scat_keys, w.scat_sum, U, op, 0, -1, nullptr, s))) return rc;
    }
    return KV_OK;
  }
  // assign: one of the occurrences of a repeated id stays (the reference's result depends on its thread
  // interleaving there); dims outside the fused kernels' range take this path for every operation
  return scatter_like(t, ids, updates, n, op, 0, -1, nullptr, s);
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

int kv_import_delta(kv_handle_t t, const int64_t* keys, const float* values, int64_t n, const int64_t* blacklist,
                    int64_t n_black, const int64_t* fkeys, const uint32_t* fvals, int64_t n_freq,
                    const int64_t* delete_keys, int64_t n_delete, int first_n, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
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
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  if (t->key_dtype == KV_DT_INT32) return fail(KV_UNIMPLEMENTED, "import with int32 keys");
  if ((rc = enter_op(t, s))) return rc;
  // clear(): dynamic_restore.hpp:60-62
  HIP_TRY(hipStreamSynchronize(s));
  t->gen += 1;            // row ids start over: slot-row hints into this table are void
  t->slot_uid = 0;        // and the fresh index carries none of its own
  t->batch_serial = 0;
  unsigned init[3] = {1, 0, 0};
  HIP_TRY(hipMemcpy(t->d_counters, init, sizeof init, hipMemcpyHostToDevice));  // stack source: synchronous
  k_fill_entries<<<nblocks((long long)t->cap + 1, TB, 8192), TB, 0, s>>>(t->entries, t->cap + 1);
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
