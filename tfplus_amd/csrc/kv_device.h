// kv_device.h — device-side types and helpers of libkvhip (included into the anonymous namespace of every unit that has
// device code or uses its constants; no kernel lives here).
#pragma once

// ------------------------------------------------------------------------------------------
// constants
// ------------------------------------------------------------------------------------------
constexpr long long EMPTY_KEY = (long long)0x8000000000000000ULL;
constexpr unsigned FLAG_BLACK = 1u;   // EmbeddingValue::in_black_   (embedding_value.h:225)
constexpr unsigned FLAG_UNDER = 2u;   // EmbeddingValue::under_threshold_
constexpr unsigned FLAG_DIRTY = 4u;   // row changed since under_threshold was computed (Adagrad: no CoverUpdate)
constexpr float CUTOFF = 1.0e-20f;    // DEFAULT_CUTOFF_VALUE (kv_variable_interface.h:55)
constexpr unsigned FLAG_FREE = 8u;    // row released by Delete (table_manager.h:405-416): skipped by scans, reusable
constexpr unsigned ROW_TOMB = 0xFFFFFFFFu;  // index entry of a deleted key (kept so probe chains stay intact;
                                            // the same key revives it, an index rebuild drops it)
constexpr unsigned ROW_FILTERED = 0x80000000u;  // tag bit: var frequency < enter_threshold
constexpr unsigned ROW_MASK = 0x7FFFFFFFu;
constexpr unsigned HEAD_BIT = 0x80000000u;      // sorted position list / ent_base: first position of its key
constexpr unsigned BASE_MASK = 0x3FFFFFFFu;
constexpr int RANK_SHIFT = 21;                  // slot_rank: entry index (21 bits, n <= 2^21) | in-tile occurrence rank << 21
constexpr unsigned SLOT_MASK = (1u << RANK_SHIFT) - 1u;
constexpr int LCOLD = 16;   // a key with at most this many occurrences in the batch is "cold": one lane group sums its
                            // rows and updates it; a "hot" key's rows are summed in chunks by whole waves
constexpr int HC = 128;     // rows per hot chunk
// ---- the entry-list pipeline (kv_fused.h) ----
constexpr unsigned EP_TAG = 0x40000000u;    // entry list: the source is row (word & ~EP_TAG) of epart, not an input position
constexpr unsigned NEW_BIT = 0x80000000u;   // ent_b row word: the key was inserted by this batch (row part 0: by another tile, row not seen yet)
constexpr unsigned HINT_NEW = 0xFFFFFFFFu;  // Entry::hint of a key inserted by the batch in flight (the partition pass resets it)
constexpr int HC2 = 512;    // entries per hot chunk of the entry-list apply: a key has at most one entry per tile, so up to
                            // 1 M ids no key spans chunks and k_apply_fin is not launched

constexpr int TB = 256;          // threads per block of the gather / maintenance kernels
#ifndef KV_TBT
#define KV_TBT 512   // (A/B: 256 = 1024-id tiles, four tile blocks per CU)
#endif
constexpr int TBT = KV_TBT;  // threads per block of the tile kernel
constexpr int IPT = 4;           // ids per thread in the tile kernel
constexpr int TILE = TBT * IPT;  // ids per tile (2048): a key present in every tile contributes
                                 // N / 2048 entries to its partition, which keeps the partition
                                 // blocks' LDS lists small enough for 4 blocks per CU
constexpr int LS = 2 * TILE;     // LDS hash slots per tile (load <= 0.5)
constexpr int MAX_P = 2048;      // partitions (power of two); 1024 up to 1 M ids, 2048 for 2 M
constexpr int MAX_CHUNKS = 32768;   // 2^16-row chunks (no capacity hint) still reach the 2^31-row limit

// In-kernel phase stamps for the diagnostic build (never in the product .so): thread 0 of each
// block stores s_memtime at phase boundaries into a buffer nothing else reads.
#ifdef KV_STAMPS
#define KV_STAMP(slot) do { if (threadIdx.x == 0) w.dbg[(size_t)blockIdx.x * 16 + (slot)] = wall_clock64(); } while (0)
#define KV_STAMPP(slot) do { if (threadIdx.x == 0) w.dbg[(size_t)(blockIdx.x + 4096) * 16 + (slot)] = wall_clock64(); } while (0)
// where the block runs: HW_ID (wave / simd / cu / sh / se) and XCC_ID
#define KV_STAMP_HW(slot) do { if (threadIdx.x == 0) w.dbg[(size_t)blockIdx.x * 16 + (slot)] = \
    ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492); } while (0)
#define KV_STAMPPV(slot, v) do { if (threadIdx.x == 0) w.dbg[(size_t)(blockIdx.x + 4096) * 16 + (slot)] = (v); } while (0)
#define KV_STAMPA(slot) do { if (threadIdx.x == 0) w.dbg[(size_t)(blockIdx.x + 8192) * 16 + (slot)] = wall_clock64(); } while (0)
#define KV_STAMPV(slot, v) do { if (threadIdx.x == 0) w.dbg[(size_t)(blockIdx.x + 8192) * 16 + (slot)] = (v); } while (0)
#define KV_STAMPT(slot) do { if (threadIdx.x == 0) w.dbg[(size_t)(blockIdx.x + 2048) * 16 + (slot)] = wall_clock64(); } while (0)
#else
#define KV_STAMP(slot) do { } while (0)
#define KV_STAMPP(slot) do { } while (0)
#define KV_STAMP_HW(slot) do { } while (0)
#define KV_STAMPPV(slot, v) do { } while (0)
#define KV_STAMPA(slot) do { } while (0)
#define KV_STAMPV(slot, v) do { } while (0)
#define KV_STAMPT(slot) do { } while (0)
#endif

// Blocks of `threads` threads of kernel `k` that are resident at once on the CURRENT device (CUs x occupancy, at most
// `cap_per_cu` per CU: above 96 SGPRs the hardware admits 6 blocks of 256 threads, one fewer than the API says), cached
// PER DEVICE: a process that drives GPUs with different CU counts or partition modes gets each device's own number
// (a function-local static kept the first caller's device).  The kernel is the template argument: one cache per
// kernel instantiation (two of one function-pointer type differ in registers, hence in occupancy).
template <auto Kernel>
static inline int resident_blocks(int threads, int cap_per_cu, int fallback_per_cu) {
  constexpr int MAXDEV = 64;
  static int cache[MAXDEV];   // 0 = not asked yet (benign race: every thread computes the same number)
  int dev = 0;
  hipGetDevice(&dev);
  const bool slot = dev >= 0 && dev < MAXDEV;
  if (slot) { const int c = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED); if (c > 0) return c; }
  int nb = 0, cus = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, threads, 0) != hipSuccess || nb < 1) nb = fallback_per_cu;
  if (nb > cap_per_cu) nb = cap_per_cu;
  const int r = nb * (cus > 0 ? cus : 256);
  if (slot) __atomic_store_n(&cache[dev], r, __ATOMIC_RELAXED);
  return r;
}

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}
// same picker as oracle/kv_oracle.cc (splitmix64 finaliser) — see kv_set_seed
__device__ __forceinline__ unsigned long long pick64(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
  x ^= x >> 27; x *= 0x94d049bb133111ebULL;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ float* row_ptr(const TableDev& t, unsigned r) {
  if (t.single || (r >> t.chunk_bits) == 0) return t.c0.rows + (size_t)r * t.dim;
  const Chunk& c = t.chunks[r >> t.chunk_bits];
  return c.rows + (size_t)(r & ((1u << t.chunk_bits) - 1)) * t.dim;
}
// the whole slab is chunk 0 (every pre-sized table): rows are c0.rows + r * dim, no chunk-table hop and no branch in
// front of the load — a loop that asks this once keeps all its row loads in flight together
__device__ __forceinline__ bool single_chunk(const TableDev& t) { return t.single != 0u; }
__device__ __forceinline__ RowMeta* meta_ptr(const TableDev& t, unsigned r) {
  if (t.single || (r >> t.chunk_bits) == 0) return t.c0.meta + (size_t)r * META_STRIDE;
  return t.chunks[r >> t.chunk_bits].meta + (size_t)(r & ((1u << t.chunk_bits) - 1)) * META_STRIDE;
}
__device__ __forceinline__ SlotMirror* mirror_ptr(const TableDev& t, unsigned r) {
  return reinterpret_cast<SlotMirror*>(meta_ptr(t, r) + 1);
}
__device__ __forceinline__ unsigned* freq_ptr(const TableDev& t, unsigned r) { return &meta_ptr(t, r)->freq; }
__device__ __forceinline__ unsigned char* flags_ptr(const TableDev& t, unsigned r) { return &meta_ptr(t, r)->flags; }
__device__ __forceinline__ long long* key_ptr(const TableDev& t, unsigned r) { return &meta_ptr(t, r)->key; }
// train_deltalist_.insert(key) (kv_variable.h:316,451,685; MarkAsDeltaListElements :791-799): one byte in the
// row's own RowMeta record, a plain store by the key's single owner thread
__device__ __forceinline__ void mark_delta(const TableDev& t, unsigned r) {
  if (t.track_delta) meta_ptr(t, r)->delta |= (unsigned char)DELTA_TRAIN;
}
// frequency word and flags of a row with ONE 8-byte load: .x = freq word, .y & 0xFF = flags
__device__ __forceinline__ uint2 load_freq_flags(const TableDev& t, unsigned r) {
  return *reinterpret_cast<const uint2*>(&meta_ptr(t, r)->freq);
}

__device__ __forceinline__ Entry load_entry(const Entry* e) {
  const uint4 v = *reinterpret_cast<const uint4*>(e);
  Entry r;
  r.key = (long long)(((unsigned long long)v.y << 32) | v.x);
  r.row = v.z;
  r.hint = v.w;
  return r;
}

// read-only probe; 0 = absent (row 0 is the zero row)
__device__ __forceinline__ unsigned table_find(const TableDev& t, long long key) {
  if (key == EMPTY_KEY) {
    Entry e = load_entry(&t.entries[t.mask + 1]);
    return (e.key == 0 && e.row != ROW_TOMB) ? e.row : 0u;
  }
  unsigned long long p = mix64((unsigned long long)key) & t.mask;
  for (;;) {
    Entry e = load_entry(&t.entries[p]);
    if (e.key == key) return e.row != ROW_TOMB ? e.row : 0u;
    if (e.key == EMPTY_KEY) return 0u;
    p = (p + 1) & t.mask;
  }
}

// read-only probe continuing from an entry the caller already loaded (so the first loads of
// several tables can be in flight together)
__device__ __forceinline__ unsigned table_find_from(const TableDev& t, long long key, unsigned long long p,
                                                   Entry e, unsigned* hint = nullptr) {
  if (key == EMPTY_KEY) {
    if (hint) *hint = e.hint;
    return (e.key == 0 && e.row != ROW_TOMB) ? e.row : 0u;
  }
  for (;;) {
    if (e.key == key) {
      if (hint) *hint = e.hint;
      return e.row != ROW_TOMB ? e.row : 0u;
    }
    if (e.key == EMPTY_KEY) return 0u;
    p = (p + 1) & t.mask;
    e = load_entry(&t.entries[p]);
  }
}
// index entry of a key that is present (nullptr when absent): where its slot-row hint lives
__device__ __forceinline__ Entry* table_entry_of(const TableDev& t, long long key) {
  if (key == EMPTY_KEY) {
    Entry* s = &t.entries[t.mask + 1];
    return load_entry(s).key == 0 ? s : nullptr;
  }
  unsigned long long p = mix64((unsigned long long)key) & t.mask;
  for (;;) {
    Entry* s = &t.entries[p];
    const Entry e = load_entry(s);
    if (e.key == key) return s;
    if (e.key == EMPTY_KEY) return nullptr;
    p = (p + 1) & t.mask;
  }
}
__device__ __forceinline__ unsigned long long home_of(const TableDev& t, long long key, unsigned long long h) {
  return key == EMPTY_KEY ? t.mask + 1 : (h & t.mask);
}

// a batch that cannot be processed (see report_deferred_error in kvhip.hip): device flag for the kernels
// that follow in the same op, pinned host word for the next call
__device__ __forceinline__ void raise_error(const TableDev& t, unsigned code) {
  atomicExch(&t.counters[1], code);
  if (t.err_host) __hip_atomic_store(t.err_host, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Find or insert.  The caller is the ONLY lane of the launch that handles `key` (batch
// dedup guarantees it), so a freshly claimed entry is never read by anyone else before the
// kernel ends; other keys racing for the same empty entry are settled by the 64-bit CAS.
// Returns the row id; *inserted tells whether it was allocated now.  Returns 0 and raises
// counters[1] when the slab is full (the host pre-sizes, so this is a bug trap).
__device__ __forceinline__ unsigned table_find_or_insert(const TableDev& t, long long key,
                                                        bool* inserted) {
  *inserted = false;
  Entry* slot;
  long long stored;
  if (key == EMPTY_KEY) {
    slot = &t.entries[t.mask + 1];
    stored = 0;  // the sentinel's home holds 0 when occupied
    Entry e = load_entry(slot);
    if (e.key == stored) {
      if (e.row != ROW_TOMB) return e.row;
      goto claimed;  // deleted earlier: the entry is still this key's, give it a row again
    }
  } else {
    stored = key;
    unsigned long long p = mix64((unsigned long long)key) & t.mask;
    for (;;) {
      slot = &t.entries[p];
      Entry e = load_entry(slot);
      if (e.key == key) {
        if (e.row != ROW_TOMB) return e.row;
        goto claimed;
      }
      if (e.key == EMPTY_KEY) {
        unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&slot->key),
                                           (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (old == (unsigned long long)EMPTY_KEY) goto claimed;
        // another key took it between our load and the CAS: keep probing
      }
      p = (p + 1) & t.mask;
    }
  }
  {
    unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&slot->key),
                                       (unsigned long long)EMPTY_KEY, (unsigned long long)stored);
    if (old != (unsigned long long)EMPTY_KEY) return load_entry(slot).row;  // cannot happen (single owner)
  }
claimed:
  unsigned r = 0;
  bool have = false;
  if (t.free_rows) {  // rows released by Delete first (pops only: Delete never runs beside an insert)
    const int f = atomicSub(reinterpret_cast<int*>(&t.counters[2]), 1);
    if (f > 0) { r = t.free_rows[f - 1]; have = true; }
    else atomicAdd(reinterpret_cast<int*>(&t.counters[2]), 1);
  }
  if (!have) {
    r = atomicAdd(&t.counters[0], 1u);
    if (r >= t.max_rows) {
      raise_error(t, 1u);
      slot->row = 0;
      return 0u;
    }
  }
  slot->row = r;
  *key_ptr(t, r) = key;
  { RowMeta* nm = meta_ptr(t, r); nm->delta = 0; nm->stamp = 0; }  // fresh (or recycled) row: in no delta list yet
  *inserted = true;
  return r;
}

// kv_variable.h:889-898 GenerateRandomInitialValue: row = 0.5 * (T[r1] + T[r2]).  The
// reference draws r1, r2 from std::rand(); here they are a hash of (key, seed) so a run is
// reproducible.  init_rule_rows: the two rows of the init table for `key`.
// (D = t.dim, handed over by init_var_row, which holds it in a register as the apply bodies always did)
__device__ __forceinline__ void init_rule_rows(const TableDev& t, long long key, const float** ia, const float** ib, int D) {
  const unsigned long long h = pick64((unsigned long long)key ^ (t.seed * 0x9E3779B97F4A7C15ULL));
  *ia = t.init_table + (size_t)((unsigned)h % t.init_rows) * D;
  *ib = t.init_table + (size_t)((unsigned)(h >> 32) % t.init_rows) * D;
}
__device__ __forceinline__ void init_rule_rows(const TableDev& t, long long key, const float** ia, const float** ib) {
  init_rule_rows(t, key, ia, ib, t.dim);
}
// The init rule's row written to dst by `lanes` cooperating lanes (lane = 0..lanes-1).  Returns
// whether this lane saw any |x| >= CUTOFF.
__device__ __forceinline__ bool init_row_coop(const TableDev& t, long long key, float* dst,
                                              int lane, int lanes) {
  const float *a, *b;
  init_rule_rows(t, key, &a, &b);
  bool big = false;
  for (int e = lane; e < t.dim; e += lanes) {
    float v = (a[e] + b[e]) * 0.5f;
    dst[e] = v;
    big |= fabsf(v) >= CUTOFF;
  }
  return big;
}

// partition that owns a key (top bits of the hash; table probes use the low bits)
__device__ __forceinline__ unsigned part_of(long long key, int pshift) {
  return pshift >= 64 ? 0u : (unsigned)(mix64((unsigned long long)key) >> pshift);
}

// exclusive scan of one value per thread across the block (NW = waves per block);
// wtot: LDS scratch [NW + 1]; returns the exclusive prefix, *total = block sum.
// A barrier that orders LDS only.  __syncthreads() also waits for the wave's outstanding GLOBAL loads (its fence
// drains vmcnt), which exposes the latency of loads requested ahead of time (index probes, id loads) at the first
// barrier behind them.  Where every hand-over between the waves goes through LDS, this one lets them stay in flight.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDSONLY: barriers that leave global loads in flight (lds_barrier)
template <int NW, bool LDSONLY = false>
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* wtot, unsigned* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl_up(incl, o);
    if (lane >= o) incl += x;
  }
  if (LDSONLY) lds_barrier(); else __syncthreads();  // wtot may still be read from a previous scan
  if (lane == 63) wtot[wv] = incl;
  if (LDSONLY) lds_barrier(); else __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const unsigned x = wtot[i];
    if (i < wv) base += x;
    tot += x;
  }
  *total = tot;
  return base + incl - v;
}

template <typename IdT>
__device__ __forceinline__ long long load_id(const IdT* ids, size_t i) {
  return (long long)ids[i];
}
// (id, occurrence count) pairs as the sharded exchange delivers them (kv_bucket_by_owner pairs_out)
struct IdCount { long long id, count; };
template <>
__device__ __forceinline__ long long load_id<IdCount>(const IdCount* ids, size_t i) { return ids[i].id; }

// sqrt and division of the row math.  fast: one v_sqrt_f32 / v_rcp_f32 (1 ulp each: the update stays within north_star's
// 1e-6 relative of the reference's correctly rounded Eigen arithmetic); else the IEEE sequences (bit-for-bit the
// oracle's results: the deterministic mode and every table that asks for it keep them).  `fast` is uniform over the launch.
#ifdef KV_FASTM_CONST
#define KV_FASTM(a) (KV_FASTM_CONST != 0)
#else
#define KV_FASTM(a) ((a).fast != 0)
#endif
__device__ __forceinline__ float kv_sqrt(float x, bool fast) { return fast ? __builtin_amdgcn_sqrtf(x) : sqrtf(x); }
__device__ __forceinline__ float kv_div(float x, float y, bool fast) { return fast ? x * __builtin_amdgcn_rcpf(y) : x / y; }

// optimizer-side slot-table access: FindOrInsertUnsafe(filter_out == nullptr), kv_variable.h:382-416.
// Called by the group leader only.  New rows get freq word 1 (day 0); hits AddFrequency(1, today).
__device__ __forceinline__ unsigned slot_find_or_insert(const TableDev& t, long long key,
                                                       unsigned day, bool* inserted) {
  unsigned r = table_find_or_insert(t, key, inserted);
  if (r == 0) return 0;
  unsigned* fp = freq_ptr(t, r);
  if (*inserted) {
    *fp = 1u;
  } else {
    unsigned lo = (*fp & 0xFFFFu) + 1u;
    if (lo > 65535u) lo = 65535u;
    *fp = (day << 16) | lo;
  }
  return r;
}

// V-wide row access (V = 4: one 16-byte access per lane; V = 1: scalar)
template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
  if (V == 4) {
    const float4 t4 = *reinterpret_cast<const float4*>(p);
    o[0] = t4.x; o[1 % V] = t4.y; o[2 % V] = t4.z; o[3 % V] = t4.w;
  } else {
    o[0] = p[0];
  }
}
// same, for data this launch reads exactly once (gradient rows): streaming load, so the table rows
// and the partition lists keep the L2 / infinity cache
template <int V>
__device__ __forceinline__ void ldv_stream(const float* p, float (&o)[V]) {
#pragma unroll
  for (int c = 0; c < V; ++c) o[c] = __builtin_nontemporal_load(p + c);
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&o)[V]) {
  if (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
  } else {
    p[0] = o[0];
  }
}
// slot row element block: existing row, or the init rule 0.5 * (T[r1] + T[r2]) for a new key
template <int V>
__device__ __forceinline__ void ldslot(const float* row, const float* ia, const float* ib, bool isnew,
                                       int e, float (&o)[V]) {
  if (isnew) {
    float a[V], b[V];
    ldv<V>(ia + e, a);
    ldv<V>(ib + e, b);
#pragma unroll
    for (int c = 0; c < V; ++c) o[c] = (a[c] + b[c]) * 0.5f;
  } else {
    ldv<V>(row + e, o);
  }
}

template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}
template <int W>
__device__ __forceinline__ bool group_any(bool p) {
  const unsigned long long m = __ballot(p);
  if (W >= 64) return m != 0;
  const int lane = threadIdx.x & 63;
  const unsigned long long gm = (W >= 64) ? ~0ull : ((1ull << W) - 1ull);
  return ((m >> (lane & ~(W - 1))) & gm) != 0;
}

// One unique key's fused optimizer update, executed by LPR cooperating lanes (lane = 0..LPR-1).
// `tag` = var row id | ROW_FILTERED; gv = the key's summed gradient, element e at lane
// (e / V) % LPR, step (e / V) / LPR.  All LPR lanes of every group in the wave must call it
// (shuffles inside); `live` masks groups without a key.  r0 / r1 (+ new flags) are the slot-table
// rows the group leader probed (probe_for_apply).
// Restates the per-id body of KvVariableGroupSparseApplyAdamV4Op / V3Op / SparseApplyAdagradOp /
// SparseGroupSparseApplyFtrlOp (training_ops.cc:7142-7197, 5871-5927, 1455-1486, 684-763).
// State rows the caller already holds (requested together with the gradient rows, so the update needs no
// second round trip): x = the var row; s[0 .. slot0_blocks(OPT)) = the first slot table's row in blocks of dim floats
// (GroupAdam m | v | z; group RectifiedAdam m | v | linear | vhat | vamsgrad; Adam m | v; Adagrad / FTRL accum in s[0]).  have_x /
// have_s say which of them are valid.  (s has opt_core's width, state_blocks(OPT): the lean paths hand it over as it is.)
template <int OPT, int V, int K>
struct PreRows {
  float x[K][V], s[state_blocks(OPT)][K][V];
};
// The row math and the stores of one key's update, on values the caller already holds: xin = the var row;
// sin = GroupAdam m | v | z, group RectifiedAdam m | v | linear | vhat | vamsgrad, Adam m | v, Adagrad accum, FTRL accum | linear.
// Element e of a row lives at lane
// (e / V) % LPR, step (e / V) / LPR.  All LPR lanes of every group of the wave call it (shuffles inside); `act`
// masks groups without an update.  fvp / f0p / f1p = the flag bytes of the var / first / second slot row.
// new1 = the second slot row was inserted now (its flags come from its values).  vblack / sblack (scatter_chain(OPT)
// only): the var / slot row is blacklisted — it reads as zeros where it is read and is left as it is.
// Restates the per-id body of KvVariableGroupSparseApplyAdamV4Op / V3Op / SparseApplyAdagradOp /
// SparseGroupSparseApplyFtrlOp / SparseApplyFtrlOp / GroupSparseApplyFtrlOp / GroupSparseApplyRectifiedAdamOp
// (training_ops.cc:7142-7197, 5871-5927, 1455-1486, 684-763, 457-484, 977-1019, 6883-6936) and, for Adam, the row
// arithmetic of the reference's Python composition (python/training/adam.py:93-163).
template <int OPT, int V, int LPR, int K>
__device__ __forceinline__ void opt_core(float* xrow, float* s0row, float* s1row, unsigned char* fvp, unsigned char* f0p,
                                         unsigned char* f1p, bool act, bool new0, int D, const float (&gv)[K][V],
                                         const OptArgs& a, int lane, const float (&xin)[K][V],
                                         const float (&sin)[state_blocks(OPT)][K][V], bool new1 = false, bool vblack = false,
                                         bool sblack = false) {
  static_assert(OPT >= OPT_ADAM_V4 && OPT <= OPT_ADAM, "opt_core: unknown optimizer");
  if (group_adam(OPT)) {
    // training_ops.cc:7166-7195 (V4) / :5895-5925 (V3); slot row = [m | v | z]
    float m[K][V], nv[K][V], sq[K][V], z[K][V], uu[K][V];
    float part = 0.f;
    const float omb1 = 1.f - a.b1, omb2 = 1.f - a.b2;
    const bool fm = KV_FASTM(a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      const bool valid = act && e0 < D;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float xo = valid ? xin[k][c] : 0.f, mo = valid ? sin[0][k][c] : 0.f;
        const float vo = valid ? sin[1][k][c] : 0.f, zo = valid ? sin[2][k][c] : 0.f;
        const float gg = gv[k][c];
        const float mn = a.b1 * mo + omb1 * gg;
        const float vn = a.b2 * vo + omb2 * (gg * gg);
        const float s = kv_sqrt(vn, fm);
        float d;
        if (OPT == OPT_ADAM_V4) {
          d = (a.b1 > a.b1p) ? (s - kv_sqrt(vo, fm)) * xo : (s + a.eps) * xo;
        } else {
          d = (a.b1 > a.b1p) ? kv_div(s - kv_sqrt(vo, fm), a.lr, fm) * xo
                             : kv_div(s - kv_sqrt(vo, fm) + a.eps, a.lr, fm) * xo;
        }
        const float zn = zo + (a.alpha * mn - d);
        const float adj = fmaxf(fminf(zn, a.l1), -a.l1);
        const float uv = adj - zn;
        m[k][c] = mn; nv[k][c] = vn; sq[k][c] = s; z[k][c] = zn; uu[k][c] = uv;
        if (valid) part += uv * uv;
      }
    }
    const float norm = kv_sqrt(group_sum<LPR>(part), fm);
    const bool upd = norm > a.l21_norm;
    const float scale = 1.f - kv_div(a.l21_norm, norm, fm);
    const float two_l2 = 2.f * a.l2;
    bool big = false, sbig = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          xn[c] = 0.f;  // blacklist: the row reads as zeros (table_manager.h:335-357)
          if (upd) {
            const float y = (OPT == OPT_ADAM_V4) ? (sq[k][c] + a.eps) + two_l2
                                                 : kv_div(sq[k][c] + a.eps, a.lr, fm) + two_l2;
            xn[c] = kv_div(uu[k][c] * scale, y, fm);
          }
          big |= fabsf(xn[c]) >= CUTOFF;
          sbig |= fabsf(m[k][c]) >= CUTOFF || fabsf(nv[k][c]) >= CUTOFF || fabsf(z[k][c]) >= CUTOFF;
        }
        stv<V>(xrow + e0, xn);
        stv<V>(s0row + e0, m[k]);
        stv<V>(s0row + e0 + D, nv[k]);
        stv<V>(s0row + e0 + 2 * D, z[k]);
      }
    }
    const bool anyx = group_any<LPR>(big), anys = group_any<LPR>(sbig);
    if (act && lane == 0) {
      // CoverUpdateUnsafe -> UpdateUnderThreshold, or MarkBlacklistUnsafe (:7187-7195)
      *fvp = (unsigned char)(upd ? (anyx ? 0u : FLAG_UNDER) : (FLAG_BLACK | FLAG_UNDER));
      *f0p = (unsigned char)(anys ? 0u : FLAG_UNDER);
    }
  } else if (OPT == OPT_ADAGRAD) {
    // training_ops.cc:1470-1482.  No CoverUpdate: flags of existing rows are left alone.
    bool sbig = false;
    const bool fm = KV_FASTM(a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xo[V], acc[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          xo[c] = xin[k][c]; acc[c] = sin[0][k][c];
          const float gg = gv[k][c];
          sbig |= fabsf(acc[c]) >= CUTOFF;
          if (a.update_slots) acc[c] = acc[c] + gg * gg;
          if (fm) xo[c] = xo[c] - (a.lr * gg) * __builtin_amdgcn_rsqf(acc[c]);
          else xo[c] = (D > 1) ? xo[c] - (a.lr * gg) * (1.f / sqrtf(acc[c]))
                               : xo[c] - (a.lr * gg) / sqrtf(acc[c]);
        }
        stv<V>(xrow + e0, xo);
        stv<V>(s0row + e0, acc);
      }
    }
    const bool anys = group_any<LPR>(sbig);
    if (act && lane == 0) {
      // the reference does not refresh under_threshold here; a later lookup does (FLAG_DIRTY)
      *fvp |= (unsigned char)FLAG_DIRTY;
      if (new0) *f0p = (unsigned char)((anys ? 0u : FLAG_UNDER) | (a.update_slots ? FLAG_DIRTY : 0u));
      else if (a.update_slots) *f0p |= (unsigned char)FLAG_DIRTY;
    }
  } else if (OPT == OPT_FTRL) {
    // OPT_FTRL: training_ops.cc:713-751 with has_l2_shrinkage; slot 0 = accum, slot 1 = linear
    float x[K][V], ac[K][V], z[K][V], uu[K][V];
    float part = 0.f;
    const bool half = a.lr_power == -0.5f;
    const float two_l2s = 2.f * a.l2s;
    const bool fm = KV_FASTM(a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      const bool valid = act && e0 < D;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        x[k][c] = valid ? xin[k][c] : 0.f; ac[k][c] = valid ? sin[0][k][c] : 0.f;
        const float zo = valid ? sin[1][k][c] : 0.f;
        const float xo = x[k][c], ao = ac[k][c];
        const float gs = gv[k][c] + two_l2s * xo;
        const float na = ao + gs * gs;
        const float pn = half ? kv_sqrt(na, fm) : powf(na, -a.lr_power);
        const float po = half ? kv_sqrt(ao, fm) : powf(ao, -a.lr_power);
        const float zn = zo + (gs - kv_div(pn - po, a.lr, fm) * xo);
        const float adj = fmaxf(fminf(zn, a.l1), -a.l1);
        const float uv = adj - zn;
        z[k][c] = zn; uu[k][c] = uv;
        if (valid) part += uv * uv;
      }
    }
    const float norm = kv_sqrt(group_sum<LPR>(part), fm);
    const bool upd = norm > a.l21_norm;
    const float scale = 1.f - kv_div(a.l21_norm, norm, fm);
    const float two_l2 = 2.f * a.l2;
    bool big = false, abig = false, zbig = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V], an[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float xo = x[k][c];
          const float gs = gv[k][c] + two_l2s * xo;
          const float na = ac[k][c] + gs * gs;
          const float pn = half ? kv_sqrt(na, fm) : powf(na, -a.lr_power);
          xn[c] = 0.f;
          if (upd) xn[c] = kv_div(uu[k][c] * scale, kv_div(pn, a.lr, fm) + two_l2, fm);
          // accum += grad_to_use.square() re-evaluates the lazy expression with the updated
          // var (:747); on the blacklist branch the reference reads a freed row — we keep
          // the pre-blacklist value like oracle/kv_oracle.cc
          const float xa = upd ? xn[c] : xo;
          const float gs2 = gv[k][c] + two_l2s * xa;
          an[c] = ac[k][c] + gs2 * gs2;
          big |= fabsf(xn[c]) >= CUTOFF;
          abig |= fabsf(an[c]) >= CUTOFF;
          zbig |= fabsf(z[k][c]) >= CUTOFF;
        }
        stv<V>(xrow + e0, xn);
        stv<V>(s0row + e0, an);
        stv<V>(s1row + e0, z[k]);
      }
    }
    const bool anyx = group_any<LPR>(big), anya = group_any<LPR>(abig), anyz = group_any<LPR>(zbig);
    if (act && lane == 0) {
      *fvp = (unsigned char)(upd ? (anyx ? 0u : FLAG_UNDER) : (FLAG_BLACK | FLAG_UNDER));
      *f0p = (unsigned char)(anya ? 0u : FLAG_UNDER);
      *f1p = (unsigned char)(anyz ? 0u : FLAG_UNDER);
    }
  } else if (OPT == OPT_FTRL_V2) {
    // KvVariableSparseApplyFtrlV2, training_ops.cc:457-484 with has_l2_shrinkage; slot 0 = accum, slot 1 = linear.
    // Element-wise FTRL-Proximal: no norm, no CoverUpdate and no blacklist (flags as the Adagrad branch treats them)
    const bool half = a.lr_power == -0.5f;
    const float two_l2s = 2.f * a.l2s, two_l2 = 2.f * a.l2;
    const bool fm = KV_FASTM(a);
    bool abig = false, zbig = false;   // the slot rows' values before the update: what a new row's flags come from
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V], an[V], zn[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float xo = xin[k][c], ao = sin[0][k][c], zo = sin[1][k][c];
          abig |= fabsf(ao) >= CUTOFF;
          zbig |= fabsf(zo) >= CUTOFF;
          const float gs = gv[k][c] + two_l2s * xo;
          const float na = ao + gs * gs;
          const float pn = half ? kv_sqrt(na, fm) : powf(na, -a.lr_power);
          const float po = half ? kv_sqrt(ao, fm) : powf(ao, -a.lr_power);
          zn[c] = zo + (gs - kv_div(pn - po, a.lr, fm) * xo);
          const float adj = fmaxf(fminf(zn[c], a.l1), -a.l1);
          xn[c] = kv_div(adj - zn[c], kv_div(pn, a.lr, fm) + two_l2, fm);
          // accum += grad_to_use.square() re-evaluates the lazy expression with the updated var (:484)
          const float gs2 = gv[k][c] + two_l2s * xn[c];
          an[c] = ao + gs2 * gs2;
        }
        stv<V>(xrow + e0, xn);
        stv<V>(s0row + e0, an);
        stv<V>(s1row + e0, zn);
      }
    }
    const bool anya = group_any<LPR>(abig), anyz = group_any<LPR>(zbig);
    if (act && lane == 0) {
      // the reference does not refresh under_threshold here; a later lookup does (FLAG_DIRTY)
      *fvp |= (unsigned char)FLAG_DIRTY;
      if (new0) *f0p = (unsigned char)((anya ? 0u : FLAG_UNDER) | FLAG_DIRTY);
      else *f0p |= (unsigned char)FLAG_DIRTY;
      if (new1) *f1p = (unsigned char)((anyz ? 0u : FLAG_UNDER) | FLAG_DIRTY);
      else *f1p |= (unsigned char)FLAG_DIRTY;
    }
  } else if (OPT == OPT_GROUP_FTRL_V2) {
    // OPT_GROUP_FTRL_V2: KvVariableGroupSparseApplyFtrlV2, training_ops.cc:977-1019 with has_l2_shrinkage; slot 0 = accum,
    // slot 1 = linear.  Group lasso with threshold l1 on the whole updated linear row
    float z[K][V];
    float part = 0.f;
    const bool half = a.lr_power == -0.5f;
    const float two_l2s = 2.f * a.l2s, two_l2 = 2.f * a.l2;
    const bool fm = KV_FASTM(a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      const bool valid = act && e0 < D;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float xo = valid ? xin[k][c] : 0.f, ao = valid ? sin[0][k][c] : 0.f, zo = valid ? sin[1][k][c] : 0.f;
        const float gs = gv[k][c] + two_l2s * xo;
        const float na = ao + gs * gs;
        const float pn = half ? kv_sqrt(na, fm) : powf(na, -a.lr_power);
        const float po = half ? kv_sqrt(ao, fm) : powf(ao, -a.lr_power);
        z[k][c] = zo + (gs - kv_div(pn - po, a.lr, fm) * xo);
        if (valid) part += z[k][c] * z[k][c];
      }
    }
    const float norm = kv_sqrt(group_sum<LPR>(part), fm);   // linear.square().sum().sqrt() (:994)
    const bool upd = norm > a.l1;
    const float l1mn = a.l1 - norm;
    bool big = false, abig = false, zbig = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V], an[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float xo = xin[k][c], ao = sin[0][k][c];
          xn[c] = 0.f;   // blacklist: the row reads as zeros (table_manager.h:335-357)
          if (upd) {
            const float gs = gv[k][c] + two_l2s * xo;
            const float na = ao + gs * gs;
            const float pn = half ? kv_sqrt(na, fm) : powf(na, -a.lr_power);
            const float coef = kv_div(l1mn, (kv_div(pn, a.lr, fm) + two_l2) * norm, fm);
            xn[c] = coef * z[k][c];
          }
          // accum += grad_to_use.square(), TWICE (:1015-1016), each re-evaluating the lazy expression with the updated
          // var; on the blacklist branch we keep the pre-blacklist value like the SparseGroupFtrl branch above
          const float xa = upd ? xn[c] : xo;
          const float gs2 = gv[k][c] + two_l2s * xa;
          const float g2 = gs2 * gs2;
          an[c] = (ao + g2) + g2;
          big |= fabsf(xn[c]) >= CUTOFF;
          abig |= fabsf(an[c]) >= CUTOFF;
          zbig |= fabsf(z[k][c]) >= CUTOFF;
        }
        stv<V>(xrow + e0, xn);
        stv<V>(s0row + e0, an);
        stv<V>(s1row + e0, z[k]);
      }
    }
    const bool anyx = group_any<LPR>(big), anya = group_any<LPR>(abig), anyz = group_any<LPR>(zbig);
    if (act && lane == 0) {
      // CoverUpdateUnsafe or MarkBlacklistUnsafe on the var; CoverUpdateUnsafe on linear and accum (:1003-1021)
      *fvp = (unsigned char)(upd ? (anyx ? 0u : FLAG_UNDER) : (FLAG_BLACK | FLAG_UNDER));
      *f0p = (unsigned char)(anya ? 0u : FLAG_UNDER);
      *f1p = (unsigned char)(anyz ? 0u : FLAG_UNDER);
    }
  } else if (OPT == OPT_GROUP_RADAM) {
    // OPT_GROUP_RADAM: KvVariableGroupSparseApplyRectifiedAdam, training_ops.cc:6883-6936; slot row =
    // [m | v | linear | vhat | vamsgrad].  a.alpha = sqrt(1 - beta2_power), radam_c1(a) = 1 - beta1_power (host, fp32).
    // m_corr is a copy of m's TensorMap (FlatVector, :195): the nesterov assignment writes m itself
    constexpr int NB = slot0_blocks(OPT);
    float m[K][V], nv[K][V], rv[K][V], z[K][V], uu[K][V], va[K][V];
    float part = 0.f;
    const float omb1 = 1.f - a.b1, omb2 = 1.f - a.b2;
    const bool fm = KV_FASTM(a);
    const bool tract = (radam_flags(a) & RADAM_TRACTABLE) != 0, ams = (radam_flags(a) & RADAM_AMSGRAD) != 0;
    const bool nest = (radam_flags(a) & RADAM_NESTEROV) != 0;
    const float inv_lr = kv_div(1.f, a.lr, fm);   // v.constant(1) / lr (:6896)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      const bool valid = act && e0 < D;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float xo = valid ? xin[k][c] : 0.f, mo = valid ? sin[0][k][c] : 0.f, vo = valid ? sin[1][k][c] : 0.f;
        const float zo = valid ? sin[2][k][c] : 0.f, vh = valid ? sin[3][k][c] : 0.f;
        float vam = valid ? sin[4][k][c] : 0.f;
        const float gg = gv[k][c];
        float mn = a.b1 * mo + omb1 * gg;
        const float vn = a.b2 * vo + omb2 * (gg * gg);
        if (nest) mn = gg * omb1 + a.b1 * mn;
        float rm, r;
        if (!tract) {
          rm = kv_div(mn, radam_c1(a), fm);
          r = inv_lr;
        } else {
          if (ams) vam = fmaxf(vn, vam);
          rm = kv_div(radam_r_t(a) * mn, radam_c1(a), fm);
          r = kv_div(kv_div(kv_sqrt(ams ? vam : vn, fm), a.alpha, fm) + a.eps, a.lr, fm);
        }
        const float zn = zo + (rm - (r - vh) * xo);
        const float adj = fmaxf(fminf(zn, a.l1), -a.l1);
        const float uv = adj - zn;
        m[k][c] = mn; nv[k][c] = vn; rv[k][c] = r; z[k][c] = zn; uu[k][c] = uv; va[k][c] = vam;
        if (valid) part += uv * uv;
      }
    }
    const float norm = kv_sqrt(group_sum<LPR>(part), fm);
    const bool upd = norm > a.l21_norm;
    const float scale = 1.f - kv_div(a.l21_norm, norm, fm);
    const float two_l2 = 2.f * a.l2;
    bool big = false, sbig = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          xn[c] = 0.f;  // blacklist: the row reads as zeros (table_manager.h:335-357)
          if (upd) xn[c] = kv_div(uu[k][c] * scale, rv[k][c] + two_l2, fm);
          big |= fabsf(xn[c]) >= CUTOFF;
          sbig |= fabsf(m[k][c]) >= CUTOFF || fabsf(nv[k][c]) >= CUTOFF || fabsf(z[k][c]) >= CUTOFF ||
                  fabsf(rv[k][c]) >= CUTOFF || fabsf(va[k][c]) >= CUTOFF;
        }
        stv<V>(xrow + e0, xn);
        stv<V>(s0row + e0, m[k]);
        stv<V>(s0row + e0 + D, nv[k]);
        stv<V>(s0row + e0 + 2 * D, z[k]);
        stv<V>(s0row + e0 + 3 * D, rv[k]);
        // vamsgrad is assigned in the amsgrad branch only (:6901); a row inserted now gets its init value written
        if ((tract && ams) || new0) stv<V>(s0row + e0 + (NB - 1) * D, va[k]);
      }
    }
    const bool anyx = group_any<LPR>(big), anys = group_any<LPR>(sbig);
    if (act && lane == 0) {
      // CoverUpdateUnsafe -> UpdateUnderThreshold, or MarkBlacklistUnsafe (:6923-6936)
      *fvp = (unsigned char)(upd ? (anyx ? 0u : FLAG_UNDER) : (FLAG_BLACK | FLAG_UNDER));
      *f0p = (unsigned char)(anys ? 0u : FLAG_UNDER);
    }
  } else {
    // OPT_ADAM: python/training/adam.py:93-163 on one de-duplicated id; slot row = [m | v].  a.alpha = lr_t =
    // lr sqrt(1 - beta2_power) / (1 - beta1_power), adam_omb1 / adam_omb2 = 1 - beta1 / 1 - beta2 (host, fp32).  One pass:
    // nothing couples the elements of a row, so no value outlives its element block.  The gather hands a blacklisted slot
    // row over as zeros (table_manager.h:224-226) and neither scatter writes a blacklisted row (kv_variable.h:700-712)
    bool big = false, sbig = false;
    const bool fm = KV_FASTM(a);
    const float omb1 = adam_omb1(a), omb2 = adam_omb2(a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (act && e0 < D) {
        float xn[V], mn[V], vn[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const float mo = sblack ? 0.f : sin[0][k][c], vo = sblack ? 0.f : sin[1][k][c];
          const float gg = gv[k][c];
          mn[c] = a.b1 * mo + gg * omb1;
          vn[c] = a.b2 * vo + (gg * gg) * omb2;
          xn[c] = xin[k][c] - kv_div(a.alpha * mn[c], a.eps + kv_sqrt(vn[c], fm), fm);
          big |= fabsf(xn[c]) >= CUTOFF;
          sbig |= fabsf(mn[c]) >= CUTOFF || fabsf(vn[c]) >= CUTOFF;
        }
        if (!vblack) stv<V>(xrow + e0, xn);
        if (!sblack) {
          stv<V>(s0row + e0, mn);
          stv<V>(s0row + e0 + D, vn);
        }
      }
    }
    const bool anyx = group_any<LPR>(big), anys = group_any<LPR>(sbig);
    if (act && lane == 0) {
      // UpdateUnderThreshold on the rows written (kv_variable.h:706, 837-861); a blacklisted row keeps its flags
      if (!vblack) *fvp = (unsigned char)(anyx ? 0u : FLAG_UNDER);
      if (!sblack) *f0p = (unsigned char)(anys ? 0u : FLAG_UNDER);
    }
  }
}

// One unique key's fused optimizer update through the tables: resolves the row pointers, loads (or initialises, for
// a slot row inserted now) the state rows the caller does not hold yet, then opt_core.
template <int OPT, int V, int LPR, int K>
__device__ __forceinline__ void opt_update_row(const TableDev& tv, const TableDev& ts0,
                                               const TableDev& ts1, long long key, unsigned tag,
                                               unsigned r0, bool new0, unsigned r1, bool new1,
                                               bool live, const float (&gv)[K][V], const OptArgs& a,
                                               int lane, const PreRows<OPT, V, K>* pre = nullptr, bool have_x = false,
                                               bool have_s = false, bool vblack = false, bool sblack = false) {
  const int D = tv.dim;
  const bool skip = !live || (tag & ROW_FILTERED) || (tag & ROW_MASK) == 0u;  // training_ops.cc:7150-7152
  const unsigned rv = tag & ROW_MASK;
  const bool act = !skip && r0 != 0 && (!two_slots(OPT) || r1 != 0);

  float* xrow = row_ptr(tv, act ? rv : 0u);
  float* s0row = row_ptr(ts0, act ? r0 : 0u);
  float* s1row = two_slots(OPT) ? row_ptr(ts1, act ? r1 : 0u) : nullptr;

  // new slot rows are initialised in registers with the slot table's init rule
  const float *ia0 = nullptr, *ib0 = nullptr, *ia1 = nullptr, *ib1 = nullptr;
  if (act && new0) init_rule_rows(ts0, key, &ia0, &ib0);
  if (two_slots(OPT) && act && new1) init_rule_rows(ts1, key, &ia1, &ib1);
  constexpr int NS0 = slot0_blocks(OPT), NSB = state_blocks(OPT);
  float xin[K][V], sin[NSB][K][V];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (lane + k * LPR) * V;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      // (blocks 0..2 in one statement, as they always were: the FTRL kernels' register allocation follows it — tools/kres.sh)
      xin[k][c] = sin[0][k][c] = sin[1][k][c] = sin[2][k][c] = 0.f;
#pragma unroll
      for (int b3 = 3; b3 < NSB; ++b3) sin[b3][k][c] = 0.f;
    }
    if (!(act && e0 < D)) continue;
    if (pre && have_x) {
#pragma unroll
      for (int c = 0; c < V; ++c) xin[k][c] = pre->x[k][c];
    } else {
      ldv<V>(xrow + e0, xin[k]);
    }
    if (pre && have_s && !new0) {
#pragma unroll
      for (int b3 = 0; b3 < NS0; ++b3)
#pragma unroll
        for (int c = 0; c < V; ++c) sin[b3][k][c] = pre->s[b3][k][c];
    } else {
      // (blocks 0..2 as the statements they always were: one unrolled loop over all blocks gives the GroupAdam kernels
      // another register allocation — tools/kres.sh)
      ldslot<V>(s0row, ia0, ib0, new0, e0, sin[0][k]);
      if (NS0 > 1) {
        ldslot<V>(s0row, ia0, ib0, new0, e0 + D, sin[1][k]);
        if (NS0 > 2) ldslot<V>(s0row, ia0, ib0, new0, e0 + 2 * D, sin[2][k]);   // (Adam's row ends after two blocks)
      }
#pragma unroll
      for (int b3 = 3; b3 < NS0; ++b3) ldslot<V>(s0row, ia0, ib0, new0, e0 + b3 * D, sin[b3][k]);
    }
    if (two_slots(OPT)) ldslot<V>(s1row, ia1, ib1, new1, e0, sin[1][k]);
  }
  opt_core<OPT, V, LPR, K>(xrow, s0row, s1row, flags_ptr(tv, act ? rv : 0u), flags_ptr(ts0, act ? r0 : 0u),
                           two_slots(OPT) ? flags_ptr(ts1, act ? r1 : 0u) : nullptr, act, new0, D, gv, a, lane, xin, sin, new1, vblack,
                           sblack);
}

// ------------------------------------------------------------------------------------------
// multi-GPU routing: stable-by-tile counting sort of ids by owner rank = floor_mod(id, world)
// (kernels/utility.h:90-107).  world <= 64.  hist is [world][ntiles] (owner-major for the scan).
// ------------------------------------------------------------------------------------------
constexpr int RT = 1024;  // ids per routing tile (256 threads x 4)
constexpr int MAXW = 64;

// rule 0 (default): (mix64(id) >> 32) % world — balanced whatever the ids look like; rule 1: floor_mod(id, world), the
// reference's `ids % num_shards` (python/ops/embedding_ops.py:121-127), for checkpoint compatibility
__device__ __forceinline__ unsigned owner_rank(long long id, int world, int rule) {
  // (the HIGH half of the hash: the index's home slot is mix64(key) & mask — with the low bits every key of a rank
  // would share its low home-slot bits and the probe chains of a rank's table would cluster)
  if (rule == 0) return (unsigned)((mix64((unsigned long long)id) >> 32) % (unsigned long long)world);
  long long m = id % world;
  return (unsigned)(m < 0 ? m + world : m);
}

// ------------------------------------------------------------------------------------------
// segment bounds of an ascending segment-id list, for the kernels that walk segments without an offsets pass (lsz_body,
// kv_op_kernels.h; shard_finish_sparse_body, kv_route.h): lo(s) = lower_bound(segment_ids, s), clamped like
// seg_offsets_body — lo(s <= 0) = 0, lo(s >= nseg) = lower_bound(nseg) — so every position is in [0, n] whatever the list
// holds.  At most log2(n) dependent loads per bound, L2-resident after the first waves.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int lsz_lower_bound(const void* __restrict__ seg, int seg32, int n, long long s) {
  int a = 0, b = n;
  while (a < b) {
    const int m = a + ((b - a) >> 1);
    const long long x = seg32 ? (long long)reinterpret_cast<const int*>(seg)[m] : reinterpret_cast<const long long*>(seg)[m];
    if (x < s) a = m + 1; else b = m;
  }
  return a;
}
__device__ __forceinline__ int lsz_bound(const void* __restrict__ seg, int seg32, int n, long long nseg, long long s) {
  return s <= 0 ? 0 : lsz_lower_bound(seg, seg32, n, s < nseg ? s : nseg);
}
