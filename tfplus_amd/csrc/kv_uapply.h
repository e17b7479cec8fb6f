// kv_uapply.h — the optimizer apply at the reference's REAL op boundary: unique ids + pre-summed gradient rows, one launch.
//
// In an unchanged TF1 graph the reference's processor patch (python/ops/variable_scope.py:1096-1106) routes a KvVariable's
// IndexedSlices gradient through TF-core's _deduplicate_indexed_slices, so KvVariableGroupSparseApplyAdamV4 and its
// siblings receive `indices` that are already unique and `grad` rows that are already summed (training_ops.cc:7011-7021).
// For that input the batch pipeline (tile dedup, tile sums, partition pass) does work whose answer is known: every id is
// its own key, every gradient row its own sum.  With the caller's PROMISE that the ids are unique (kv_apply_*_unique) the
// op is this one kernel:
//
//   one lane group (LPR lanes) per id, 64 / LPR ids per wave and step: the id -> its index entry (row + slot-row hint; a key
//   the table does not hold yet is inserted on the spot: FindOrInsertUnsafe, kv_variable.h:382-416) -> ONE round trip for
//   the gradient row, the var row and its record, the hinted slot row and its record -> frequency filter / un-blacklisting,
//   AddFrequency on the slot row, the fused row update (opt_core: training_ops.cc row math) -> stores.
//
// A broken promise is caught, not raced.  Every row record carries a 16-bit stamp (RowMeta::stamp): the serial of the last
// unique-apply launch that updated the row.  The key's group reads the stamp with the record and flips it to this
// launch's serial with ONE returning atomic XOR on the record's flag word (performed at the memory side, so it orders
// groups on different XCDs):
//   * the stamp read already equals the serial   -> a group of this launch updated the row before: duplicate, skipped;
//   * the XOR returns a stamp other than the one read -> another group flipped it in between: duplicate.
// Either way the table's error word is raised (code 4; the next call on the table returns KV_INVALID_ARGUMENT) and the
// caller learns that the batch was not applied as the reference would have (sequentially, under the table lock).  The
// host clears all stamps when the 16-bit serial wraps (every 65535 launches per table: one pass over the records).
#pragma once

// FindOrInsertUnsafe (kv_variable.h:382-416) for the unique apply: the caller's probe found no row for `key`.
// *state: 1 = inserted by this call (the row is returned), 2 = the key has an index entry after all — another group of this
// launch holds the same id (returns its row, or 0 while that group has not published it), 3 = the row slab is full.
// The new row's stamp is set by an atomic exchange that has been PERFORMED (at the memory side) before the row is
// published: a group that finds the row through the index reads this launch's serial there, or — from a stale cached
// line — a stamp that its own atomic XOR then shows to be stale.  Either way the duplicate is caught.
__device__ __forceinline__ unsigned uniq_insert(const TableDev& t, long long key, unsigned serial, unsigned* state) {
  Entry* slot;
  unsigned long long stored;
  unsigned long long p = 0;
  const bool sentinel = key == EMPTY_KEY;
  if (sentinel) { slot = &t.entries[t.mask + 1]; stored = 0ull; }
  else { stored = (unsigned long long)key; p = mix64((unsigned long long)key) & t.mask; slot = &t.entries[p]; }
  for (;;) {
    const Entry e = load_entry(slot);
    if ((unsigned long long)e.key == stored && !(sentinel && e.key == EMPTY_KEY)) {
      if (e.row == ROW_TOMB) {   // deleted earlier: the entry is still this key's — give it a row again
        if (atomicCAS(&slot->row, ROW_TOMB, 0u) == ROW_TOMB) break;
        *state = 2u; return 0u;
      }
      *state = 2u; return e.row;
    }
    if (e.key == EMPTY_KEY) {
      const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&slot->key),
                                               (unsigned long long)EMPTY_KEY, stored);
      if (old == (unsigned long long)EMPTY_KEY) break;   // claimed
      if (old == stored) { *state = 2u; return 0u; }
      if (sentinel) continue;
    } else if (sentinel) {
      *state = 2u; return 0u;   // unreachable: entries[cap] holds EMPTY or 0
    }
    if (!sentinel) { p = (p + 1) & t.mask; slot = &t.entries[p]; }
  }
  unsigned r = 0;
  bool have = false;
  if (t.free_rows) {   // rows released by Delete first
    const int f = atomicSub(reinterpret_cast<int*>(&t.counters[2]), 1);
    if (f > 0) { r = t.free_rows[f - 1]; have = true; }
    else atomicAdd(reinterpret_cast<int*>(&t.counters[2]), 1);
  }
  if (!have) {
    r = atomicAdd(&t.counters[0], 1u);
    if (r >= t.max_rows) { raise_error(t, 1u); *state = 3u; return 0u; }
  }
  (void)__hip_atomic_exchange(reinterpret_cast<unsigned*>(&meta_ptr(t, r)->flags), (serial & 0xFFFFu) << 16, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stamp is in place before anyone can find the row
  __hip_atomic_store(&slot->row, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *state = 1u;
  return r;
}

template <int OPT, int V, int LPR, int K>
__device__ __forceinline__ void uapply_body(const PartArgs& a, const void* __restrict__ ids, int ids32, long long n) {
  constexpr int G = 64 / LPR;
  if (*reinterpret_cast<volatile unsigned*>(&a.tv.counters[1])) return;   // an earlier batch left the error flag up
  const int D = a.tv.dim;
  const int wl = threadIdx.x & 63, lane = wl % LPR, g = wl / LPR;
  int eoff[K];
  bool evalid[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { const int e0 = (lane + k * LPR) * V; evalid[k] = e0 < D; eoff[k] = evalid[k] ? e0 : 0; }
  // the lean update for every key whose slot mirror stands; any other key or table goes through finish_key (kv_key_update.h)
  const LeanCtx lc = lean_ctx<OPT>(a);
  const unsigned serial = a.uniq_serial & 0xFFFFu;
  const float* const gbase = a.grad;
  const long long nbatch = (n + G - 1) / G;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  // Two batches ahead: the id of batch b + 2 strides and the index entry of batch b + 1 stride are requested while batch b
  // is worked on, so a batch pays one exposed round trip (its rows), not three (id -> entry -> rows).
  auto id_at = [&](long long bb) -> long long {
    long long j = bb * G + g;
    if (j >= n) j = n - 1;   // (past the end: a valid address, the value is not used)
    return ids32 ? (long long)static_cast<const int*>(ids)[j] : static_cast<const long long*>(ids)[j];
  };
  const long long b0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  long long key_n = id_at(b0);
  long long key_nn = id_at(b0 + nwaves);
  unsigned long long p_n = home_of(a.tv, key_n, mix64((unsigned long long)key_n));
  Entry e_n = load_entry(&a.tv.entries[p_n]);
  for (long long b = b0; b < nbatch; b += nwaves) {   // wave-uniform
    const long long i = b * G + g;
    const bool live0 = i < n;
    const long long ic = live0 ? i : n - 1;
    const long long key = key_n;
    const unsigned long long p = p_n;
    const Entry e0 = e_n;
    key_n = key_nn;
    p_n = home_of(a.tv, key_n, mix64((unsigned long long)key_n));
    e_n = load_entry(&a.tv.entries[p_n]);
    key_nn = id_at(b + 2 * nwaves);
    unsigned hint = 0;
    unsigned row = table_find_from(a.tv, key, p, e0, &hint);
    bool isnew = false, dup = false;
    if (__builtin_expect(__ballot(live0 && (row == 0u || hint == HINT_NEW)) != 0ull, 0)) {
      // a key the table does not hold yet is inserted by the group's leader (uniq_insert).  An entry marked HINT_NEW belongs
      // to an insert in flight: within one stream-ordered op that is another group of this launch — a duplicate.
      unsigned r2 = row, fl = 0;
      if (live0 && lane == 0) {
        if (row == 0u) r2 = uniq_insert(a.tv, key, serial, &fl);
        else fl = 2u;
      }
      if (LPR > 1) { r2 = __shfl(r2, 0, LPR); fl = __shfl(fl, 0, LPR); }
      if (live0 && (row == 0u || hint == HINT_NEW)) { row = fl == 1u ? r2 : 0u; isnew = fl == 1u; dup = fl == 2u; hint = 0; }
    }
    const bool live = live0 && !dup;
    const bool st_live = live && row != 0u;

    // ---- everything the key needs, in one round trip ---------------------------------------------------------------------
    float gv[K][V];
    {
      const float* src = gbase + (size_t)ic * D;
#pragma unroll
      for (int k = 0; k < K; ++k) ldv_stream<V>(src + eoff[k], gv[k]);
    }
    RowMeta m0{};
    uint2 vm = make_uint2(0u, 0u);
    uint4 mir = make_uint4(0u, 0u, 0u, 0u);
    bool hint_loaded = false, have_x = false, have_s = false;
    PreRows<OPT, V, K> pre;
    // (the same loads as papply_body's prefetch lambda, kv_papply.h: keep the two in step — kv_key_update.h says why they are two)
    if (lc.fast) {
      constexpr int NS0 = slot0_blocks(OPT);
      const unsigned rr = st_live ? row : 0u;
      const unsigned hh = (st_live && hint < lc.smax) ? hint : 0u;
      const RowMeta* const vrec = lc.vmeta + (size_t)rr * META_STRIDE;
      mir = *reinterpret_cast<const uint4*>(vrec + 1);   // the slot record's copy, in the var record's own line
      vm = *reinterpret_cast<const uint2*>(&vrec->freq);
      const float* xr = lc.vrows + (size_t)rr * D;
      const float* sr = lc.srows + (size_t)hh * lc.SD;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        ldv<V>(xr + eoff[k], pre.x[k]);
#pragma unroll
        for (int b3 = 0; b3 < NS0; ++b3) ldv<V>(sr + b3 * D + eoff[k], pre.s[b3][k]);
      }
      hint_loaded = false; have_x = true; have_s = hh != 0u;   // (the general path reads the slot record itself)
    } else {
      if (st_live && !isnew) vm = load_freq_flags(a.tv, row);
      const uint4 rq = make_uint4((unsigned)key, (unsigned)((unsigned long long)key >> 32), st_live ? row : 0u, st_live ? hint : 0u);
      prefetch_state<OPT, V, LPR, K>(a, rq, st_live, lane, D, m0, hint_loaded, pre, have_x, have_s);
      if (!have_x) {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int cc = 0; cc < V; ++cc) pre.x[k][cc] = 0.f;
      }
    }

    // ---- the promise: nobody else of this launch holds the row (see the head of this file) ----------------------------------
    const unsigned st0 = vm.y >> 16;
    bool mine = st_live && !isnew;
    if (mine && st0 == serial) { dup = true; mine = false; }   // a group of this launch has been here already
    unsigned old = 0;
    const bool asked = mine && lane == 0;
    if (asked)
      old = __hip_atomic_fetch_xor(reinterpret_cast<unsigned*>(&meta_ptr(a.tv, row)->flags), (st0 ^ serial) << 16, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    const bool go = live && !dup;   // (a duplicate caught by the stamp it read is skipped; one caught by the XOR has raced already)

    // ---- a key inserted now: the init rule's row, record with frequency word 1, never filtered (kv_variable.h:400-407) -------
    bool vnew = false;
    {
      const bool nk = go && st_live && isnew;
      if (__builtin_expect(__ballot(nk) != 0ull, 0)) {
        const bool any = init_var_row<V, LPR, K>(a.tv, key, row, nk, D, eoff, evalid, pre.x);
        if (nk) {
          const unsigned nfl = any ? 0u : (unsigned)FLAG_UNDER;
          if (lane == 0) {
            RowMeta nm; nm.key = key; nm.freq = 1u; nm.flags = (unsigned char)nfl; nm.delta = 0; nm.stamp = (unsigned short)serial;
            *meta_ptr(a.tv, row) = nm;
          }
          vm.x = 1u; vm.y = nfl | (serial << 16);
          have_x = true;
          vnew = true;
        }
      }
    }

    // ---- the update ----------------------------------------------------------------------------------------------------------
    const uint4 ra = make_uint4((unsigned)key, (unsigned)((unsigned long long)key >> 32), row | (vnew ? NEW_BIT : 0u), hint);
    const bool general = key_update<OPT, V, LPR, K>(a, lc, row, hint, vnew, go, lane, D, gv, vm, mir, pre);
    if (!lc.fast || __ballot(general) != 0ull)
      finish_key<MODE_APPLY, OPT, V, LPR, K>(a, ra, general, hint_loaded && general, m0, gv, lane, &pre, have_x && general,
                                             have_s && general);
    // ---- what the XOR found -----------------------------------------------------------------------------------------------------
    if (asked && (old >> 16) != st0) dup = true;
    if (__builtin_expect(__ballot(dup && lane == 0) != 0ull, 0)) {
      if (dup && lane == 0) raise_error(a.tv, 4u);
    }
  }
}

template <int OPT, int V, int LPR, int K>
__global__ void __launch_bounds__(256, (K == 1 ? 4 : 2)) k_uapply(PartArgs a, const void* __restrict__ ids, int ids32, long long n) {
  uapply_body<OPT, V, LPR, K>(a, ids, ids32, n);
}

// many tables in one launch (blockIdx.y = table; arguments from the MultiDesc array)
template <int OPT, int V, int LPR, int K>
__global__ void __launch_bounds__(256, (K == 1 ? 4 : 2)) k_uapply_multi(const MultiDesc* __restrict__ descs, int ids32) {
  const MultiDesc& m = descs[blockIdx.y];
  if (m.n == 0) return;
  uapply_body<OPT, V, LPR, K>(m.a, m.ids, ids32, m.n);
}

// the id count from the device (kv_apply_unique_counted): *n_dev is the number of ids and gradient rows that are valid, at
// most the n_max the host sized the launch for.  One load of a uniform address (a scalar load: every wave gets the word
// once), then the check: a count outside 0 .. n_max raises the table's error word (code 5) and nothing is applied; with 0 ids
// nothing is read at all (uapply_body's id_at clamps to n - 1).
template <int OPT, int V, int LPR, int K>
__global__ void __launch_bounds__(256, (K == 1 ? 4 : 2)) k_uapply_counted(PartArgs a, const void* __restrict__ ids, int ids32,
                                                                           long long n_max, const long long* __restrict__ n_dev) {
  const long long n = *n_dev;
  if (n < 0 || n > n_max) {
    if (blockIdx.x == 0 && threadIdx.x == 0) raise_error(a.tv, 5u);
    return;
  }
  if (n == 0) return;
  uapply_body<OPT, V, LPR, K>(a, ids, ids32, n);
}

// dispatch on the row geometry (as k_papply: kv_row_geom.h, the float4 rungs up to ENTRY_MAX_Q).  KV_UNIMPLEMENTED for other
// dims: the caller falls back to the batch pipeline, which serves them.  md != nullptr: `ntab` tables in one launch (n = the
// largest table's ids, pa = any table's arguments: only the dim is read).  n_dev != nullptr (single table only): n is the
// most ids the call may hold — the grid is sized from it — and the kernel takes the count from *n_dev (k_uapply_counted)
template <int OPT>
int launch_uapply_t(const PartArgs& pa, const void* ids, int ids32, long long n, hipStream_t s, const MultiDesc* md = nullptr,
                    int ntab = 0, const long long* n_dev = nullptr) {
  return with_row_geom<ENTRY_MAX_Q>(pa.tv.dim, [&](auto g) -> int {
    constexpr int V = decltype(g)::V, LPR = decltype(g)::LPR, K = decltype(g)::K;
    constexpr int G = 64 / LPR;
    const int resident = resident_blocks<k_uapply<OPT, V, LPR, K>>(256, 6, 2);   // per device
    const long long nbatch = (n + G - 1) / G;
    const long long want = (nbatch + 3) / 4;
    int grid = (int)(want < 1 ? 1 : want > resident ? resident : want);
    if (md) {   // all tables' blocks are one resident generation
      if (ntab > 0 && (long long)grid * ntab > resident) grid = resident / ntab > 1 ? resident / ntab : 1;
      k_uapply_multi<OPT, V, LPR, K><<<dim3((unsigned)grid, (unsigned)ntab), 256, 0, s>>>(md, ids32);
    } else if (n_dev) {
      k_uapply_counted<OPT, V, LPR, K><<<grid, 256, 0, s>>>(pa, ids, ids32, n, n_dev);
    } else {
      k_uapply<OPT, V, LPR, K><<<grid, 256, 0, s>>>(pa, ids, ids32, n);
    }
    return KV_OK;
  });
}
