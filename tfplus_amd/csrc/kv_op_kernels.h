// kv_op_kernels.h — the small kernels only the table ops (kv_ops.hip) launch: point queries, delete, export / import /
// delta, the inference gathers, unique / dedup helpers, the sparse lookup's combiners, its backward and their batched forms, the
// serving-mode sparse lookup (kv_lookup_sparse_zeros),
// kv_take_rows.  Included by kv_ops.hip
// alone, behind kv_device.h, inside its anonymous namespace.
#pragma once

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

// KvVariableGatherOrZeros: read-only, no dedup needed (no writes, repeated keys hit cache).
// FindOrZeros kv_variable.h:239-254 / BatchGetWithFn table_manager.h:112-154.
template <typename IdT>
__global__ void __launch_bounds__(TB) k_gather_or_zeros(TableDev t, const IdT* __restrict__ ids,
                                                        float* __restrict__ out, long long n) {
  const int D = t.dim;
  const int lane8 = threadIdx.x & 7;
  for (long long i = (long long)blockIdx.x * (TB / 8) + (threadIdx.x >> 3); i < n;
       i += (long long)gridDim.x * (TB / 8)) {
    const unsigned r = table_find(t, load_id(ids, (size_t)i));
    const float* row = row_ptr(t, r);  // blacklisted rows are stored as zeros; row 0 is zeros
    float* o = out + (size_t)i * D;
    if ((D & 3) == 0) {
      for (int q = lane8; q < (D >> 2); q += 8)
        reinterpret_cast<float4*>(o)[q] = reinterpret_cast<const float4*>(row)[q];
    } else {
      for (int e = lane8; e < D; e += 8) o[e] = row[e];
    }
  }
}

// The same op for dims 4·VQ (VQ a power of two <= 64), wave-shaped like k_gather: one wave takes 64
// consecutive ids per step, lane l probes id l (64 independent probes in flight per wave, none of them
// repeated by neighbouring lanes), then the wave copies the rows VQ lanes per row, CH copy instructions
// in flight, row ids handed over by shuffle, streaming stores (the output is not read again here).
// ids_kind: 0 int64, 1 int32, 2 (id, count) int64 pairs.  `wave` of `nwaves` waves share the rows.
// Software pipeline over the wave's steps: while step i copies its rows, the home index entries of step
// i + 1 and the ids of step i + 2 are already in flight, so a step costs one round trip, not three — the
// gather keeps the store bandwidth busy from a few waves per CU (it runs beside the partition pass).
template <int VQ, int CWMAX = 4>
__device__ __forceinline__ void goz_wave(const TableDev& t, const void* __restrict__ ids, int ids_kind,
                                         float* __restrict__ out, long long n, long long wave, long long nwaves) {
  constexpr int RW = 64 / VQ;            // rows per copy instruction
  constexpr int CW = VQ < CWMAX ? VQ : CWMAX;    // copy instructions in flight (4 with many waves per CU: the probe hop
                                                 // wants the occupancy; 8 for the few gather waves beside the partition pass)
  const int lane = threadIdx.x & 63;
  const int v = lane % VQ, sub = lane / VQ;
  const long long stride = nwaves * 64;
  auto load_key = [&](long long i) -> long long {
    if (i >= n) return EMPTY_KEY;
    return ids_kind == 1 ? (long long)reinterpret_cast<const int*>(ids)[i]
                         : reinterpret_cast<const long long*>(ids)[i << (ids_kind == 2 ? 1 : 0)];
  };
  long long r0 = wave * 64;
  if (r0 >= n) return;
  long long k1 = load_key(r0 + lane);                  // step i + 1's key (first: step 0's)
  long long k2 = load_key(r0 + stride + lane);         // step i + 2's
  unsigned long long p1 = home_of(t, k1, mix64((unsigned long long)k1));
  Entry e1 = load_entry(&t.entries[p1]);
  for (; r0 < n; r0 += stride) {
    // this step's rows: finish the probe started one step ago (row 0 reads zeros: misses, lanes past the end)
    const unsigned rr = (r0 + lane < n) ? table_find_from(t, k1, p1, e1) : 0u;
    // next step: its home entries leave now, the ids of the step after it too
    k1 = k2;
    p1 = home_of(t, k1, mix64((unsigned long long)k1));
    if (r0 + stride < n) e1 = load_entry(&t.entries[p1]);
    k2 = load_key(r0 + 2 * stride + lane);
#pragma unroll
    for (int j0 = 0; j0 < VQ; j0 += CW) {
      float4 val[CW];
      unsigned rj[CW];
#pragma unroll
      for (int j = 0; j < CW; ++j) rj[j] = __shfl(rr, (j0 + j) * RW + sub);
#pragma unroll
      for (int j = 0; j < CW; ++j) val[j] = reinterpret_cast<const float4*>(row_ptr(t, rj[j]))[v];
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        const long long ii = r0 + (j0 + j) * RW + sub;
        if (ii < n) {
          float4* dst = reinterpret_cast<float4*>(out + (size_t)ii * (VQ * 4)) + v;
          __builtin_nontemporal_store(val[j].x, &dst->x); __builtin_nontemporal_store(val[j].y, &dst->y);
          __builtin_nontemporal_store(val[j].z, &dst->z); __builtin_nontemporal_store(val[j].w, &dst->w);
        }
      }
    }
  }
}
template <typename IdT, int VQ>
__global__ void __launch_bounds__(TB) k_gather_or_zeros_w(TableDev t, const IdT* __restrict__ ids,
                                                          float* __restrict__ out, long long n) {
  goz_wave<VQ>(t, ids, sizeof(IdT) == 4 ? 1 : 0, out, n, (long long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6),
               (long long)gridDim.x * (TB / 64));
}

// the gather for any dim behind one entry: wave-shaped for dims 4, 8, ..., 256, else 8 lanes per row
template <int CWMAX = 4>
__device__ __forceinline__ void goz_any(const TableDev& t, const void* __restrict__ ids, int ids_kind,
                                        float* __restrict__ out, long long n, long long blk, long long nblk) {
  const int D = t.dim;
  const long long wave = blk * (blockDim.x / 64) + (threadIdx.x >> 6);
  const long long nwaves = nblk * (blockDim.x / 64);
  if ((D & 3) == 0) {  // block-uniform
    switch (D >> 2) {
      case 1: goz_wave<1, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 2: goz_wave<2, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 4: goz_wave<4, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 8: goz_wave<8, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 16: goz_wave<16, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 32: goz_wave<32, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      case 64: goz_wave<64, CWMAX>(t, ids, ids_kind, out, n, wave, nwaves); return;
      default: break;
    }
  }
  const int lane8 = threadIdx.x & 7;
  const long long gpb = blockDim.x / 8;
  for (long long i = blk * gpb + (threadIdx.x >> 3); i < n; i += nblk * gpb) {
    const long long key = ids_kind == 1 ? (long long)reinterpret_cast<const int*>(ids)[i]
                                        : reinterpret_cast<const long long*>(ids)[i << (ids_kind == 2 ? 1 : 0)];
    const unsigned r = table_find(t, key);
    const float* row = row_ptr(t, r);
    float* o = out + (size_t)i * D;
    if ((D & 3) == 0) {
      for (int q = lane8; q < (D >> 2); q += 8)
        reinterpret_cast<float4*>(o)[q] = reinterpret_cast<const float4*>(row)[q];
    } else {
      for (int e = lane8; e < D; e += 8) o[e] = row[e];
    }
  }
}

// BatchKvVariableGatherOrZerosV2 (kernels/kv_variable_ops.cc:431-470): N tables, N id lists, N
// outputs — the reference loops over the tables; here ONE launch covers them all (blockIdx.y =
// table, tables may differ in dim), which is what a 26-feature serving step needs.
struct BatchGatherDesc {
  TableDev t;
  const void* ids;
  float* out;
  long long n;
  int ids_int32;
};
__global__ void __launch_bounds__(TB) k_batch_gather_or_zeros(const BatchGatherDesc* __restrict__ descs) {
  const BatchGatherDesc& d = descs[blockIdx.y];
  goz_any(d.t, d.ids, d.ids_int32 ? 1 : 0, d.out, d.n, blockIdx.x, gridDim.x);
}

__global__ void k_store_count(const unsigned* ctr, long long* out) { *out = (long long)*ctr; }

// kv_dedup_segment_sum: inverse[i] = dense unique index of input position i
__global__ void k_dedup_inverse(WsDev w, long long n, int* inverse) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    inverse[i] = (int)w.ent_b[w.slot_rank[i] & SLOT_MASK];
}

// ---------------------------------------------------------------------------------------------
// embedding_lookup_sparse (python/ops/embedding_ops.py:279-441) fused behind the lookup index:
//   k_seg_offsets   CSR offsets of the sorted segment ids: off[s] = first position of segment s
//   k_seg_combine   out[s] = combine_j( w_j * rows[row(id_j)] ) over the segment's positions, in
//                   position order (tf.segment_sum order); mean: / sum w, sqrtn: / sqrt(sum w^2)
// Segment ids outside [prev, num_segments) are clamped (memory safety only; TF rejects them).
template <typename SegT>
__device__ __forceinline__ void seg_offsets_body(const SegT* __restrict__ seg, long long n, long long nseg,
                                                 unsigned* __restrict__ off) {
  for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i <= n; i += (long long)gridDim.x * TB) {
    long long prev = i > 0 ? (long long)seg[i - 1] : -1;
    long long cur = i < n ? (long long)seg[i] : nseg;
    prev = prev < -1 ? -1 : (prev > nseg ? nseg : prev);
    cur = cur < 0 ? 0 : (cur > nseg ? nseg : cur);
    for (long long sgi = prev + 1; sgi <= cur; ++sgi) off[sgi] = (unsigned)i;
  }
}
template <typename SegT>
__global__ void __launch_bounds__(TB) k_seg_offsets(const SegT* __restrict__ seg, long long n, long long nseg,
                                                    unsigned* __restrict__ off) {
  seg_offsets_body(seg, n, nseg, off);
}

// VQ = float4 lanes per row (dim / 4, power of two <= 64) or 0 = one thread per element.
// has_w: sp_weights given (the reference multiplies, sums and divides by the weight sums);
// otherwise tf.sparse_segment_{sum,mean,sqrt_n} (empty segment -> zeros).
template <int VQ>
__global__ void __launch_bounds__(TB) k_seg_combine(TableDev t, WsDev w, const unsigned* __restrict__ off,
                                                    const float* __restrict__ wts, long long nseg,
                                                    int combiner, float* __restrict__ out) {
  const int D = t.dim;
  constexpr int LPS = VQ > 0 ? VQ : 1;          // lanes per segment
  const int v = threadIdx.x % LPS;
  const long long g0 = ((long long)blockIdx.x * TB + threadIdx.x) / LPS;
  const long long gstride = (long long)gridDim.x * TB / LPS;
  for (long long sgi = g0; sgi < nseg; sgi += gstride) {
    const unsigned lo = off[sgi], hi = off[sgi + 1];
    float wsum = 0.f, w2 = 0.f;
    if constexpr (VQ > 0) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      // SU ids of the segment at a time: their three dependent hops (slot -> row id -> row) overlap;
      // the sums are still taken in id order
      constexpr int SU = 4;
      for (unsigned j = lo; j < hi; j += SU) {
        unsigned sl[SU], r[SU];
        float wj[SU];
        float4 x[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const bool ok = j + u < hi;
          sl[u] = ok ? (w.slot_rank[j + u] & SLOT_MASK) : 0xFFFFFFFFu;
          wj[u] = ok ? (wts ? wts[j + u] : 1.f) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) r[u] = sl[u] != 0xFFFFFFFFu ? w.ent_b[sl[u]] : 0u;
#pragma unroll
        for (int u = 0; u < SU; ++u) x[u] = reinterpret_cast<const float4*>(row_ptr(t, r[u]))[v];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          if (sl[u] == 0xFFFFFFFFu) continue;
          acc.x += x[u].x * wj[u]; acc.y += x[u].y * wj[u]; acc.z += x[u].z * wj[u]; acc.w += x[u].w * wj[u];
          wsum += wj[u]; w2 += wj[u] * wj[u];
        }
      }
      float den = 1.f;
      if (combiner == 1) den = wsum; else if (combiner == 2) den = sqrtf(w2);
      if (combiner != 0 && (wts || hi > lo)) { acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den; }
      reinterpret_cast<float4*>(out + (size_t)sgi * D)[v] = acc;
    } else {
      for (int e = 0; e < D; ++e) {
        float acc = 0.f;
        wsum = 0.f; w2 = 0.f;
        for (unsigned j = lo; j < hi; ++j) {
          const unsigned r = w.ent_b[w.slot_rank[j] & SLOT_MASK];
          const float wj = wts ? wts[j] : 1.f;
          acc += row_ptr(t, r)[e] * wj;
          wsum += wj; w2 += wj * wj;
        }
        float den = 1.f;
        if (combiner == 1) den = wsum; else if (combiner == 2) den = sqrtf(w2);
        if (combiner != 0 && (wts || hi > lo)) acc /= den;
        out[(size_t)sgi * D + e] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// kv_lookup_sparse_zeros: embedding_lookup_sparse outside training (python/ops/kv_variable_ops.py:1072-1080, 1105-1113:
// unique -> KvVariableGatherOrZerosV2; embedding_ops.py:359-441: gather(idx) -> (x weights) -> segment_sum /
// sparse_segment_{sum,mean,sqrt_n}) in ONE launch, read-only: no dedup, no offsets pass, no workspace.
//   out[s] = combine_j( w_j * row(id_j) ) over the segment's positions in position order, row() = what
//   k_gather_or_zeros reads (row 0, the zero row, for a key the index does not hold)
// A group of LPS lanes owns a segment (VQ lanes, one float4 each, for dims 4 * VQ; VQ == 0: the whole wave, lane v owns
// elements v, v + 64, ... of any dim up to 1024).  Two things differ from k_seg_combine:
//  * segment bounds: lo(s) = lower_bound(segment_ids, s), searched by the group's lane 0; hi(s) = lo(s + 1) comes from
//    the next group of the wave by shuffle, and the wave's last bound is searched by the last group's lane 1 in the same
//    loop (VQ == 1 has no such lane: there lane 63 searches twice).  Clamped like seg_offsets_body: lo(s <= 0) = 0,
//    lo(s >= nseg) = lower_bound(nseg), so every position is in [0, n] whatever the list holds.
//    Cost, DERIVED and not measured: at most log2(n) dependent loads per bound, L2-resident after the first waves
//    (~200 cycles an L2 hit), i.e. 11-18 hops = 1-1.5 us at serving sizes (2 k - 200 k ids), all groups' searches in
//    flight together — below the ~6 us of the launch boundary a separate offsets kernel would add, and without the
//    workspace bookkeeping that would bar graph capture.
//  * row lookup: there is no entry list.  Lane u of the group probes position pos + u (LPS probes of a group in flight,
//    none repeated by a neighbour), the row numbers and weights go round by shuffle, SU rows in flight per lane; the
//    additions stay in position order.  Rows are plain loads (repeated keys hit L2), out is written once, streaming.
//    The probe is NOT software-pipelined across chunks as goz_wave's is: a chunk of LPS positions pays id -> entry -> row
//    before the next chunk's probe starts, so with small groups (dim 4 / 8: LPS 1 / 2) a long segment advances one or two
//    positions per three hops.  At serving shapes (1-8 ids per segment, dims 64 / 128) a segment is one chunk; measured
//    there (profiles/serving_sparse.txt) the batched launch takes 2.3-3.3x the plain batched gather of the same ids: the
//    bound search and the probe are one dependent chain per wave step.  Pipelining both across a wave's steps, as
//    goz_wave does, is the next step for this kernel.
// No LDS, no atomics, no float reduction across lanes.  (lsz_bound: kv_device.h — the sharded combining finish walks
// its segments the same way.)
template <int VQ>
__device__ __forceinline__ void lsz_body(const TableDev& t, const void* __restrict__ ids, int ids32,
                                         const void* __restrict__ seg, int seg32, const float* __restrict__ wts,
                                         int n, long long nseg, int combiner, float* __restrict__ out,
                                         long long blk, long long nblk) {
  constexpr int LPS = VQ > 0 ? VQ : 64;     // lanes per segment
  constexpr int G = 64 / LPS;               // segments per wave and step
  constexpr int SU = LPS < 4 ? LPS : 4;     // rows in flight per lane
  constexpr int NE = 16;                    // VQ == 0: elements per lane at the most (dim <= 1024)
  const int D = t.dim;
  const int lane = threadIdx.x & 63;
  const int v = lane % LPS, sub = lane / LPS, gbase = sub * LPS;
  const int kmax = VQ > 0 ? 0 : (D + 63) >> 6;
  const long long wave = blk * (blockDim.x / 64) + (threadIdx.x >> 6);
  const long long nwaves = nblk * (blockDim.x / 64);
  for (long long base = wave * G; base < nseg; base += nwaves * G) {   // wave-uniform
    const long long sgi = base + sub;
    // the bounds: lane 0 of each group its segment's first position, the wave's last bound beside them
    int b0 = 0, b1 = 0;
    if (v == 0) b0 = lsz_bound(seg, seg32, n, nseg, sgi);
    else if (LPS > 1 && lane == 64 - LPS + 1) b0 = lsz_bound(seg, seg32, n, nseg, base + G);
    if (LPS == 1 && lane == 63) b1 = lsz_bound(seg, seg32, n, nseg, base + G);
    const int lo = __shfl(b0, gbase);
    const int hi_next = __shfl(b0, sub < G - 1 ? gbase + LPS : gbase);
    const int hi_last = LPS > 1 ? __shfl(b0, 64 - LPS + 1) : __shfl(b1, 63);
    const int hi = sub < G - 1 ? hi_next : hi_last;
    const int len = sgi < nseg && hi > lo ? hi - lo : 0;   // (a list that is not ascending may give hi < lo: nothing is read)
    float wsum = 0.f, w2 = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float accs[VQ > 0 ? 1 : NE];
    if constexpr (VQ == 0) {
#pragma unroll
      for (int k = 0; k < NE; ++k) accs[k] = 0.f;
    }
    unsigned pos = (unsigned)lo;   // the chunk's first position; rem: the segment's positions from there on
    for (int rem = len; __any(rem > 0); rem -= LPS, pos += LPS) {
      // lane v: the probe of position pos + v (row 0, weight 0 past the segment's end)
      const bool live = v < rem;
      unsigned r = 0u;
      float wv = 0.f;
      if (live) {
        const unsigned p = pos + v;
        const long long key = ids32 ? (long long)reinterpret_cast<const int*>(ids)[p] : reinterpret_cast<const long long*>(ids)[p];
        wv = wts ? wts[p] : 1.f;
        r = table_find(t, key);
      }
      for (int u0 = 0; u0 < LPS && __any(u0 < rem); u0 += SU) {
        unsigned ru[SU];
        float wu[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) { ru[u] = __shfl(r, gbase + u0 + u); wu[u] = __shfl(wv, gbase + u0 + u); }
        if constexpr (VQ > 0) {
          float4 x[SU];
#pragma unroll
          for (int u = 0; u < SU; ++u) x[u] = reinterpret_cast<const float4*>(row_ptr(t, ru[u]))[v];
#pragma unroll
          for (int u = 0; u < SU; ++u) {
            if (u0 + u >= rem) continue;
            acc.x += x[u].x * wu[u]; acc.y += x[u].y * wu[u]; acc.z += x[u].z * wu[u]; acc.w += x[u].w * wu[u];
            wsum += wu[u]; w2 += wu[u] * wu[u];
          }
        } else {
          const float* rowp[SU];
#pragma unroll
          for (int u = 0; u < SU; ++u) rowp[u] = row_ptr(t, ru[u]);
#pragma unroll
          for (int k = 0; k < NE; ++k) {
            if (k < kmax) {   // wave-uniform
              const int e = v + (k << 6);
              float x[SU];
#pragma unroll
              for (int u = 0; u < SU; ++u) x[u] = e < D ? rowp[u][e] : 0.f;
#pragma unroll
              for (int u = 0; u < SU; ++u)
                if (u0 + u < rem) accs[k] += x[u] * wu[u];
            }
          }
#pragma unroll
          for (int u = 0; u < SU; ++u)
            if (u0 + u < rem) { wsum += wu[u]; w2 += wu[u] * wu[u]; }
        }
      }
    }
    if (sgi >= nseg) continue;
    float den = 1.f;
    if (combiner == 1) den = wsum; else if (combiner == 2) den = sqrtf(w2);
    const bool divide = combiner != 0 && (wts || len > 0);
    if constexpr (VQ > 0) {
      if (divide) { acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den; }
      float4* dst = reinterpret_cast<float4*>(out + (size_t)sgi * D) + v;
      __builtin_nontemporal_store(acc.x, &dst->x); __builtin_nontemporal_store(acc.y, &dst->y);
      __builtin_nontemporal_store(acc.z, &dst->z); __builtin_nontemporal_store(acc.w, &dst->w);
    } else {
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const int e = v + (k << 6);
        if (e < D) __builtin_nontemporal_store(divide ? accs[k] / den : accs[k], out + (size_t)sgi * D + e);
      }
    }
  }
}
// the lookup for any dim behind one entry, as goz_any: VQ lanes per segment for dims 4, 8, ..., 256, else the whole wave
__device__ __forceinline__ void lsz_any(const TableDev& t, const void* __restrict__ ids, int ids32,
                                        const void* __restrict__ seg, int seg32, const float* __restrict__ wts, int n,
                                        long long nseg, int combiner, float* __restrict__ out, long long blk, long long nblk) {
  const int D = t.dim;
  if ((D & 3) == 0) {  // block-uniform
    switch (D >> 2) {
      case 1: lsz_body<1>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 2: lsz_body<2>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 4: lsz_body<4>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 8: lsz_body<8>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 16: lsz_body<16>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 32: lsz_body<32>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      case 64: lsz_body<64>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk); return;
      default: break;
    }
  }
  lsz_body<0>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blk, nblk);
}
template <int VQ>
__global__ void __launch_bounds__(TB) k_lookup_sparse_zeros(TableDev t, const void* __restrict__ ids, int ids32,
                                                            const void* __restrict__ seg, int seg32,
                                                            const float* __restrict__ wts, int n, long long nseg,
                                                            int combiner, float* __restrict__ out) {
  lsz_body<VQ>(t, ids, ids32, seg, seg32, wts, n, nseg, combiner, out, blockIdx.x, gridDim.x);
}
// the batched form: blockIdx.y = table, tables free to differ in dim and key dtype; a table's blocks past its own
// segments leave at once
struct BatchSparseZerosDesc {
  TableDev t;
  const void* ids;
  const void* seg;
  const float* wts;
  float* out;
  long long nseg;
  int n;
  int ids_int32;
};
__global__ void __launch_bounds__(TB) k_batch_lookup_sparse_zeros(const BatchSparseZerosDesc* __restrict__ descs,
                                                                  int seg32, int combiner) {
  const BatchSparseZerosDesc& d = descs[blockIdx.y];
  lsz_any(d.t, d.ids, d.ids_int32, d.seg, seg32, d.wts, d.n, d.nseg, combiner, d.out, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// k_take_rows: out[i] = src[idx[i]] (SCATTER = 0) or out[idx[i]] = src[i] (SCATTER = 1) over rows of
// `nu` units of type U (float4 when the row is a multiple of 16 bytes).  The exchange's permute /
// un-permute / expand steps of the sharded path.
template <typename U, int SCATTER>
__global__ void __launch_bounds__(TB) k_take_rows(const U* __restrict__ src, const int* __restrict__ idx,
                                                  long long n, unsigned nu, int sh, U* __restrict__ out,
                                                  const int* __restrict__ idx_outer = nullptr) {
  const long long total = n * nu;
  const long long stride = (long long)gridDim.x * TB;
  for (long long x = (long long)blockIdx.x * TB + threadIdx.x; x < total; x += stride) {
    long long i;
    unsigned e;
    if (sh >= 0) { i = x >> sh; e = (unsigned)(x & (nu - 1)); }
    else { i = x / nu; e = (unsigned)(x - i * nu); }
    const long long j = idx_outer ? idx[idx_outer[i]] : idx[i];   // two-level gather: src[idx[idx_outer[i]]]
    if (SCATTER) out[j * nu + e] = src[x];
    else out[x] = src[j * nu + e];
  }
}

// ------------------------------------------------------------------------------------------
// k_seg_combine_e: embedding_lookup_sparse's combiner over the tiles' entries
// ------------------------------------------------------------------------------------------
// out[s] = combine_j( w_j * rows[row(id_j)] ) over segment s's positions in position order (tf.segment_sum's order;
// embedding_ops.py:395-441); position j -> its entry in its tile (pos_ent, filed by k_ltile) -> the entry's row word.  A
// key this batch inserted in ANOTHER tile may not know its row yet (NEW_BIT, row part 0): it is probed — the partition
// pass in front of this kernel has published every new row.  VQ lanes (power of two >= dim / 4) per segment, SU
// positions of a segment in flight; the sums are taken in position order whatever SU is.
template <int VQ>
__device__ __forceinline__ void seg_combine_e_body(const TableDev& t, const unsigned short* __restrict__ pos_ent,
                                                   const unsigned* __restrict__ ent_b, const long long* __restrict__ ent_key,
                                                   const unsigned* __restrict__ off, const float* __restrict__ wts,
                                                   long long nseg, int combiner, float* __restrict__ out) {
  const int D4 = t.dim >> 2;
  const int v = threadIdx.x % VQ;
  const bool vlive = v < D4;
  const int vv = vlive ? v : 0;
  const long long g0 = ((long long)blockIdx.x * TB + threadIdx.x) / VQ;
  const long long gstride = (long long)gridDim.x * TB / VQ;
  constexpr int SU = 4;
  for (long long sgi = g0; sgi < nseg; sgi += gstride) {
    const unsigned lo = off[sgi], hi = off[sgi + 1];
    float wsum = 0.f, w2 = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned j = lo; j < hi; j += SU) {
      unsigned e[SU], r[SU];
      float wj[SU];
      float4 x[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const bool ok = j + u < hi;
        const unsigned pe = ok ? (unsigned)pos_ent[j + u] : 0xFFFFu;
        e[u] = pe != 0xFFFFu ? ((j + u) / (unsigned)TILE) * (unsigned)TILE + pe : 0xFFFFFFFFu;
        wj[u] = ok ? (wts ? wts[j + u] : 1.f) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) r[u] = e[u] != 0xFFFFFFFFu ? ent_b[e[u]] : 0u;
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        if (__builtin_expect((r[u] & NEW_BIT) != 0u && (r[u] & ROW_MASK) == 0u, 0)) r[u] = table_find(t, ent_key[e[u]]);
        r[u] &= ROW_MASK;
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) x[u] = reinterpret_cast<const float4*>(row_ptr(t, r[u]))[vv];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        if (!(j + u < hi)) continue;
        acc.x += x[u].x * wj[u]; acc.y += x[u].y * wj[u]; acc.z += x[u].z * wj[u]; acc.w += x[u].w * wj[u];
        wsum += wj[u]; w2 += wj[u] * wj[u];
      }
    }
    float den = 1.f;
    if (combiner == 1) den = wsum; else if (combiner == 2) den = sqrtf(w2);
    if (combiner != 0 && (wts || hi > lo)) { acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den; }
    if (vlive) reinterpret_cast<float4*>(out + (size_t)sgi * t.dim)[v] = acc;
  }
}
template <int VQ>
__global__ void __launch_bounds__(TB) k_seg_combine_e(TableDev t, const unsigned short* __restrict__ pos_ent,
                                                      const unsigned* __restrict__ ent_b, const long long* __restrict__ ent_key,
                                                      const unsigned* __restrict__ off, const float* __restrict__ wts,
                                                      long long nseg, int combiner, float* __restrict__ out) {
  seg_combine_e_body<VQ>(t, pos_ent, ent_b, ent_key, off, wts, nseg, combiner, out);
}

// inverse[i] = the dense number of position i's id: position -> its entry in its tile -> the number k_papply PA_UNIQUE gave it
__global__ void __launch_bounds__(TB) k_inverse_e(const unsigned short* __restrict__ pos_ent, const unsigned* __restrict__ ent_b,
                                                  long long n, int* __restrict__ inverse) {
  for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < n; i += (long long)gridDim.x * TB)
    inverse[i] = (int)ent_b[(size_t)(i / TILE) * TILE + pos_ent[i]];
}

// ---------------------------------------------------------------------------------------------
// The backward of the sparse lookup: values[j] = scale_j * seg_grad[segment of j], scale_j = w_j (sum), w_j / sum_s(w)
// (mean), w_j / sqrtf(sum_s(w^2)) (sqrtn); w_j = 1 without weights.  Defined bit for bit: a segment's denominator is summed
// in float32 from +0 in position order (seg_combine_e_body's order and roundings), the scale is one IEEE division, each
// element one multiply.
//   k_seg_offsets   the CSR offsets, as in the forward
//   k_seg_den       weighted mean / sqrtn: den[s], one thread per segment (unweighted: the segment's length, straight
//                   from the offsets — no pass)
//   k_seg_expand    one lane group (VQ float4 lanes; VQ = 0: one thread per element) per position: reads seg_grad,
//                   writes each values row exactly once.  Rows of empty segments are never read: no position names them.
// A segment id outside [0, nseg) is clamped into it (memory safety only, like k_seg_offsets).
__device__ __forceinline__ void seg_den_body(const unsigned* __restrict__ off, const float* __restrict__ wts, long long nseg,
                                             int combiner, float* __restrict__ den) {
  for (long long sgi = (long long)blockIdx.x * TB + threadIdx.x; sgi < nseg; sgi += (long long)gridDim.x * TB) {
    const unsigned lo = off[sgi], hi = off[sgi + 1];
    float a = 0.f;
    if (combiner == 1) for (unsigned j = lo; j < hi; ++j) a += wts[j];
    else for (unsigned j = lo; j < hi; ++j) { const float wj = wts[j]; a += wj * wj; }
    den[sgi] = combiner == 1 ? a : sqrtf(a);
  }
}
__global__ void __launch_bounds__(TB) k_seg_den(const unsigned* __restrict__ off, const float* __restrict__ wts, long long nseg,
                                                int combiner, float* __restrict__ den) {
  seg_den_body(off, wts, nseg, combiner, den);
}

// the scale of position j in segment sg
__device__ __forceinline__ float seg_scale(const unsigned* __restrict__ off, const float* __restrict__ den,
                                           const float* __restrict__ wts, long long j, long long sg, int combiner) {
  const float wj = wts ? wts[j] : 1.f;
  if (combiner == 0) return wj;
  float d;
  if (wts) d = den[sg];
  else { d = (float)(off[sg + 1] - off[sg]); if (combiner == 2) d = sqrtf(d); }
  return wj / d;
}
template <typename SegT>
__device__ __forceinline__ long long seg_of(const SegT* __restrict__ seg, long long j, long long nseg) {
  const long long sg = (long long)seg[j];
  return sg < 0 ? 0 : (sg >= nseg ? nseg - 1 : sg);
}
template <typename SegT, int VQ>
__device__ __forceinline__ void seg_expand_body(const float* __restrict__ seg_grad, const SegT* __restrict__ seg,
                                                const unsigned* __restrict__ off, const float* __restrict__ den,
                                                const float* __restrict__ wts, long long n, long long nseg, int D, int combiner,
                                                float* __restrict__ values) {
  if constexpr (VQ > 0) {
    const int D4 = D >> 2;
    const int v = threadIdx.x % VQ;
    const long long g0 = ((long long)blockIdx.x * TB + threadIdx.x) / VQ;
    const long long gstride = (long long)gridDim.x * TB / VQ;
    for (long long j = g0; j < n; j += gstride) {
      const long long sg = seg_of(seg, j, nseg);
      const float sc = seg_scale(off, den, wts, j, sg, combiner);
      const float4* src = reinterpret_cast<const float4*>(seg_grad + (size_t)sg * D);
      float4* dst = reinterpret_cast<float4*>(values + (size_t)j * D);
      for (int q = v; q < D4; q += VQ) {   // (one round for dims up to 256; the lanes past the row's end take none)
        const float4 g = src[q];
        dst[q] = make_float4(g.x * sc, g.y * sc, g.z * sc, g.w * sc);
      }
    }
  } else {
    const long long total = n * D;
    for (long long x = (long long)blockIdx.x * TB + threadIdx.x; x < total; x += (long long)gridDim.x * TB) {
      const long long j = x / D;
      const int e = (int)(x - j * D);
      const long long sg = seg_of(seg, j, nseg);
      values[x] = seg_grad[(size_t)sg * D + e] * seg_scale(off, den, wts, j, sg, combiner);
    }
  }
}
template <typename SegT, int VQ>
__global__ void __launch_bounds__(TB) k_seg_expand(const float* __restrict__ seg_grad, const SegT* __restrict__ seg,
                                                   const unsigned* __restrict__ off, const float* __restrict__ den,
                                                   const float* __restrict__ wts, long long n, long long nseg, int D, int combiner,
                                                   float* __restrict__ values) {
  seg_expand_body<SegT, VQ>(seg_grad, seg, off, den, wts, n, nseg, D, combiner, values);
}

// ---------------------------------------------------------------------------------------------
// The sparse lookup and its backward over many tables in one launch per stage (blockIdx.y = table).  The per-table sparse
// arguments travel in an array of these, next to the MultiDesc array the batched tile and partition passes read (which
// stays as narrow as the hot batched kernels index it).  A table with nseg == 0 takes no part.
struct SparseDesc {
  const void* seg;         // [n] segment ids (one dtype for the whole call)
  const float* wts;        // [n] or null
  unsigned* off;           // [nseg + 1] the table's Workspace::seg_off
  float* den;              // [nseg] the table's Workspace::seg_den (backward, weighted mean / sqrtn)
  const float* seg_grad;   // backward: [nseg, dim]
  float* out;              // forward: [nseg, dim]; backward: values [n, dim]
  long long n, nseg;
};
template <typename SegT>
__global__ void __launch_bounds__(TB) k_seg_offsets_multi(const SparseDesc* __restrict__ descs) {
  const SparseDesc& d = descs[blockIdx.y];
  if (d.nseg == 0) return;
  seg_offsets_body(reinterpret_cast<const SegT*>(d.seg), d.n, d.nseg, d.off);
}
template <int VQ>
__global__ void __launch_bounds__(TB) k_seg_combine_e_multi(const MultiDesc* __restrict__ mdescs,
                                                            const SparseDesc* __restrict__ descs, int combiner) {
  const MultiDesc& m = mdescs[blockIdx.y];
  const SparseDesc& d = descs[blockIdx.y];
  if (d.nseg == 0) return;
  seg_combine_e_body<VQ>(m.a.tv, m.w.pos_ent, m.w.ent_b, m.w.ent_key, d.off, d.wts, d.nseg, combiner, d.out);
}
__global__ void __launch_bounds__(TB) k_seg_den_multi(const SparseDesc* __restrict__ descs, int combiner) {
  const SparseDesc& d = descs[blockIdx.y];
  if (d.nseg == 0 || !d.wts) return;
  seg_den_body(d.off, d.wts, d.nseg, combiner, d.den);
}
template <typename SegT, int VQ>
__global__ void __launch_bounds__(TB) k_seg_expand_multi(const SparseDesc* __restrict__ descs, int D, int combiner) {
  const SparseDesc& d = descs[blockIdx.y];
  if (d.nseg == 0) return;
  seg_expand_body<SegT, VQ>(d.seg_grad, reinterpret_cast<const SegT*>(d.seg), d.off, d.den, d.wts, d.n, d.nseg, D, combiner,
                            d.out);
}

// ---------------------------------------------------------------------------------------------
// The position records of the sharded sparse apply (kv_types.h SegSrc / SegDesc; kv_sums_seg.hip sums from them): what
// k_seg_expand computes per values row, kept per POSITION instead — pseg[j] = the clamped segment (seg_of), pscale[j] =
// seg_scale(j).  The offsets and denominators in front of it are the backward's own bodies, so a scale is the same bits as
// the one kv_lookup_sparse_grad multiplies by.  The batched forms read a SegDesc array (blockIdx.y = table; n == 0: no part).
template <typename SegT>
__device__ __forceinline__ void pos_records_body(const SegT* __restrict__ seg, const unsigned* __restrict__ off,
                                                 const float* __restrict__ den, const float* __restrict__ wts, long long n,
                                                 long long nseg, int combiner, int* __restrict__ pseg, float* __restrict__ pscale) {
  for (long long j = (long long)blockIdx.x * TB + threadIdx.x; j < n; j += (long long)gridDim.x * TB) {
    const long long sg = seg_of(seg, j, nseg);
    pseg[j] = (int)sg;
    pscale[j] = seg_scale(off, den, wts, j, sg, combiner);
  }
}
template <typename SegT>
__global__ void __launch_bounds__(TB) k_pos_records(SegDesc d, int combiner) {
  pos_records_body(reinterpret_cast<const SegT*>(d.seg), d.off, d.den, d.wts, d.n, d.nseg, combiner, d.pseg, d.pscale);
}
template <typename SegT>
__global__ void __launch_bounds__(TB) k_pos_offsets_multi(const SegDesc* __restrict__ descs) {
  const SegDesc& d = descs[blockIdx.y];
  if (d.n == 0) return;
  seg_offsets_body(reinterpret_cast<const SegT*>(d.seg), d.n, d.nseg, d.off);
}
__global__ void __launch_bounds__(TB) k_pos_den_multi(const SegDesc* __restrict__ descs, int combiner) {
  const SegDesc& d = descs[blockIdx.y];
  if (d.n == 0 || !d.den) return;   // (den: named where the table has weights and the combiner divides)
  seg_den_body(d.off, d.wts, d.nseg, combiner, d.den);
}
template <typename SegT>
__global__ void __launch_bounds__(TB) k_pos_records_multi(const SegDesc* __restrict__ descs, int combiner) {
  const SegDesc& d = descs[blockIdx.y];
  if (d.n == 0) return;
  pos_records_body(reinterpret_cast<const SegT*>(d.seg), d.off, d.den, d.wts, d.n, d.nseg, combiner, d.pseg, d.pscale);
}
