// kv_route.h — the sharded layer's own kernels (included by kv_shard.hip only, after kv_device.h): the routing rule's
// counting sort of ids by owner rank and the fixed-capacity exchange segments (k_owner_*, k_seg_headers), and the sharded
// lookup's output rows from the records that came back (k_shard_finish) or their combination into segments
// (k_shard_finish_sparse), and the owner's read-only serve of the records it received (k_shard_serve_zeros).
#pragma once

// ------------------------------------------------------------------------------------------
// multi-GPU routing: stable-by-tile counting sort of ids by owner rank (owner_rank, kv_device.h;
// kernels/utility.h:90-107).  world <= 64.  hist is [world][ntiles] (owner-major for the scan).
// ------------------------------------------------------------------------------------------
template <typename IdT>
__global__ void __launch_bounds__(TB) k_owner_hist(const IdT* __restrict__ ids, long long n, int world, int rule,
                                                   unsigned ntiles, unsigned* __restrict__ hist,
                                                   const long long* __restrict__ n_dev) {
  if (n_dev) n = min(n, *n_dev);   // the list's length is still on the device (kv_unique without a sync)
  __shared__ unsigned h[MAXW];
  if (threadIdx.x < MAXW) h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RT;
#pragma unroll
  for (int k = 0; k < RT / TB; ++k) {
    const long long i = base + k * TB + threadIdx.x;
    if (i < n) atomicAdd(&h[owner_rank(load_id(ids, (size_t)i), world, rule)], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < world) hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// one block: exclusive scan of hist in (owner, tile) order -> base offsets; counts[w] = ids owned by w
__global__ void __launch_bounds__(1024) k_owner_scan(unsigned* __restrict__ hist, unsigned total,
                                                     unsigned ntiles, int world, long long* __restrict__ counts) {
  __shared__ unsigned wtot[17];
  const unsigned per = (total + 1023) / 1024;
  const unsigned b0 = min(total, threadIdx.x * per), b1 = min(total, b0 + per);
  unsigned sum = 0;
  for (unsigned i = b0; i < b1; ++i) sum += hist[i];
  unsigned tot;
  unsigned run = block_excl_scan<16>(sum, wtot, &tot);
  for (unsigned i = b0; i < b1; ++i) { const unsigned c = hist[i]; hist[i] = run; run += c; }
  __syncthreads();
  if ((int)threadIdx.x < world) {
    const unsigned lo = hist[(size_t)threadIdx.x * ntiles];
    const unsigned hi = ((int)threadIdx.x + 1 < world) ? hist[(size_t)(threadIdx.x + 1) * ntiles] : tot;
    counts[threadIdx.x] = (long long)hi - (long long)lo;
  }
}

template <typename IdT>
__global__ void __launch_bounds__(TB) k_owner_scatter(const IdT* __restrict__ ids, long long n, int world, int rule,
                                                      unsigned ntiles, const unsigned* __restrict__ base_off,
                                                      long long* __restrict__ out_ids, int* __restrict__ perm,
                                                      const long long* __restrict__ n_dev,
                                                      const int* __restrict__ counts_in,
                                                      long long* __restrict__ pairs_out, int* __restrict__ pos_out) {
  if (n_dev) n = min(n, *n_dev);
  __shared__ unsigned h[MAXW];
  if ((int)threadIdx.x < world) h[threadIdx.x] = base_off[(size_t)threadIdx.x * ntiles + blockIdx.x];
  __syncthreads();
  const long long base = (long long)blockIdx.x * RT;
#pragma unroll
  for (int k = 0; k < RT / TB; ++k) {
    const long long i = base + k * TB + threadIdx.x;
    if (i < n) {
      const long long id = load_id(ids, (size_t)i);
      const unsigned pos = atomicAdd(&h[owner_rank(id, world, rule)], 1u);
      out_ids[pos] = id;
      perm[pos] = (int)i;
      // optional extras of the sharded lookup: the exchange payload (id, occurrence count) in
      // bucket order, and where input position i went (the inverse of perm)
      if (pairs_out) { pairs_out[2 * (size_t)pos] = id; pairs_out[2 * (size_t)pos + 1] = counts_in ? (long long)counts_in[i] : 1ll; }
      if (pos_out) pos_out[i] = (int)pos;
    }
  }
}
// The sharded lookup's exchange payload in FIXED-CAPACITY segments (no size collective, no host sync): owner d's
// segment is seg[d][0 .. C]: record 0 = header {pairs in the segment, 0}, records 1 .. = (id, occurrence count).
// A record whose count is 0 is skipped by the owner's tile pass, so padding costs nothing but its bytes.  slot_of[u]
// = where unique id u went (its row comes back at the same place).  More than C ids for one owner: the extra
// ones are dropped and *overflow is raised (the host doubles C; hashed ownership keeps this from happening).
__global__ void __launch_bounds__(TB) k_owner_scatter_fixed(const long long* __restrict__ ids, const int* __restrict__ cnts,
                                                            long long n, int world, int rule,
                                                            unsigned ntiles, const unsigned* __restrict__ base_off,
                                                            unsigned C, long long* __restrict__ seg, int* __restrict__ slot_of,
                                                            unsigned* __restrict__ overflow) {
  __shared__ unsigned h[MAXW];
  if ((int)threadIdx.x < world)   // rank inside the owner's bucket = global offset - the bucket's start
    h[threadIdx.x] = base_off[(size_t)threadIdx.x * ntiles + blockIdx.x] - base_off[(size_t)threadIdx.x * ntiles];
  __syncthreads();
  const long long base = (long long)blockIdx.x * RT;
#pragma unroll
  for (int k = 0; k < RT / TB; ++k) {
    const long long i = base + k * TB + threadIdx.x;
    if (i < n && cnts[i] > 0) {   // the list has gaps (sparse unique numbers): a count of 0 names no key
      const long long id = ids[i];
      const unsigned d = owner_rank(id, world, rule);
      const unsigned r = atomicAdd(&h[d], 1u);
      if (r < C) {
        const size_t slot = (size_t)d * (C + 1) + 1 + r;
        seg[2 * slot] = id;
        seg[2 * slot + 1] = (long long)cnts[i];
        slot_of[i] = (int)slot;
      } else {
        slot_of[i] = 0;        // record 0 is a header: its "row" is never a real one
        atomicExch(overflow, 1u);
      }
    }
  }
}
// the segments' headers {records in the segment (at most C), 0}
__global__ void k_seg_headers(const long long* __restrict__ counts, int world, unsigned C, long long* __restrict__ seg,
                              unsigned* __restrict__ need) {
  const int d = threadIdx.x;
  if (need && d == 0) *need = 0u;
  __syncthreads();
  if (d < world) {
    seg[2 * (size_t)d * (C + 1)] = counts[d] < (long long)C ? counts[d] : (long long)C;
    seg[2 * (size_t)d * (C + 1) + 1] = 0;
    if (need) atomicMax(need, (unsigned)(counts[d] < 0x7FFFFFFFll ? counts[d] : 0x7FFFFFFFll));
  }
}
// k_owner_hist over the sparse unique list of the sharded route (entries with a count of 0 name no key)
__global__ void __launch_bounds__(TB) k_owner_hist_u32(const long long* __restrict__ ids, const int* __restrict__ cnts, long long n,
                                                       int world, int rule, unsigned ntiles, unsigned* __restrict__ hist) {
  __shared__ unsigned h[MAXW];
  if (threadIdx.x < MAXW) h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RT;
#pragma unroll
  for (int k = 0; k < RT / TB; ++k) {
    const long long i = base + k * TB + threadIdx.x;
    if (i < n && cnts[i] > 0) atomicAdd(&h[owner_rank(ids[i], world, rule)], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < world) hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// k_shard_finish: the sharded lookup's output rows from the records that came back
// ------------------------------------------------------------------------------------------
// out[i] = rows[slot_of[uniq_of_entry[tile * TILE + pos_ent[i]]]]: position -> its entry in the tile (k_ltile<NOTABLE>
// filed it) -> the entry's distinct-id number (k_papply PA_UNIQUE wrote it to ent_b) -> the record the id was sent in
// -> the row the owner returned.  A wave takes 64 positions, lane l resolves position l, the rows go VQ lanes per row
// with streaming stores (the copy of goz_wave).
template <int VQ, int CW = 4>
__device__ __forceinline__ void shard_finish_body(const unsigned short* __restrict__ pos_ent, const unsigned* __restrict__ ent_u,
                                                  const int* __restrict__ slot_of, const float* __restrict__ rows,
                                                  float* __restrict__ out, long long n, int dim,
                                                  const float* __restrict__ rows_self, unsigned self_lo, unsigned self_len) {
  constexpr int RW = 64 / VQ;
  const int lane = threadIdx.x & 63;
  const int v = lane % VQ, sub = lane / VQ;
  const int D4 = dim >> 2;   // float4 per row (<= VQ: lanes past it are masked)
  const bool vlive = v < D4;
  const int vv = vlive ? v : 0;
  const long long nwaves = (long long)gridDim.x * (TB / 64);
  for (long long r0 = ((long long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) * 64; r0 < n; r0 += nwaves * 64) {
    const long long i = r0 + lane;
    unsigned rec = 0;   // record 0: a header's row (zeros) — positions past the end, ids that found no room in their segment
    if (i < n) {
      const unsigned e = pos_ent[i];
      if (e != 0xFFFFu) rec = (unsigned)slot_of[ent_u[(size_t)(i / TILE) * TILE + e]];
    }
#pragma unroll
    for (int j0 = 0; j0 < VQ; j0 += CW) {
      float4 val[CW];
      unsigned rj[CW];
#pragma unroll
      for (int j = 0; j < CW && j0 + j < VQ; ++j) rj[j] = __shfl(rec, (j0 + j) * RW + sub);
#pragma unroll
      for (int j = 0; j < CW && j0 + j < VQ; ++j)   // (records [self_lo, self_lo + self_len): this rank's own segment, read where the serve wrote it)
        val[j] = reinterpret_cast<const float4*>((((unsigned)rj[j] - self_lo < self_len) ? rows_self : rows) + (size_t)rj[j] * dim)[vv];
#pragma unroll
      for (int j = 0; j < CW && j0 + j < VQ; ++j) {
        const long long ii = r0 + (j0 + j) * RW + sub;
        if (ii < n && vlive) {
          float4* dst = reinterpret_cast<float4*>(out + (size_t)ii * dim) + v;
          __builtin_nontemporal_store(val[j].x, &dst->x); __builtin_nontemporal_store(val[j].y, &dst->y);
          __builtin_nontemporal_store(val[j].z, &dst->z); __builtin_nontemporal_store(val[j].w, &dst->w);
        }
      }
    }
  }
}
template <int VQ, int CW = 4>
__global__ void __launch_bounds__(TB) k_shard_finish(const unsigned short* __restrict__ pos_ent, const unsigned* __restrict__ ent_u,
                                                     const int* __restrict__ slot_of, const float* __restrict__ rows,
                                                     float* __restrict__ out, long long n, int dim,
                                                     const float* __restrict__ rows_self, unsigned self_lo, unsigned self_len) {
  shard_finish_body<VQ, CW>(pos_ent, ent_u, slot_of, rows, out, n, dim, rows_self, self_lo, self_len);
}
// several tables of one row geometry in one launch (blockIdx.y = table)
struct FinishDesc {
  const unsigned short* pos_ent;
  const unsigned* ent_u;
  const int* slot_of;
  const float* rows;
  float* out;
  long long n;
  const float* rows_self;
  unsigned self_lo, self_len;
  int dim, pad;
};
template <int VQ, int CW = 4>
__global__ void __launch_bounds__(TB) k_shard_finish_multi(const FinishDesc* __restrict__ descs) {
  const FinishDesc d = descs[blockIdx.y];
  shard_finish_body<VQ, CW>(d.pos_ent, d.ent_u, d.slot_of, d.rows, d.out, d.n, d.dim, d.rows_self, d.self_lo, d.self_len);
}

// ------------------------------------------------------------------------------------------
// k_shard_finish_sparse: the COMBINING finish (kv_shard_lookup_finish_sparse and the sparse whole ops) —
//   out[s] = combine_j( w_j * row_j ) over the positions j of segment s, in position order,
// row_j = the row k_shard_finish writes for position j, read where that kernel reads it.  The [n, dim] rows are never
// written: the records' rows already sit in the receive buffer (this rank's own in the send buffer), one launch walks the
// segments and writes [num_segments, dim] once.
//  * the segment walk is lsz_body's (kv_op_kernels.h): a group of VQ lanes owns a segment, 64 / VQ segments per wave step,
//    the bounds from lsz_bound (kv_device.h) by the group's lane 0, the neighbour's bound by shuffle, the wave's last bound
//    searched beside them.  No LDS, no atomics, no float reduction across lanes; out is written once, streaming.
//  * the row fetch is shard_finish_body's: lane u of the group resolves position pos + u (pos_ent -> 0xFFFF: record 0, else
//    slot_of[ent_u[tile base + entry]]), records and weights go round the group by shuffle, up to 4 rows in flight per lane
//    (float4 loads from rows, or rows_self for this rank's own in-place segment); the additions stay in position order.
//  * VQ = row_lanes(dim): dims that are not a power of two times 4 (12, 20, 100 ...) run the next instantiation with the
//    lanes v >= dim / 4 masked.  A masked lane still resolves its position — the chunk is VQ positions whatever the dim —
//    and reads float4 0 of the rows it is handed; it accumulates into registers nobody stores.
// A chunk pays four dependent loads (pos_ent -> ent_u -> slot_of -> row) where lsz_body pays three (id -> entry -> row),
// and is not pipelined across chunks either: see DESIGN.md §4 for what was measured.
// ------------------------------------------------------------------------------------------
struct FinishSparseDesc {
  FinishDesc f;          // f.out: [nseg, dim]; f.n: the routed batch's length (0: every segment is empty)
  const void* seg;       // [n] ascending, int32 or int64
  const float* wts;      // [n] or null
  long long nseg;
};
template <int VQ>
__device__ __forceinline__ void shard_finish_sparse_body(const FinishSparseDesc& d, int seg32, int combiner) {
  constexpr int G = 64 / VQ;                // segments per wave and step
  constexpr int SU = VQ < 4 ? VQ : 4;       // rows in flight per lane
  const FinishDesc& f = d.f;
  const void* __restrict__ seg = d.seg;
  const float* __restrict__ wts = d.wts;
  const unsigned short* __restrict__ pos_ent = f.pos_ent;
  const unsigned* __restrict__ ent_u = f.ent_u;
  const int* __restrict__ slot_of = f.slot_of;
  const int dim = f.dim, n = (int)f.n;
  const long long nseg = d.nseg;
  const int lane = threadIdx.x & 63;
  const int v = lane % VQ, sub = lane / VQ, gbase = sub * VQ;
  const bool vlive = v < (dim >> 2);        // float4 per row <= VQ: lanes past it are masked
  const int vv = vlive ? v : 0;
  const long long wave = (long long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (TB / 64);
  for (long long base = wave * G; base < nseg; base += nwaves * G) {   // wave-uniform
    const long long sgi = base + sub;
    // the bounds: lane 0 of each group its segment's first position, the wave's last bound beside them
    int b0 = 0, b1 = 0;
    if (v == 0) b0 = lsz_bound(seg, seg32, n, nseg, sgi);
    else if (VQ > 1 && lane == 64 - VQ + 1) b0 = lsz_bound(seg, seg32, n, nseg, base + G);
    if (VQ == 1 && lane == 63) b1 = lsz_bound(seg, seg32, n, nseg, base + G);
    const int lo = __shfl(b0, gbase);
    const int hi_next = __shfl(b0, sub < G - 1 ? gbase + VQ : gbase);
    const int hi_last = VQ > 1 ? __shfl(b0, 64 - VQ + 1) : __shfl(b1, 63);
    const int hi = sub < G - 1 ? hi_next : hi_last;
    const int len = sgi < nseg && hi > lo ? hi - lo : 0;   // (a list that is not ascending may give hi < lo: nothing is read)
    float wsum = 0.f, w2 = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned pos = (unsigned)lo;   // the chunk's first position; rem: the segment's positions from there on
    for (int rem = len; __any(rem > 0); rem -= VQ, pos += VQ) {
      // lane v: the record of position pos + v (record 0, weight 0 past the segment's end)
      unsigned rec = 0u;
      float wv = 0.f;
      if (v < rem) {
        const unsigned p = pos + v;
        wv = wts ? wts[p] : 1.f;
        const unsigned e = pos_ent[p];
        if (e != 0xFFFFu) rec = (unsigned)slot_of[ent_u[(size_t)(p / TILE) * TILE + e]];
      }
      for (int u0 = 0; u0 < VQ && __any(u0 < rem); u0 += SU) {
        unsigned ru[SU];
        float wu[SU];
        float4 x[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) { ru[u] = __shfl(rec, gbase + u0 + u); wu[u] = __shfl(wv, gbase + u0 + u); }
#pragma unroll
        for (int u = 0; u < SU; ++u)   // (records [self_lo, self_lo + self_len): this rank's own segment, read where the serve wrote it)
          x[u] = reinterpret_cast<const float4*>(((ru[u] - f.self_lo < f.self_len) ? f.rows_self : f.rows) + (size_t)ru[u] * dim)[vv];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          if (u0 + u >= rem) continue;
          acc.x += x[u].x * wu[u]; acc.y += x[u].y * wu[u]; acc.z += x[u].z * wu[u]; acc.w += x[u].w * wu[u];
          wsum += wu[u]; w2 += wu[u] * wu[u];
        }
      }
    }
    if (sgi >= nseg || !vlive) continue;
    float den = 1.f;
    if (combiner == 1) den = wsum; else if (combiner == 2) den = sqrtf(w2);
    if (combiner != 0 && (wts || len > 0)) { acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den; }
    float4* dst = reinterpret_cast<float4*>(f.out + (size_t)sgi * dim) + v;
    __builtin_nontemporal_store(acc.x, &dst->x); __builtin_nontemporal_store(acc.y, &dst->y);
    __builtin_nontemporal_store(acc.z, &dst->z); __builtin_nontemporal_store(acc.w, &dst->w);
  }
}
template <int VQ>
__global__ void __launch_bounds__(TB) k_shard_finish_sparse(FinishSparseDesc d, int seg32, int combiner) {
  shard_finish_sparse_body<VQ>(d, seg32, combiner);
}
// several tables of one row geometry in one launch (blockIdx.y = table); a table's blocks past its own segments leave at once
template <int VQ>
__global__ void __launch_bounds__(TB) k_shard_finish_sparse_multi(const FinishSparseDesc* __restrict__ descs, int seg32, int combiner) {
  const FinishSparseDesc d = descs[blockIdx.y];
  shard_finish_sparse_body<VQ>(d, seg32, combiner);
}

// ------------------------------------------------------------------------------------------
// k_shard_serve_zeros: the owner's READ-ONLY serve (kv_shard_lookup_serve_zeros) — rows[record] = the table's row of the
// record's id, or zeros where k_gather_or_zeros reads zeros (row 0: a key the index does not hold; a blacklisted key and one
// under the enter threshold are stored as zeros).  Nothing of the table is written: no insert, no frequency word, no stamp.
// ------------------------------------------------------------------------------------------
// The records are `world` segments of C + 1 (id, count) pairs (k_owner_scatter_fixed / k_papply PA_UNIQUE wrote them, the
// exchange moved them): record 0 of a segment is its header {records in the segment, 0}, records 1 .. cnt are live, the rest
// is padding.  Segment `self_seg` is read from pairs_self (this rank's own segment where it stayed in the send buffer), the
// others from pairs.  The work follows the LIVE records: the header counts (clamped to 0 .. C — nothing else of a peer's
// segment is trusted, and a count is only ever a loop bound) and their prefix sums sit in LDS, a dense index q walks the live
// records, q -> its segment by a search over the prefix, its record = q - prefix[segment] + 1.  Padding is neither probed
// nor written; the counts of the records are not read.  A wave step is goz_wave's (kv_op_kernels.h): lane l probes live
// record l, the home entries of the next step and the ids of the step after it are in flight, the rows go VQ lanes per row
// with the row and record numbers handed over by shuffle — with plain stores: the rows are read again at once, by the exchange
// and by this rank's own finish (as the training serve's, kv_fused.h).  Every segment's header row is written as zeros:
// k_shard_finish reads record 0 for an id that found no room in its segment.
struct ServeZerosDesc {
  TableDev t;
  const long long* pairs;        // [world][C + 1][2]
  const long long* pairs_self;   // segment self_seg is read here
  float* rows;                   // [world][C + 1][dim]
  unsigned C;
  int world;
  int self_seg;                  // -1: every segment is read from pairs
  int pad;
};
template <int VQ, int CWMAX = 4>
__device__ __forceinline__ void shard_serve_zeros_body(const ServeZerosDesc& d) {
  constexpr int RW = 64 / VQ;
  constexpr int CW = VQ < CWMAX ? VQ : CWMAX;
  const TableDev& t = d.t;
  const int lane = threadIdx.x & 63;
  const int v = lane % VQ, sub = lane / VQ;
  const int D4 = t.dim >> 2;   // float4 per row (<= VQ: lanes past it are masked)
  const bool vlive = v < D4;
  const int vv = vlive ? v : 0;
  const unsigned C = d.C, S = C + 1;
  const int world = d.world;
  auto seg_pairs = [&](int p) { return (p == d.self_seg ? d.pairs_self : d.pairs) + 2 * (size_t)p * S; };
  // pre[p] = live records in front of segment p; pre[MAXW] = all of them (segments past `world` hold none)
  __shared__ unsigned pre[MAXW + 1];
  if (threadIdx.x < 64) {
    long long c = lane < world ? seg_pairs(lane)[0] : 0ll;
    c = c < 0 ? 0ll : (c > (long long)C ? (long long)C : c);
    unsigned x = (unsigned)c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    pre[lane + 1] = x;
    if (lane == 0) pre[0] = 0u;
  }
  // the headers' rows: zeros (world * D4 float4, the first block's)
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < world * D4; i += TB)
      reinterpret_cast<float4*>(d.rows + (size_t)(i / D4) * S * t.dim)[i % D4] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const long long total = pre[MAXW];
  // live record q -> its id; *g = its record number in the buffers (0 past the end: never written)
  auto load_rec = [&](long long q, unsigned* g) -> long long {
    *g = 0u;
    if (q >= total) return EMPTY_KEY;
    int p = 0;   // the last segment whose prefix is <= q (empty segments in front of it share that prefix: skipped)
#pragma unroll
    for (int step = MAXW / 2; step > 0; step >>= 1)
      if (pre[p + step] <= (unsigned)q) p += step;
    const unsigned rec = (unsigned)q - pre[p] + 1u;   // 1 .. count of segment p <= C
    *g = (unsigned)p * S + rec;
    return seg_pairs(p)[2 * (size_t)rec];
  };
  const long long nwaves = (long long)gridDim.x * (TB / 64);
  const long long stride = nwaves * 64;
  long long q0 = ((long long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) * 64;
  if (q0 >= total) return;
  unsigned g1, g2;
  long long k1 = load_rec(q0 + lane, &g1);            // step i + 1's id (first: step 0's)
  long long k2 = load_rec(q0 + stride + lane, &g2);   // step i + 2's
  unsigned long long p1 = home_of(t, k1, mix64((unsigned long long)k1));
  Entry e1 = load_entry(&t.entries[p1]);
  for (; q0 < total; q0 += stride) {
    // this step's rows: finish the probe started one step ago (row 0 reads zeros: misses, lanes past the end)
    const unsigned rr = (q0 + lane < total) ? table_find_from(t, k1, p1, e1) : 0u;
    const unsigned gg = g1;
    // next step: its home entries leave now, the ids of the step after it too
    k1 = k2; g1 = g2;
    p1 = home_of(t, k1, mix64((unsigned long long)k1));
    if (q0 + stride < total) e1 = load_entry(&t.entries[p1]);
    k2 = load_rec(q0 + 2 * stride + lane, &g2);
#pragma unroll
    for (int j0 = 0; j0 < VQ; j0 += CW) {
      float4 val[CW];
      unsigned rj[CW], gj[CW];
#pragma unroll
      for (int j = 0; j < CW; ++j) { rj[j] = __shfl(rr, (j0 + j) * RW + sub); gj[j] = __shfl(gg, (j0 + j) * RW + sub); }
#pragma unroll
      for (int j = 0; j < CW; ++j) val[j] = reinterpret_cast<const float4*>(row_ptr(t, rj[j]))[vv];
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        const long long qq = q0 + (j0 + j) * RW + sub;
        if (qq < total && vlive) {
          float4* dst = reinterpret_cast<float4*>(d.rows + (size_t)gj[j] * t.dim) + v;
          // (by component — still one 16-byte store: a whole-struct copy out of val[] keeps the array in memory, 16 KiB of LDS per block)
          dst->x = val[j].x; dst->y = val[j].y; dst->z = val[j].z; dst->w = val[j].w;
        }
      }
    }
  }
}
// several tables of one row geometry in one launch (blockIdx.y = table); a single table is the one-table case
template <int VQ>
__global__ void __launch_bounds__(TB) k_shard_serve_zeros(const ServeZerosDesc* __restrict__ descs) {
  const ServeZerosDesc d = descs[blockIdx.y];
  shard_serve_zeros_body<VQ>(d);
}
