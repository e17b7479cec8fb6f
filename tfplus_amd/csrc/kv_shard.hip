// kv_shard.hip — sharded tables on the table core (kv_host.h): hashed ownership, fixed-capacity exchange, RCCL over xGMI
// (SURVEY.md §8e).  kv_comm_* (RCCL by dlopen, grouped send / recv; or the caller's transport), kv_shard_* (route / serve /
// finish phases and the whole ops; the read-only lookup is the training one with another serve: serve_zeros_impl), the
// batched kv_multi_shard_* ops, and kv_bucket_by_owner, the routing rule's stand-alone form.  The only unit that knows RCCL; its own kernels are kv_route.h's.
// One body per phase over the tables todo[0..m), whose one-table case (descriptor by value, nothing staged) is the phase's C entry
// point: route_impl, serve_zeros_impl, finish_impl, finish_sparse_impl, presum_impl, presum_sparse_impl (arguments: *_desc); the
// training serve and the owner's apply are the table ops' own.  One body per whole op (shards_lookup, shards_apply): the single
// forms are its one-table case, the sparse lookups those with the combining finish, the sparse applies those whose pre-sum reads
// segment gradients (SparseArgs); segment sizes: shard_bytes, batched groups: groups_of.  A shard's last batch: kv_shard_batch.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include "kv_host.h"
#include "kv_shard_batch.h"

using namespace kvhip_internal;

struct kv_comm {
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0, device = 0;
  hipStream_t stream = nullptr;      // the collectives' own stream
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  // host-staged transport (kv_comm_create_staged): the caller's callbacks move the segments
  kv_comm_exchange_fn xfn = nullptr;
  kv_comm_max_fn mfn = nullptr;
  void* user = nullptr;
  bool self_via_rccl = false;        // kv_comm_set_self_via_rccl: this rank's own segment goes through RCCL too
};

struct kv_shard {
  kv_table* table = nullptr;         // this rank's share of the rows
  kv_table* route = nullptr;         // owns the workspace of the local unique index (no rows of its own)
  int world = 1, rank = 0, rule = KV_OWNER_HASH;
  long long max_ids = 0;
  unsigned C = 0;                    // (id, count) records per peer segment, header not counted
  long long* uniq = nullptr;         // [max_ids]
  int* ucnt = nullptr;               // [max_ids]
  int* slot_of = nullptr;            // [max_ids] unique id -> record in the send buffer
  long long* send_pairs = nullptr;   // [world][C + 1][2]
  long long* recv_pairs = nullptr;
  float* send_rows = nullptr;        // [world][C + 1][dim]
  float* recv_rows = nullptr;
  long long* counts = nullptr;       // [world]
  unsigned* hist = nullptr;          // [world][tiles]
  unsigned* gcount = nullptr;        // [MAXW + 1] the route's per-owner record counters (k_papply PA_UNIQUE; zero between launches)
  unsigned* overflow = nullptr;      // pinned, mapped: a segment was too small for a batch
  unsigned long long overflows = 0;  // batches reported so far
  unsigned* need = nullptr;          // device [2]: the largest segment the last routed batch wanted; the same over all ranks
  unsigned* need_host = nullptr;     // pinned copy of need[1]
  bool lossless = true;              // ranks agree on the capacity before every exchange (the default: nothing can be lost);
                                     // kv_shard_set_lossless(shard, 0) opts into the synchronisation-free mode
  unsigned long long grows = 0;      // times the capacity was raised
  ShardBatch batch;                  // the batch last routed and served: written only through its transitions (kv_shard_batch.h)
  const kv_comm* verified = nullptr; // the communicator whose ranks were seen to agree on world / capacity / dim
  hipEvent_t ev_fork = nullptr, ev_done = nullptr;
  int ranks_seen = 0;                // ranks whose handshake record arrived in the first exchange (shard_verify)
  // per-phase timing of the whole ops (kv_shard_profile): events on the communicator's stream at the phase boundaries of
  // every prof_every-th step; one sample in flight, collected by the next sampled call or by the read
  int prof_every = 0;
  unsigned prof_seq_l = 0, prof_seq_a = 0;
  hipEvent_t pev[10] = {};           // lookup: [0..5] = 5 phases; apply: [6..9] = 3 phases
  bool pend_l = false, pend_a = false;
  double psum[KV_SHARD_PHASES] = {};
  long long pcnt[KV_SHARD_PHASES] = {};
};

namespace {

#include "kv_device.h"
#include "kv_route.h"

// RCCL is reached through dlopen: the copy the process already holds (PyTorch bundles one under the same soname)
// is reused, so there is one RCCL per process; nothing links against it when the table is not sharded
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;   // lossless mode only
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
};

RcclApi* rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    // PyTorch's wheel carries its RCCL under the soname librccl.so, ROCm's own is librccl.so.1: whichever the process
    // already holds wins, so that there is one RCCL (one set of xGMI channels) per process
    for (const char* name : {"librccl.so", "librccl.so.1"})
      if ((api.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!api.lib)
      for (const char* name : {"librccl.so.1", "librccl.so"})
        if ((api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!api.lib) return;
    auto sym = [&](const char* n) { return dlsym(api.lib, n); };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(sym("ncclAllReduce"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.GroupStart && api.GroupEnd && api.Send && api.Recv;
  });
  return &api;
}

static const char* nccl_err(ncclResult_t r) { return rccl()->GetErrorString ? rccl()->GetErrorString(r) : "?"; }
#define NCCL_TRY(expr)                                                                \
  do {                                                                                \
    ncclResult_t _r = (expr);                                                         \
    if (_r != ncclSuccess) return fail(KV_INTERNAL, "%s failed: %s", #expr, nccl_err(_r)); \
  } while (0)

// a new communicator's fields, its own stream and events (its device is current); false: they could not be created
static bool comm_init(kv_comm* c, int world, int rank, int device) {
  c->world = world; c->rank = rank; c->device = device;
  return hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming) == hipSuccess;
}

// the segments really travel (RCCL or the caller's transport); else: a world of one whose exchange is a device copy
static inline bool wired(const kv_comm* c) { return c->comm != nullptr || c->xfn != nullptr; }

// phase timing of the whole sharded ops (kv_shard_profile): see kv_shard
void shard_prof_collect(kv_shard* sh, bool lookup) {
  bool& pend = lookup ? sh->pend_l : sh->pend_a;
  if (!pend) return;
  const int e0 = lookup ? 0 : 6, np = lookup ? 5 : 3, p0 = lookup ? 0 : 5;
  if (hipEventSynchronize(sh->pev[e0 + np]) == hipSuccess)
    for (int i = 0; i < np; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sh->pev[e0 + i], sh->pev[e0 + i + 1]) == hipSuccess) { sh->psum[p0 + i] += ms; sh->pcnt[p0 + i] += 1; }
    }
  pend = false;
}

// does this call carry markers?  (collects the previous sample first: its events are about to be reused)
bool shard_prof_begin(kv_shard* sh, bool lookup) {
  if (sh->prof_every <= 0) return false;
  unsigned& seq = lookup ? sh->prof_seq_l : sh->prof_seq_a;
  if ((seq++ % (unsigned)sh->prof_every) != 0u) return false;
  shard_prof_collect(sh, lookup);
  for (hipEvent_t& e : sh->pev)
    if (!e && hipEventCreate(&e) != hipSuccess) return false;
  return true;
}

inline void shard_prof_mark(kv_shard* sh, bool on, int ev, hipStream_t w) { if (on) hipEventRecord(sh->pev[ev], w); }

void shard_free_buffers(kv_shard* sh) {
  hipFree(sh->send_pairs); hipFree(sh->recv_pairs); hipFree(sh->send_rows); hipFree(sh->recv_rows);
  sh->send_pairs = sh->recv_pairs = nullptr; sh->send_rows = sh->recv_rows = nullptr;
}

static int64_t shard_nrec(const kv_shard* sh) { return (int64_t)sh->world * (sh->C + 1); }   // the records of a send or receive buffer

int shard_alloc_buffers(kv_shard* sh, unsigned C) {
  const size_t rec = (size_t)sh->world * (C + 1);
  if (rec > (1ull << 21)) return fail(KV_INVALID_ARGUMENT, "peer_capacity %u x world %d exceeds 2^21 records per exchange", C, sh->world);
  shard_free_buffers(sh);
  HIP_TRY(hipMalloc(&sh->send_pairs, rec * 16));
  HIP_TRY(hipMalloc(&sh->recv_pairs, rec * 16));
  HIP_TRY(hipMalloc(&sh->send_rows, rec * sh->table->dim * sizeof(float)));
  HIP_TRY(hipMalloc(&sh->recv_rows, rec * sh->table->dim * sizeof(float)));
  HIP_TRY(hipMemset(sh->send_pairs, 0, rec * 16));
  HIP_TRY(hipMemset(sh->recv_pairs, 0, rec * 16));
  sh->C = C;
  return KV_OK;
}

// the lossless agreements' grow step: a route wanted `need` records in one segment, more than C (every rank saw that number)
static int shard_grow(kv_shard* sh, unsigned need, long long max_ids) {
  if (int rc = shard_alloc_buffers(sh, (unsigned)std::min<long long>(max_ids, (long long)need + need / 4 + 64))) return rc;
  *reinterpret_cast<volatile unsigned*>(sh->overflow) = 0;   // raised by the attempt that is now repeated
  ++sh->grows;
  return KV_OK;
}

// bytes_per_peer bytes to / from every rank: grouped ncclSend / ncclRecv (xGMI is point to point: one pair per
// link), on the communicator's own stream, behind everything `stream` was given and in front of what it gets next.
// nseg buffers (the tables of a multi-table step) go out in ONE group: RCCL runs a group's sends and receives as one
// launch, so 40 tables cost one exchange, not 40.
// stay: this rank's own segment is read from the send buffer by the kernels themselves
struct Seg { const void* send; void* recv; int64_t bytes_per_peer; bool stay; };
static int comm_exchange(kv_comm* c, int nseg, const Seg* seg, hipStream_t s) {
  if (c->xfn) {   // the caller's transport: everything queued so far has run, then the segments move on the host's clock
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < nseg; ++k) {
      const int r = c->xfn(c->user, seg[k].send, seg[k].recv, seg[k].bytes_per_peer);
      if (r) return fail(KV_INTERNAL, "the staged exchange failed (callback returned %d)", r);
    }
    return KV_OK;
  }
  if (!c->comm) {   // world of one without RCCL
    for (int k = 0; k < nseg; ++k)
      if (!seg[k].stay)
        HIP_TRY(hipMemcpyAsync(seg[k].recv, seg[k].send, (size_t)seg[k].bytes_per_peer, hipMemcpyDeviceToDevice, s));
    return KV_OK;
  }
  const bool hop = s != c->stream;   // the sharded ops run on the communicator's stream themselves: no hop
  if (hop) {
    HIP_TRY(hipEventRecord(c->ev_in, s));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_in, 0));
  }
  // this rank's own segment never meets RCCL: it stays in place (stay: the sharded whole ops read it in the send
  // buffer) or is a device copy at HBM speed, queued in front of the group — unless kv_comm_set_self_via_rccl asked for
  // it to go through ncclSend / ncclRecv like a peer's
  const bool self_rccl = c->self_via_rccl;
  if (!self_rccl)
    for (int k = 0; k < nseg; ++k)
      if (!seg[k].stay) {
        const size_t b = (size_t)seg[k].bytes_per_peer;
        HIP_TRY(hipMemcpyAsync((char*)seg[k].recv + c->rank * b, (const char*)seg[k].send + c->rank * b, b, hipMemcpyDeviceToDevice, c->stream));
      }
  const bool grouped = c->world > 1 || self_rccl;
  if (grouped) NCCL_TRY(rccl()->GroupStart());
  ncclResult_t bad = ncclSuccess;   // a failed Send / Recv must not leave the group open on this communicator
  for (int p = 0; p < c->world && bad == ncclSuccess; ++p) {
    if (p == c->rank && !self_rccl) continue;
    for (int k = 0; k < nseg && bad == ncclSuccess; ++k) {   // peer-major: both ends of a pair post the tables in the same order
      const size_t b = (size_t)seg[k].bytes_per_peer;
      bad = rccl()->Send((const char*)seg[k].send + p * b, b, ncclChar, p, c->comm, c->stream);
      if (bad == ncclSuccess) bad = rccl()->Recv((char*)seg[k].recv + p * b, b, ncclChar, p, c->comm, c->stream);
    }
  }
  if (grouped) {
    const ncclResult_t e = rccl()->GroupEnd();
    if (bad == ncclSuccess) bad = e;
  }
  if (bad != ncclSuccess) return fail(KV_INTERNAL, "grouped send / recv failed: %s", nccl_err(bad));
  if (hop) {
    HIP_TRY(hipEventRecord(c->ev_out, c->stream));
    HIP_TRY(hipStreamWaitEvent(s, c->ev_out, 0));
  }
  return KV_OK;
}

// A batch that sent one owner more than peer_capacity distinct ids raised the pinned flag (the surplus read zeros).
// It is reported by the first call that ENDS after the flag landed — after that call has queued all its work, so a
// rank that reports keeps step with its peers (an early return would leave them waiting in the exchange).  The
// capacity is not changed here: it must change on every rank at once.
// (`seen` is the flag as the call found it when it STARTED: a batch's own overflow is reported by the next call, never
// by itself — which call reports does not depend on how fast the kernels ran.)
static unsigned shard_take_flag(kv_shard* sh) {
  return __atomic_exchange_n(sh->overflow, 0u, __ATOMIC_RELAXED);
}

static int shard_late_report(kv_shard* sh, unsigned seen) {
  if (!seen) return KV_OK;
  ++sh->overflows;
  return fail(KV_RESOURCE_EXHAUSTED, "an earlier sharded batch sent one owner more than peer_capacity (%u) distinct ids: the surplus "
                                     "ids read zeros and their gradients were dropped (this call itself was queued in full); "
                                     "create the shards with a larger peer_capacity on every rank", sh->C);
}

// The whole-op entry points (kv_shard_lookup / kv_shard_apply / kv_multi_shard_*) do the exchanges themselves, so they
// leave this rank's own segments where they are: every kernel that reads a receive buffer downstream (the owner lookup's
// tile pass, the finish, the owner apply's tile sums and k_papply) takes records [rank * (C + 1), +C + 1) from the send
// buffer.
static bool shard_can_stay(const kv_shard* sh) {
  return shard_nrec(sh) <= FUSED_MAX_N;
}

// ... as the owner ops are told (ws_view): the (id, count) records, and for the apply (grad) the summed gradient rows
static SelfSegment shard_self(const kv_shard* sh, bool grad) {
  if (!sh->batch.own_segment_stays()) return SelfSegment{};
  return SelfSegment{(unsigned)sh->rank * (sh->C + 1), sh->C + 1, sh->send_pairs, grad ? sh->send_rows : nullptr};
}

// A shard's segment sizes in bytes, of the (id, count) records and of the rows: one peer's segment, or (whole) the buffer of
// `world` segments.  Every memset and exchange of the whole ops takes its size from here (an exchange that is not wired is
// one device copy of the whole buffer).
struct SegBytes { int64_t pairs, rows; };
static SegBytes shard_bytes(const kv_shard* sh, bool whole) {
  const int64_t rec = (int64_t)(sh->C + 1) * (whole ? sh->world : 1);
  return SegBytes{rec * 16, rec * sh->table->dim * (int64_t)sizeof(float)};
}

// The arguments of a shard's route over n ids (d is zeroed) — the index on the entry-list kernels:
// a table-less tile pass (k_ltile<NOTABLE>: entries, mrow, every position's entry number; d.w is ITS view) and k_papply in
// PA_UNIQUE mode (the distinct ids numbered, uniq / ucnt written, every entry learns its id's number).  The finish then reads
// position -> entry -> number -> record, the gradient pre-sum is k_tsum + k_papply PA_DEDUP.
static void route_desc(kv_shard* sh, long long n, MultiDesc& d) {
  kv_table* rt = sh->route;
  d.w = ws_view(rt, n);
  choose_partitions(rt, d.w, n);   // (the distinct-id hint of the previous route of this length: k_papply publishes it)
  d.w.zero_counts = sh->ucnt;
  d.w.pos_ent = rt->ws.pos_ent;
  PartArgs& pa = d.a;
  pa = self_part_args(rt, n);   // (det: the route table follows its table's mode and is never in occurrence order)
  pa.out_keys = sh->uniq;
  pa.out_counts = sh->ucnt;
  pa.sparse_unique = 1;   // unique numbers with gaps: no counter to serialise on
  pa.day_lk = pa.day;
  if (!pa.det) {   // the numbered ids go straight to their owners' segments (the deterministic mode keeps the ordered scatter)
    pa.route_world = sh->world; pa.route_rule = sh->rule; pa.route_C = sh->C;
    pa.route_seg = sh->send_pairs; pa.route_slot_of = sh->slot_of; pa.route_overflow = sh->overflow; pa.route_gcount = sh->gcount;
    pa.route_need = sh->need; pa.route_uhint = sh->overflow + 1;   // (the launch's last block writes the headers)
  }
}

// ... of its gradient pre-sum (d is zeroed): the tile sums of the ids repeated inside their tile, then the per-id sums
// straight into the records the ids were sent in (k_papply PA_DEDUP over the route's entries, in the route's partitioning)
static void presum_desc(kv_shard* sh, const float* grad, MultiDesc& d) {
  kv_table* rt = sh->route;
  d.w = ws_view(rt, sh->batch.n());
  if (rt->batch.P()) use_partitions(d.w, rt->batch.P());
  PartArgs& pa = d.a;
  pa = self_part_args(rt, sh->batch.n());
  pa.grad = grad;
  pa.out_sum = sh->send_rows;
  pa.out_map = sh->slot_of;
  pa.epart = d.w.epart;
  pa.day_lk = pa.day;
}

// ... and of its finish, over the rows that came back: position -> entry -> dense unique index -> the record its id was
// sent in (this rank's own records, where they stayed in place, in the send buffer)
static FinishDesc finish_desc(const kv_shard* sh, float* out) {
  const kv_table* rt = sh->route;
  FinishDesc d{};
  d.pos_ent = rt->ws.pos_ent; d.ent_u = rt->ws.ent_b; d.slot_of = sh->slot_of; d.rows = sh->recv_rows; d.out = out;
  d.n = sh->batch.n(); d.rows_self = sh->send_rows;
  d.self_lo = (unsigned)sh->rank * (sh->C + 1); d.self_len = sh->batch.own_segment_stays() ? sh->C + 1 : 0u;
  d.dim = rt->dim;
  return d;
}

// ... and of its COMBINING finish: the same rows, walked segment by segment (k_shard_finish_sparse, kv_route.h)
static FinishSparseDesc finish_sparse_desc(const kv_shard* sh, const void* seg, const float* wts, int64_t nseg, float* out) {
  FinishSparseDesc d{};
  d.f = finish_desc(sh, out);
  d.seg = seg; d.wts = wts; d.nseg = nseg;
  return d;
}

// The segments of the sparse lookups' combining finish, per table of the call.  all: every table is combined (the single
// forms: segment_ids may be null where the batch is empty); else seg[k] == nullptr means table k is finished plainly.
struct SparseArgs {
  const void* const* seg;
  int seg_dtype;
  const float* const* wts;   // may be null, and so may wts[k]
  const int64_t* nseg;
  int combiner;
  bool all;
  bool sparse(int k) const { return all || seg[k] != nullptr; }
  const float* w(int k) const { return wts ? wts[k] : nullptr; }
};

// the argument errors of a combining finish over a batch of n ids (kvhip.h kv_shard_lookup_finish_sparse)
static int sparse_finish_check(const char* what, const void* seg, int seg_dtype, int64_t n, int64_t nseg, int combiner, const float* out) {
  if (nseg < 0 || nseg > (1ll << 31) - 2) return fail(KV_INVALID_ARGUMENT, "%s: bad num_segments", what);
  if (nseg > 0 && (!out || (n > 0 && !seg))) return fail(KV_INVALID_ARGUMENT, "%s: segment ids / output pointer is null", what);
  if (seg_dtype != KV_DT_INT32 && seg_dtype != KV_DT_INT64) return fail(KV_INVALID_ARGUMENT, "%s: segment ids must be int32 or int64", what);
  if (combiner < KV_COMBINER_SUM || combiner > KV_COMBINER_SQRTN)
    return fail(KV_INVALID_ARGUMENT, "%s: combiner must be one of 'mean', 'sqrtn' or 'sum'", what);
  return KV_OK;
}

// the argument errors of a sparse gradient pre-sum over a batch of n ids (kvhip.h kv_shard_apply_route_sparse): with n > 0
// there is a gradient to expand, so there must be segments
static int sparse_presum_check(const char* what, const float* seg_grad, const void* seg, int seg_dtype, int64_t n, int64_t nseg, int combiner) {
  if (n > 0 && (!seg_grad || !seg)) return fail(KV_INVALID_ARGUMENT, "%s: segment gradients / segment ids pointer is null", what);
  if (seg_dtype != KV_DT_INT32 && seg_dtype != KV_DT_INT64) return fail(KV_INVALID_ARGUMENT, "%s: segment ids must be int32 or int64", what);
  if (combiner < KV_COMBINER_SUM || combiner > KV_COMBINER_SQRTN)
    return fail(KV_INVALID_ARGUMENT, "%s: combiner must be one of 'mean', 'sqrtn' or 'sum'", what);
  if (n > 0 && (nseg < 1 || nseg > (1ll << 31) - 2)) return fail(KV_INVALID_ARGUMENT, "%s: bad num_segments", what);
  return KV_OK;
}

// a route with nothing to send — an empty batch, or one that failed or was refused: void headers in the send buffer, so that
// the peers are not left waiting
static int shard_void_route(kv_shard* sh, hipStream_t w) {
  sh->batch.route_voided();
  HIP_TRY(hipMemsetAsync(sh->counts, 0, (size_t)sh->world * 8, w));
  k_seg_headers<<<1, MAXW, 0, w>>>(sh->counts, sh->world, sh->C, sh->send_pairs, sh->need);
  return KV_OK;
}

static const int ONLY = 0;   // the todo list of a one-table call: shards[0]
// the shards' route tables, locked: every route-side phase holds them from its checks to its last launch
static MultiLock route_locks(const kv_shard_t* shards, const int* todo, int m) {
  if (m == 1) return MultiLock(shards[todo[0]]->route);   // (one mutex, nothing allocated)
  std::vector<kv_table*> rts;
  for (int j = 0; j < m; ++j) rts.push_back(shards[todo[j]]->route);
  return MultiLock(std::move(rts));
}

static int shard_fork(kv_shard* sh, hipStream_t s, hipStream_t work) {
  if (s == work) return KV_OK;   // the caller works on the communicator's stream itself: one queue, no hops
  HIP_TRY(hipEventRecord(sh->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(work, sh->ev_fork, 0));
  return KV_OK;
}

static int shard_done(kv_shard* sh, hipStream_t s, hipStream_t work, int join) {
  HIP_TRY(hipEventRecord(sh->ev_done, work));
  if (join && s != work) HIP_TRY(hipStreamWaitEvent(s, sh->ev_done, 0));
  return KV_OK;
}

// Once per (shard, communicator): every rank tells every other its {world, rank, capacity, dim, owner rule}.  The
// exchange has no size negotiation, so ranks that disagree would otherwise hang in RCCL or read each other's padding.
static int shard_verify(kv_shard* sh, kv_comm* comm) {
  if (sh->verified == comm) return KV_OK;
  const int W = sh->world;
  std::vector<long long> mine((size_t)W * 4), theirs((size_t)W * 4, 0);
  for (int p = 0; p < W; ++p) {
    mine[4 * p] = ((long long)W << 32) | (unsigned)sh->rank;
    mine[4 * p + 1] = sh->C; mine[4 * p + 2] = sh->table->dim; mine[4 * p + 3] = sh->rule;
  }
  long long *ds = nullptr, *dr = nullptr;
  HIP_TRY(hipMalloc(&ds, mine.size() * 8));
  if (hipMalloc(&dr, mine.size() * 8) != hipSuccess) { hipFree(ds); return fail(KV_RESOURCE_EXHAUSTED, "kv_shard: out of memory"); }
  int rc = KV_OK;
  do {
    if (hipMemcpy(ds, mine.data(), mine.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(KV_INTERNAL, "kv_shard: copy"); break; }
    if ((rc = kv_comm_all_to_all(comm, ds, dr, wired(comm) ? 32 : 32 * W, comm->stream))) break;
    if (hipStreamSynchronize(comm->stream) != hipSuccess || hipMemcpy(theirs.data(), dr, theirs.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail(KV_INTERNAL, "kv_shard: the first exchange failed");
      break;
    }
    for (int p = 0; p < W && !rc; ++p) {
      if ((theirs[4 * p] >> 32) != W || (int)(theirs[4 * p] & 0xFFFFFFFF) != (wired(comm) ? p : sh->rank))
        rc = fail(KV_FAILED_PRECONDITION, "kv_shard: rank %d of the communicator is not shard %d of a world of %d", p, p, W);
      else if (theirs[4 * p + 1] != (long long)sh->C || theirs[4 * p + 2] != sh->table->dim || theirs[4 * p + 3] != sh->rule)
        rc = fail(KV_FAILED_PRECONDITION, "kv_shard: rank %d was created with peer_capacity %lld, dim %lld, owner rule %lld; this "
                                          "rank with %u, %d, %d — they must be equal on every rank",
                  p, theirs[4 * p + 1], theirs[4 * p + 2], theirs[4 * p + 3], sh->C, sh->table->dim, sh->rule);
    }
  } while (0);
  hipFree(ds); hipFree(dr);
  if (!rc) { sh->verified = comm; sh->ranks_seen = W; }
  return rc;
}

// Lossless mode (kv_shard_set_lossless): before anything is exchanged every rank learns the largest segment ANY rank's
// route wanted (one 4-byte all-reduce per table, one stream synchronisation for all tables) and, when that exceeds the
// capacity, every rank raises its capacity to the same new value — they all computed it from the same number — and
// routes the batch again.  grown[k] != 0: shards[k] must be routed again.  The price is the host round trip per lookup
// that the default mode avoids; nothing is ever dropped.
static int shard_agree_many(const kv_shard_t* shards, int ntab, kv_comm* comm, hipStream_t w, char* grown) {
  bool any = false;
  for (int k = 0; k < ntab; ++k) { grown[k] = 0; any = any || shards[k]->lossless; }
  if (!any) return KV_OK;
  if (comm->comm) {
    if (!rccl()->AllReduce) return fail(KV_UNIMPLEMENTED, "lossless sharding needs ncclAllReduce");
    NCCL_TRY(rccl()->GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (int k = 0; k < ntab && bad == ncclSuccess; ++k)
      if (shards[k]->lossless)
        bad = rccl()->AllReduce(shards[k]->need, shards[k]->need + 1, 1, ncclUint32, ncclMax, comm->comm, w);
    const ncclResult_t e = rccl()->GroupEnd();
    if (bad == ncclSuccess) bad = e;
    if (bad != ncclSuccess) return fail(KV_INTERNAL, "ncclAllReduce failed: %s", nccl_err(bad));
  }
  for (int k = 0; k < ntab; ++k)
    if (shards[k]->lossless)
      HIP_TRY(hipMemcpyAsync(shards[k]->need_host, shards[k]->need + (comm->comm ? 1 : 0), sizeof(unsigned), hipMemcpyDeviceToHost, w));
  HIP_TRY(hipStreamSynchronize(w));
  if (comm->xfn && comm->world > 1) {   // the caller's transport: the maximum over the ranks, table by table
    if (!comm->mfn) return fail(KV_UNIMPLEMENTED, "lossless sharding over a staged communicator needs its max_u32 callback");
    for (int k = 0; k < ntab; ++k)
      if (shards[k]->lossless) {
        uint32_t v = *shards[k]->need_host;
        const int r = comm->mfn(comm->user, &v);
        if (r) return fail(KV_INTERNAL, "the staged agreement failed (callback returned %d)", r);
        *shards[k]->need_host = v;
      }
  }
  for (int k = 0; k < ntab; ++k) {
    kv_shard* sh = shards[k];
    if (!sh->lossless || *sh->need_host <= sh->C) continue;
    if (int rc = shard_grow(sh, *sh->need_host, sh->max_ids)) return rc;
    grown[k] = 1;
  }
  return KV_OK;
}

// Several sharded tables in one step (the 40 embedding tables of a DCN): every table's route phase, then ONE grouped
// exchange carrying all their segments, every table's serve phase, ONE exchange back, every table's finish — two
// exchanges per lookup and one per apply whatever the number of tables.  Same results as the per-table ops.
static int multi_shard_check(const kv_shard_t* shards, int ntab, kv_comm_t comm, const char* what) {
  if (!shards || ntab < 1 || ntab > 4096 || !comm) return fail(KV_INVALID_ARGUMENT, "%s: bad arguments", what);
  for (int k = 0; k < ntab; ++k) {
    if (!shards[k] || shards[k]->world != comm->world || shards[k]->table->device != shards[0]->table->device)
      return fail(KV_INVALID_ARGUMENT, "%s: shard %d / communicator mismatch", what, k);
    for (int j = 0; j < k; ++j)
      if (shards[j] == shards[k]) return fail(KV_INVALID_ARGUMENT, "%s: shard %d is listed twice", what, k);
  }
  return KV_OK;
}

// ---- the route-side phases, each over the tables todo[0..m) --------------------------------------------
// On the shards' private route tables; every check and every buffer that may have to grow comes before the first launch.  m > 1:
// one launch for all tables, their descriptors staged; m == 1: the single-table kernels, the descriptor by value, nothing staged.
// A table joins a batched ROUTE when it has no ordered owner scatter (not the deterministic mode) and its batch is not empty.
static bool shard_batchable(const kv_shard* sh, int64_t n) {
  return !sh->table->deterministic && n > 0 && n <= sh->max_ids;
}

// route: the table-less tile pass (m > 1: grid.y = table), then k_papply in PA_UNIQUE mode — numbering, the owners' segments, each
// table's headers by its own last block.  m == 1 alone: the deterministic mode's ordered owner scatter, an empty batch's void route.
static int route_impl(const char* what, const kv_shard_t* shards, const int* todo, int m, const void* const* ids, const int64_t* n, hipStream_t s) {
  int rc;
  for (int j = 0; j < m; ++j)
    if (const int k = todo[j]; (n[k] > 0 && !ids[k]) || n[k] < 0 || n[k] > shards[k]->max_ids)
      return fail(KV_INVALID_ARGUMENT, "%s: n %lld (max %lld)", what, (long long)n[k], shards[k]->max_ids);
  MultiLock lock = route_locks(shards, todo, m);
  for (int j = 0; j < m; ++j) {
    kv_shard* sh = shards[todo[j]];
    kv_table* rt = sh->route;
    if ((rc = hand_over(rt, s))) return rc;   // the phases of one shard keep their order whatever streams they are given
    rt->deterministic = sh->table->deterministic;   // the route index (tile pass, position order) follows the table's mode
    sh->batch.begin_route(n[todo[j]]);
    if (sh->batch.n() > 0 && ((rc = ensure_workspace(rt, sh->batch.n(), true, s)) || (rc = ensure_pos_ent(rt, sh->batch.n(), s)))) return rc;
  }
  if (m == 1) {
    kv_shard* sh = shards[todo[0]];
    const long long n0 = sh->batch.n();
    if (n0 == 0) {   // an empty batch: void headers
      if ((rc = shard_void_route(sh, s))) return rc;
      sh->batch.routed_empty();
      return KV_OK;
    }
    MultiDesc d{};
    route_desc(sh, n0, d);
    launch_ltile_notable(sh->route, d.a.tv, d.w, ids[todo[0]], n0, s);
    WsDev wd = d.w;
    wd.zero_counts = nullptr; wd.pos_ent = nullptr;   // (the tile pass alone files those)
    if ((rc = launch_papply_ud(wd, d.a, PA_UNIQUE, s))) return fail(rc, "route: no kernel for dim %d", d.a.tv.dim);
    sh->batch.route_published(sh->route->batch.publish(++g_serial, n0, BatchIndex::ENTRIES, d.w.P));
    if (d.a.det) {   // the ordered owner scatter
      const unsigned ntr = (unsigned)((n0 + RT - 1) / RT);
      k_owner_hist_u32<<<ntr, TB, 0, s>>>(sh->uniq, sh->ucnt, n0, sh->world, sh->rule, ntr, sh->hist);
      k_owner_scan<<<1, 1024, 0, s>>>(sh->hist, ntr * sh->world, ntr, sh->world, sh->counts);
      k_seg_headers<<<1, MAXW, 0, s>>>(sh->counts, sh->world, sh->C, sh->send_pairs, sh->need);
      k_owner_scatter_fixed<<<ntr, TB, 0, s>>>(sh->uniq, sh->ucnt, n0, sh->world, sh->rule, ntr, sh->hist, sh->C, sh->send_pairs, sh->slot_of, sh->overflow);
    }
  } else {
    Staged<MultiDesc> hd(shards[todo[0]]->table->device, 1, m);
    if (hd.rc) return hd.rc;
    WsDev wmax{};
    for (int j = 0; j < m; ++j) {
      kv_shard* sh = shards[todo[j]];
      route_desc(sh, sh->batch.n(), hd[j]);
      hd[j].ids = ids[todo[j]]; hd[j].n = sh->batch.n();
      widen(wmax, hd[j].w);
    }
    const MultiDesc* md;
    if ((rc = hd.upload(s, &md))) return rc;
    launch_ltile_multi_notable(wmax, m, md, s);
    // (PA_UNIQUE never reaches the code that depends on the row geometry: one variant serves every dim)
    PartArgs p0 = hd[0].a;
    p0.tv.dim = 4;
    if ((rc = launch_papply_ud(wmax, p0, PA_UNIQUE, s, md, m))) return fail(rc, "route: no kernel for dim %d", hd[0].a.tv.dim);
    for (int j = 0; j < m; ++j)
      shards[todo[j]]->batch.route_published(shards[todo[j]]->route->batch.publish(++g_serial, hd[j].n, BatchIndex::ENTRIES, hd[j].w.P));
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// finish, out[i] = the row that came back for ids[i]: tables of one row geometry (row_lanes(dim)), no empty batch.  1 launch
static int finish_impl(const char* what, const kv_shard_t* shards, const int* todo, int m, float* const* outs, hipStream_t s) {
  int rc;
  MultiLock lock = route_locks(shards, todo, m);
  long long nmax = 0;
  for (int j = 0; j < m; ++j) {
    kv_shard* sh = shards[todo[j]];
    if (!sh->batch.route_holds_ids(sh->route->batch)) return fail(KV_FAILED_PRECONDITION, "%s: finish without kv_shard_lookup_route", what);
    if (!outs[todo[j]]) return fail(KV_INVALID_ARGUMENT, "%s: output pointer is null", what);
    if ((rc = hand_over(sh->route, s))) return rc;
    nmax = std::max(nmax, sh->batch.n());
  }
  const unsigned gx = (unsigned)nblocks(nmax, TB, 8192);
  const int q = row_lanes(shards[todo[0]]->table->dim);
  if (m == 1) {
    const FinishDesc d = finish_desc(shards[todo[0]], outs[todo[0]]);
    with_lanes(q, [&](auto vq) {
      k_shard_finish<decltype(vq)::value><<<gx, TB, 0, s>>>(d.pos_ent, d.ent_u, d.slot_of, d.rows, d.out, d.n, d.dim, d.rows_self, d.self_lo, d.self_len);
    });
  } else {
    Staged<FinishDesc> hd(shards[todo[0]]->table->device, 1, m);
    if (hd.rc) return hd.rc;
    for (int j = 0; j < m; ++j) hd[j] = finish_desc(shards[todo[j]], outs[todo[j]]);
    const FinishDesc* md;
    if ((rc = hd.upload(s, &md))) return rc;
    with_lanes(q, [&](auto vq) { k_shard_finish_multi<decltype(vq)::value><<<dim3(gx, (unsigned)m), TB, 0, s>>>(md); });
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// the COMBINING finish of the tables todo[0..m) — all of one row geometry (row_lanes(dim)), their arguments checked
// (sparse_finish_check): 1 launch.  One table takes its descriptor by value: nothing is staged, nothing allocated.
static int finish_sparse_impl(const char* what, const kv_shard_t* shards, const int* todo, int m, const SparseArgs& sp,
                              float* const* outs, hipStream_t s) {
  int rc;
  MultiLock lock = route_locks(shards, todo, m);
  const int q = row_lanes(shards[todo[0]]->table->dim);
  std::vector<FinishSparseDesc> ds(m);
  long long work = 0;   // lanes of the table with the most of them
  for (int j = 0; j < m; ++j) {
    const int k = todo[j];
    kv_shard* sh = shards[k];
    if (!sh->batch.route_holds(sh->route->batch)) return fail(KV_FAILED_PRECONDITION, "%s: finish without kv_shard_lookup_route", what);
    if ((rc = hand_over(sh->route, s))) return rc;
    ds[j] = finish_sparse_desc(sh, sp.seg[k], sp.w(k), sp.nseg[k], outs[k]);
    work = std::max<long long>(work, sp.nseg[k] * q);
  }
  if (work == 0) return KV_OK;
  const int seg32 = sp.seg_dtype == KV_DT_INT32, combiner = sp.combiner;
  const unsigned gx = (unsigned)nblocks(work, TB, 8192);
  if (m == 1) {
    const FinishSparseDesc d = ds[0];
    with_lanes(q, [&](auto vq) { k_shard_finish_sparse<decltype(vq)::value><<<gx, TB, 0, s>>>(d, seg32, combiner); });
  } else {
    Staged<FinishSparseDesc> hd(shards[todo[0]]->table->device, 1, m);
    if (hd.rc) return hd.rc;
    for (int j = 0; j < m; ++j) hd[j] = ds[j];
    const FinishSparseDesc* md;
    if ((rc = hd.upload(s, &md))) return rc;
    const dim3 grid(gx, (unsigned)m);
    with_lanes(q, [&](auto vq) { k_shard_finish_sparse_multi<decltype(vq)::value><<<grid, TB, 0, s>>>(md, seg32, combiner); });
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// The owner's READ-ONLY serve of the tables todo[0..m) — all of one row geometry (row_lanes(dim)): 1 launch
// (k_shard_serve_zeros, kv_route.h).  The tables are entered as kv_batch_gather_or_zeros enters them: behind their last op on
// whatever stream, a pending lookup pass settled, the deferred error reported, as vars they keep their mirrors; no serial bump,
// no workspace, no batch index — the shard's serve token is void, and its last served batch is marked read-only whatever
// happens below (its route has overwritten the route index of the batch before it: shard_refuse_apply).
static int serve_zeros_impl(const kv_shard_t* shards, const int* todo, int m, hipStream_t s) {
  int rc;
  std::vector<kv_table*> tbs;
  unsigned gx = 1;
  for (int j = 0; j < m; ++j) {
    kv_shard* sh = shards[todo[j]];
    sh->batch.served_read_only();
    tbs.push_back(sh->table);
  }
  for (int j = 0; j < m; ++j)
    if ((rc = require_initialized(shards[todo[j]]->table))) return rc;   // FindOrZeros -> CheckInitializedInternal (kv_variable.h:242)
  MultiLock lock(tbs);
  for (kv_table* tb : lock.ts)
    if ((rc = enter_op(tb, s, KEEP_VAR, true, false))) return rc;
  Staged<ServeZerosDesc> hd(shards[todo[0]]->table->device, 0, m);
  if (hd.rc) return hd.rc;
  for (int j = 0; j < m; ++j) {
    const kv_shard* sh = shards[todo[j]];
    ServeZerosDesc& d = hd[j];
    d.t = dev_view(sh->table);
    d.pairs = sh->recv_pairs; d.pairs_self = sh->send_pairs; d.rows = sh->send_rows;
    d.C = sh->C; d.world = sh->world;
    d.self_seg = sh->batch.own_segment_stays() ? sh->rank : -1;
    // one 64-record step per wave were every segment full (the waves past the live records leave at once)
    gx = std::max(gx, (unsigned)nblocks((long long)sh->world * sh->C, TB, 8192));
  }
  const ServeZerosDesc* md;
  if ((rc = hd.upload(s, &md))) return rc;
  const dim3 grid(gx, (unsigned)m);
  with_lanes(row_lanes(shards[todo[0]]->table->dim), [&](auto vq) { k_shard_serve_zeros<decltype(vq)::value><<<grid, TB, 0, s>>>(md); });
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// A read-only lookup's route overwrote the route index of the batch before it: a training apply behind it would pre-sum its
// gradients into the wrong records.  Refused before anything is queued — every rank made the same calls, so every rank
// refuses alike and no peer is left waiting in a grouped recv.
static int shard_refuse_apply(const kv_shard* sh, const char* what) {
  if (sh->batch.may_apply()) return KV_OK;
  return fail(KV_FAILED_PRECONDITION, "%s: the shard's last served batch was a read-only lookup (kv_shard_lookup_zeros / "
                                      "kv_shard_lookup_serve_zeros), which leaves nothing to apply — nothing was queued; run the "
                                      "training lookup of the batch first", what);
}

// gradient pre-sum (tables of one dim, no empty batch; m > 1: none in deterministic mode): the tile sums, then k_papply PA_DEDUP
static int presum_impl(const char* what, const kv_shard_t* shards, const int* todo, int m, const float* const* grads, hipStream_t s) {
  int rc;
  MultiLock lock = route_locks(shards, todo, m);
  for (int j = 0; j < m; ++j) {
    kv_shard* sh = shards[todo[j]];
    if (!sh->batch.route_holds_ids(sh->route->batch)) return fail(KV_FAILED_PRECONDITION, "%s: the batch's lookup must come first (kv_shard_lookup_route)", what);
    if (!grads[todo[j]]) return fail(KV_INVALID_ARGUMENT, "%s: grad pointer is null", what);
    if ((rc = hand_over(sh->route, s))) return rc;
    if ((rc = ensure_workspace(sh->route, sh->batch.n(), true, s))) return rc;
  }
  if (m == 1) {
    MultiDesc d{};
    presum_desc(shards[todo[0]], grads[todo[0]], d);
    if ((rc = launch_tsum(d.a.tv, d.w, d.a.grad, s))) return fail(rc, "tile sums: no kernel for dim %d", d.a.tv.dim);
    if ((rc = launch_papply_ud(d.w, d.a, PA_DEDUP, s))) return fail(rc, "gradient pre-sum: no kernel for dim %d", d.a.tv.dim);
  } else {
    Staged<MultiDesc> hd(shards[todo[0]]->table->device, 1, m);
    if (hd.rc) return hd.rc;
    WsDev wmax{};
    for (int j = 0; j < m; ++j) {
      presum_desc(shards[todo[j]], grads[todo[j]], hd[j]);
      hd[j].a.det = 0; hd[j].n = hd[j].a.n;
      widen(wmax, hd[j].w);
    }
    const MultiDesc* md;
    if ((rc = hd.upload(s, &md))) return rc;
    if ((rc = launch_tsum(hd[0].a.tv, wmax, nullptr, s, md, m))) return fail(rc, "tile sums: no kernel for dim %d", hd[0].a.tv.dim);
    if ((rc = launch_papply_ud(wmax, hd[0].a, PA_DEDUP, s, md, m))) return fail(rc, "gradient pre-sum: no kernel for dim %d", hd[0].a.tv.dim);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// The SPARSE gradient pre-sum of the tables todo[0..m) — all of one dim, and where m > 1 none in deterministic mode: grads[k]
// holds table k's SEGMENT gradients [nseg, dim].  The position records first (launch_pos_records: every position's clamped
// segment and scale, kv_lookup_sparse_grad's own), then the two launches of the plain pre-sum in their per-segment forms
// (kv_sums_seg.hip): the [n, dim] values are neither written nor read.  Every check and every buffer that may have to grow
// comes before the first launch.  One table takes its arguments by value: nothing is staged.
static int presum_sparse_impl(const char* what, const kv_shard_t* shards, const int* todo, int m, const float* const* grads,
                              const SparseArgs& sp, hipStream_t s) {
  int rc;
  MultiLock lock = route_locks(shards, todo, m);
  for (int j = 0; j < m; ++j) {
    const int k = todo[j];
    kv_shard* sh = shards[k];
    if (!sh->batch.route_holds_ids(sh->route->batch))
      return fail(KV_FAILED_PRECONDITION, "%s: the batch's lookup must come first (kv_shard_lookup_route)", what);
    if ((rc = sparse_presum_check(what, grads[k], sp.seg[k], sp.seg_dtype, sh->batch.n(), sp.nseg[k], sp.combiner))) return rc;
  }
  std::vector<SegDesc> sd(m);
  for (int j = 0; j < m; ++j) {
    const int k = todo[j];
    kv_shard* sh = shards[k];
    kv_table* rt = sh->route;
    const bool need_den = sp.w(k) != nullptr && sp.combiner != KV_COMBINER_SUM;
    if ((rc = hand_over(rt, s))) return rc;
    if ((rc = ensure_workspace(rt, sh->batch.n(), true, s)) || (rc = ensure_seg(rt, sp.nseg[k], need_den, s)) ||
        (rc = ensure_pos_records(rt, sh->batch.n(), s)))
      return rc;
    SegDesc& q = sd[j];
    q.seg = sp.seg[k]; q.wts = sp.w(k); q.off = rt->ws.seg_off; q.den = need_den ? rt->ws.seg_den : nullptr;
    q.pseg = rt->ws.pseg; q.pscale = rt->ws.pscale; q.n = sh->batch.n(); q.nseg = sp.nseg[k];
    q.src = SegSrc{grads[k], rt->ws.pseg, rt->ws.pscale};
  }
  const int seg32 = sp.seg_dtype == KV_DT_INT32;
  if (m == 1) {
    MultiDesc d{};
    presum_desc(shards[todo[0]], nullptr, d);
    if ((rc = launch_pos_records(1, sd.data(), nullptr, seg32, sp.combiner, s))) return rc;
    if ((rc = launch_tsum_seg(d.a.tv, d.w, sd[0].src, s))) return fail(rc, "tile sums: no kernel for dim %d", d.a.tv.dim);
    if ((rc = launch_papply_dedup_seg(d.w, d.a, sd[0].src, s))) return fail(rc, "gradient pre-sum: no kernel for dim %d", d.a.tv.dim);
    HIP_TRY(hipGetLastError());
    return KV_OK;
  }
  const int device = shards[todo[0]]->table->device;
  Staged<MultiDesc> hd(device, 1, m);
  if (hd.rc) return hd.rc;
  Staged<SegDesc> hs(device, 2, m);
  if (hs.rc) return hs.rc;
  WsDev wmax{};
  for (int j = 0; j < m; ++j) {
    presum_desc(shards[todo[j]], nullptr, hd[j]);
    hd[j].a.det = 0;
    hd[j].n = hd[j].a.n;
    widen(wmax, hd[j].w);
    hs[j] = sd[j];
  }
  const MultiDesc* md;
  const SegDesc* sdev;
  if ((rc = hd.upload(s, &md)) || (rc = hs.upload(s, &sdev))) return rc;
  if ((rc = launch_pos_records(m, sd.data(), sdev, seg32, sp.combiner, s))) return rc;
  if ((rc = launch_tsum_seg(hd[0].a.tv, wmax, SegSrc{}, s, md, sdev, m))) return fail(rc, "tile sums: no kernel for dim %d", hd[0].a.tv.dim);
  if ((rc = launch_papply_dedup_seg(wmax, hd[0].a, SegSrc{}, s, md, sdev, m))) return fail(rc, "gradient pre-sum: no kernel for dim %d", hd[0].a.tv.dim);
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

// ---- the whole ops: kv_shard_lookup / kv_shard_apply are kv_multi_shard_lookup / kv_multi_shard_apply of one table -----------
// A failure of THIS rank's phase (out of memory, a bad argument) must not leave the peers waiting in a grouped recv: the
// exchanges are queued all the same — void headers for a failed route, zero rows for a failed serve or pre-sum — and the
// first error is returned once everything is queued.  Only a failed exchange or agreement returns at once.
struct FirstError {
  int code = KV_OK;
  std::string msg;
  int operator()(int r) { if (r && !code) { code = r; msg = kv_last_error(); } return r; }
};

static int shard_zero_rows(kv_shard* sh, hipStream_t w) {
  HIP_TRY(hipMemsetAsync(sh->send_rows, 0, (size_t)shard_bytes(sh, true).rows, w));
  return KV_OK;
}

// one grouped exchange for all tables: their (id, count) segments, or (rows) their row segments
static int shards_exchange(const kv_shard_t* shards, int ntab, kv_comm* comm, bool rows, hipStream_t w) {
  std::vector<Seg> seg(ntab);
  for (int k = 0; k < ntab; ++k) {
    const kv_shard* sh = shards[k];
    const SegBytes b = shard_bytes(sh, !wired(comm));
    const bool stay = sh->batch.own_segment_stays();
    seg[k] = rows ? Seg{sh->send_rows, sh->recv_rows, b.rows, stay} : Seg{sh->send_pairs, sh->recv_pairs, b.pairs, stay};
  }
  return comm_exchange(comm, ntab, seg.data(), w);
}

// The tables [0, ntab) that take part in a batched launch, split by key(k) (negative: table k takes no part): the groups of at
// least two tables, in ascending key order, each in table order.  The callers launch those and then, in table order, the
// tables left over one by one.
template <class Key>
static std::vector<std::vector<int>> groups_of(int ntab, Key key) {
  std::vector<std::vector<int>> out;
  if (ntab < 2) return out;
  std::vector<std::pair<int, int>> kk;
  for (int k = 0; k < ntab; ++k) {
    const int q = key(k);
    if (q >= 0) kk.emplace_back(q, k);
  }
  std::sort(kk.begin(), kk.end());
  for (size_t i = 0, j; i < kk.size(); i = j) {
    for (j = i + 1; j < kk.size() && kk[j].first == kk[i].first;) ++j;
    if (j - i < 2) continue;
    out.emplace_back();
    for (size_t e = i; e < j; ++e) out.back().push_back(kk[e].second);
  }
  return out;
}

// the owner side of a table can join a batched lookup / apply over the receive buffers
static bool shard_owner_batchable(const kv_shard* sh) {
  return sh->table->key_dtype == KV_DT_INT64 && shard_nrec(sh) <= (1ll << 21);
}

// Forked from `s` onto the communicator's stream (the caller's stream is free for the dense tower; phases and exchanges in
// one queue: no event hop between a kernel and its exchange): verify, route, lossless agreement and the re-route of grown
// tables, exchange, serve, exchange, finish.  single: kv_shard_lookup — the phase events of kv_shard_profile are its alone.
// read_only: kv_shard_lookup_zeros / kv_multi_shard_lookup_zeros — the same op but for the serve (serve_zeros_impl, one launch
// per row geometry: the owners' tables are read, never written) and the profile, which does not sample it.
// sp: the sparse lookups — the same op but for the finish of the tables sp->sparse(k), which combines the rows into segments
// (finish_sparse_impl, one launch per row geometry; sampled as `finish`).  A table whose sparse arguments are wrong is
// treated as one whose route failed: void headers, both exchanges, its output untouched, the error at the end.
static int shards_lookup(const char* what, bool single, bool read_only, const kv_shard_t* shards, int ntab, kv_comm* comm, const void* const* ids,
                         const int64_t* n, float* const* outs, int join, hipStream_t s, const SparseArgs* sp = nullptr) {
  int rc;
  DeviceGuard dg(shards[0]->table->device);
  hipStream_t w = comm->stream;
  // The lossless mode's agreement reads a device word on the host: one stream synchronisation, not allowed inside a stream
  // capture.  Refused HERE, before the communicator's stream is forked into the capture and before anything is queued (a
  // refusal behind the fork would leave the side stream unjoined and invalidate the caller's capture).
  bool lossless = false;
  for (int k = 0; k < ntab; ++k) lossless = lossless || shards[k]->lossless;
  if (lossless && (stream_is_capturing(s) || stream_is_capturing(w)))
    return fail(KV_FAILED_PRECONDITION, "%s under stream capture: the lossless mode (the default) synchronises once per lookup; "
                                        "capture sharded steps with kv_shard_set_lossless(shard, 0)%s",
                what, single ? " and a peer_capacity sized for the workload" : "");
  for (int k = 0; k < ntab; ++k)
    if ((rc = shard_verify(shards[k], comm))) return rc;
  std::vector<unsigned> seen(ntab);
  for (int k = 0; k < ntab; ++k) seen[k] = shard_take_flag(shards[k]);
  kv_shard* const sh0 = shards[0];
  if ((rc = shard_fork(sh0, s, w))) return rc;
  FirstError note;
  std::vector<char> routed(ntab, 1), done(ntab, 0);
  auto sparse = [&](int k) { return sp && sp->sparse(k); };
  for (int k = 0; k < ntab; ++k)
    if (sparse(k) && note(sparse_finish_check(what, sp->seg[k], sp->seg_dtype, n[k], sp->nseg[k], sp->combiner, outs[k]))) routed[k] = 0;
  for (int k = 0; k < ntab; ++k) shards[k]->batch.exchanged_by_library(shard_can_stay(shards[k]));
  const bool pm = single && !read_only && shard_prof_begin(sh0, true);
  shard_prof_mark(sh0, pm, 0, w);
  auto route = [&](const int* todo, int m) {   // false: refused or failed — void headers are due, the peers are not left waiting
    const bool ok = routed[todo[0]] && !note(route_impl(what, shards, todo, m, ids, n, w));
    for (int j = 0; j < m; ++j) routed[todo[j]] = ok;
    return ok;
  };
  // the tables whose route is the entry-list one go together: 2 launches for all of them; then the others, one by one
  for (const auto& grp : groups_of(ntab, [&](int k) { return routed[k] && shard_batchable(shards[k], n[k]) ? 0 : -1; }))
    if (route(grp.data(), (int)grp.size()))
      for (int k : grp) done[k] = 1;
  for (int k = 0; k < ntab; ++k)
    if (!done[k] && !route(&k, 1) && (rc = shard_void_route(shards[k], w))) return rc;
  {   // lossless tables: one agreement for all of them (every rank takes part, whatever its own route did), then the grown
      // ones are routed again — or, where this rank's batch was refused, get void headers in the new buffers too
    std::vector<char> grown(ntab, 0);
    if ((rc = shard_agree_many(shards, ntab, comm, w, grown.data()))) return rc;
    for (int k = 0; k < ntab; ++k)
      if (grown[k]) {
        shards[k]->batch.exchanged_by_library(shard_can_stay(shards[k]));   // (the record count changed)
        if (!route(&k, 1) && (rc = shard_void_route(shards[k], w))) return rc;
      }
  }
  shard_prof_mark(sh0, pm, 1, w);
  if ((rc = shards_exchange(shards, ntab, comm, false, w))) return rc;
  shard_prof_mark(sh0, pm, 2, w);
  // the owners' lookups: the tables of one dim in one batched lookup over their receive buffers (tile pass of all of them
  // in one launch; the partition passes stay pending for the batched apply)
  done.assign(ntab, 0);
  if (read_only) {   // the read-only serve instead: the tables of one row geometry in one launch, then the tables left over, one launch each
    auto serve = [&](const int* todo, int m) -> int {
      if (note(serve_zeros_impl(shards, todo, m, w)))
        for (int j = 0; j < m; ++j)
          if ((rc = shard_zero_rows(shards[todo[j]], w))) return rc;
      for (int j = 0; j < m; ++j) done[todo[j]] = 1;
      return KV_OK;
    };
    for (const auto& grp : groups_of(ntab, [&](int k) { return row_lanes(shards[k]->table->dim); }))
      if ((rc = serve(grp.data(), (int)grp.size()))) return rc;
    for (int k = 0; k < ntab; ++k)
      if (!done[k] && (rc = serve(&k, 1))) return rc;
  }
  for (const auto& grp : groups_of(ntab, [&](int k) { return !read_only && shard_owner_batchable(shards[k]) ? shards[k]->table->dim : -1; })) {
    const int m = (int)grp.size();
    std::vector<kv_handle_t> tb(m);
    std::vector<const void*> ip(m);
    std::vector<int64_t> nn(m);
    std::vector<float*> op(m);
    std::vector<kv_batch_token_t> tok(m, 0);
    std::vector<unsigned> caps(m);
    std::vector<SelfSegment> selfs(m);
    for (int j = 0; j < m; ++j) {
      kv_shard* sh = shards[grp[j]];
      tb[j] = sh->table; ip[j] = sh->recv_pairs; nn[j] = shard_nrec(sh); op[j] = sh->send_rows; caps[j] = sh->C + 1;
      sh->batch.serve_begins();
      selfs[j] = shard_self(sh, false);
    }
    if (note(multi_lookup_impl(m, tb.data(), ip.data(), nullptr, nn.data(), op.data(), tok.data(), w, 2, caps.data(), selfs.data()))) {
      for (int k : grp)
        if ((rc = shard_zero_rows(shards[k], w))) return rc;
    } else {
      for (int j = 0; j < m; ++j) shards[grp[j]]->batch.served(tok[j]);
    }
    for (int k : grp) done[k] = 1;
  }
  for (int k = 0; k < ntab; ++k)
    if (!done[k] && note(kv_shard_lookup_serve(shards[k], w)) && (rc = shard_zero_rows(shards[k], w))) return rc;
  shard_prof_mark(sh0, pm, 3, w);
  if ((rc = shards_exchange(shards, ntab, comm, true, w))) return rc;
  shard_prof_mark(sh0, pm, 4, w);
  // finish, of every table whose own route succeeded: the tables of one row geometry in one launch — the plain ones, then
  // the combining ones (an empty batch still writes its segments)
  done.assign(ntab, 0);
  auto plain = [&](int k) { return routed[k] && !sparse(k) && shards[k]->batch.n() > 0; };
  for (const auto& grp : groups_of(ntab, [&](int k) { return plain(k) ? row_lanes(shards[k]->table->dim) : -1; }))
    if (!note(finish_impl(what, shards, grp.data(), (int)grp.size(), outs, w)))
      for (int k : grp) done[k] = 1;
  for (int k = 0; k < ntab; ++k)
    if (plain(k) && !done[k]) note(finish_impl(what, shards, &k, 1, outs, w));
  for (const auto& grp : groups_of(ntab, [&](int k) { return routed[k] && sparse(k) && sp->nseg[k] > 0 ? row_lanes(shards[k]->table->dim) : -1; })) {
    note(finish_sparse_impl(what, shards, grp.data(), (int)grp.size(), *sp, outs, w));
    for (int k : grp) done[k] = 1;
  }
  for (int k = 0; k < ntab; ++k)
    if (routed[k] && !done[k] && sparse(k) && sp->nseg[k] > 0) note(finish_sparse_impl(what, shards, &k, 1, *sp, outs, w));
  shard_prof_mark(sh0, pm, 5, w);
  if (pm) sh0->pend_l = true;
  if ((rc = shard_done(sh0, s, w, join))) return rc;
  if (note.code) return fail(note.code, "%s (this rank's exchanges were queued all the same)", note.msg.c_str());
  for (int k = 0; k < ntab; ++k)
    if ((rc = shard_late_report(shards[k], seen[k]))) return rc;
  return KV_OK;
}

// backward, as shards_lookup: the gradient pre-sum, ONE exchange, the owners' applies.  A rank whose pre-sum failed still
// takes part in the exchange (zero gradient rows).  slot1 may be null (no table has a second slot table).
// sp != nullptr (the sparse applies): grads[k] of a table with segments holds its SEGMENT gradients, and its pre-sum is the
// sparse one (presum_sparse_impl) — in groups of its own, by dim; the exchange and the owners' side know no difference.
static int shards_apply(const char* what, bool single, const kv_shard_t* shards, int ntab, kv_comm* comm, int optimizer,
                        const kv_handle_t* slot0, const kv_handle_t* slot1, const float* const* grads, const float* hp, int join,
                        hipStream_t s, const SparseArgs* sp = nullptr) {
  int rc;
  DeviceGuard dg(shards[0]->table->device);
  hipStream_t w = comm->stream;
  kv_shard* const sh0 = shards[0];
  auto sparse = [&](int k) { return sp != nullptr && sp->sparse(k); };
  for (int k = 0; k < ntab; ++k)
    if ((rc = shard_refuse_apply(shards[k], what))) return rc;
  if ((rc = shard_fork(sh0, s, w))) return rc;
  FirstError note;
  const bool pm = single && shard_prof_begin(sh0, false);
  shard_prof_mark(sh0, pm, 6, w);
  // gradient pre-sum: the tables of one dim whose route has no ordered owner scatter in two launches
  std::vector<char> done(ntab, 0);   // 1: summed; 2: its group failed (zero gradient rows)
  auto presum = [&](const int* todo, int m) {   // (a group is all sparse or all plain)
    return sparse(todo[0]) ? presum_sparse_impl(what, shards, todo, m, grads, *sp, w) : presum_impl(what, shards, todo, m, grads, w);
  };
  for (const auto& grp : groups_of(ntab, [&](int k) {
         return shards[k]->batch.n() > 0 && !shards[k]->table->deterministic ? shards[k]->table->dim * 2 + (sparse(k) ? 1 : 0) : -1; })) {
    const char r = note(presum(grp.data(), (int)grp.size())) ? 2 : 1;
    for (int k : grp) done[k] = r;
  }
  for (int k = 0; k < ntab; ++k)   // the others one by one (an empty batch has nothing to sum)
    if (done[k] != 1 && (done[k] == 2 || (shards[k]->batch.n() > 0 && note(presum(&k, 1)))) && (rc = shard_zero_rows(shards[k], w))) return rc;
  shard_prof_mark(sh0, pm, 7, w);
  if ((rc = shards_exchange(shards, ntab, comm, true, w))) return rc;
  shard_prof_mark(sh0, pm, 8, w);
  // the owners' applies: the tables of one dim whose serve lookups left their batch index in one batched apply
  done.assign(ntab, 0);
  for (const auto& grp : groups_of(ntab, [&](int k) {
         const kv_shard* sh = shards[k];
         const BatchIndex::Plan served = sh->table->batch.plan(sh->batch.serve_token(), shard_nrec(sh), fused_tab(sh->table));
         return optimizer >= 0 && optimizer <= OPT_ADAM && shard_owner_batchable(sh) && BatchIndex::takes_entries(served) && slot0[k] != nullptr &&
                        (!two_slots(optimizer) || (slot1 && slot1[k]))
                    ? sh->table->dim : -1; })) {
    const int m = (int)grp.size();
    std::vector<kv_handle_t> vs(m), s0(m), s1(m);
    std::vector<const float*> gp(m);
    std::vector<const void*> ip(m);
    std::vector<int64_t> nn(m);
    std::vector<kv_batch_token_t> tok(m);
    std::vector<SelfSegment> selfs(m);
    for (int j = 0; j < m; ++j) {
      kv_shard* sh = shards[grp[j]];
      vs[j] = sh->table; s0[j] = slot0[grp[j]]; s1[j] = slot1 ? slot1[grp[j]] : nullptr;
      gp[j] = sh->recv_rows; ip[j] = sh->recv_pairs; nn[j] = shard_nrec(sh); tok[j] = sh->batch.serve_token();
      selfs[j] = shard_self(sh, true);
    }
    // (require_reuse: the ids are (id, count) records — an apply that rebuilt its index from them would read them as plain ids)
    note(multi_apply(shard_opt_call(optimizer, hp), m, vs.data(), s0.data(), s1.data(), gp.data(), ip.data(), nn.data(), tok.data(), w,
                     false, true, selfs.data()));
    for (int k : grp) done[k] = 1;
  }
  for (int k = 0; k < ntab; ++k)
    if (!done[k]) note(kv_shard_apply_serve(shards[k], optimizer, slot0[k], slot1 ? slot1[k] : nullptr, hp, w));
  shard_prof_mark(sh0, pm, 9, w);
  if (pm) sh0->pend_a = true;
  if ((rc = shard_done(sh0, s, w, join))) return rc;
  if (note.code) return fail(note.code, "%s (this rank's exchange was queued all the same)", note.msg.c_str());
  return KV_OK;
}

// the sparse whole ops: shards_lookup with the combining finish
static int shard_lookup_sparse(const char* what, bool read_only, kv_shard_t sh, kv_comm_t comm, const void* ids, const void* segment_ids,
                               int segment_dtype, const float* weights, int64_t n, int64_t num_segments, int combiner, float* out, int join,
                               kv_stream_t stream) {
  if (!sh || !comm || comm->world != sh->world) return fail(KV_INVALID_ARGUMENT, "%s: shard / communicator mismatch", what);
  const SparseArgs sp{&segment_ids, segment_dtype, &weights, &num_segments, combiner, true};
  return shards_lookup(what, true, read_only, &sh, 1, comm, &ids, &n, &out, join, (hipStream_t)stream, &sp);
}

static int multi_shard_lookup_sparse(const char* what, bool read_only, const kv_shard_t* shards, int ntab, kv_comm_t comm,
                                     const void* const* ids, const void* const* segment_ids, int segment_dtype,
                                     const float* const* weights, const int64_t* n, const int64_t* num_segments, int combiner,
                                     float* const* outs, int join, kv_stream_t stream) {
  int rc;
  if ((rc = multi_shard_check(shards, ntab, comm, what))) return rc;
  if (!ids || !segment_ids || !n || !num_segments || !outs) return fail(KV_INVALID_ARGUMENT, "%s: null argument list", what);
  const SparseArgs sp{segment_ids, segment_dtype, weights, num_segments, combiner, false};
  return shards_lookup(what, false, read_only, shards, ntab, comm, ids, n, outs, join, (hipStream_t)stream, &sp);
}

}  // namespace

extern "C" {

int kv_bucket_by_owner(kv_handle_t t, const void* ids, int64_t n, const int64_t* n_dev, int world, int owner_rule, int64_t* out_ids,
                       int32_t* perm, int64_t* counts_dev, const int32_t* id_counts, int64_t* pairs_out,
                       int32_t* pos_out, kv_stream_t stream) {
  int rc;
  if ((rc = check_table(t))) return rc;
  if (world < 1 || world > MAXW) return fail(KV_INVALID_ARGUMENT, "world %d: 1..%d ranks", world, MAXW);
  if (owner_rule != KV_OWNER_HASH && owner_rule != KV_OWNER_MOD) return fail(KV_INVALID_ARGUMENT, "owner_rule %d", owner_rule);
  if (n < 0 || n > (1ll << 31) - 1 || (n > 0 && (!ids || !out_ids || !perm)) || !counts_dev)
    return fail(KV_INVALID_ARGUMENT, "bad arguments");
  DeviceGuard dg(t->device);
  std::lock_guard<std::mutex> l(t->mu);
  hipStream_t s = (hipStream_t)stream;
  const unsigned ntiles = (unsigned)((n + RT - 1) / RT);
  const size_t need = (size_t)std::max(1u, ntiles) * world;
  if (t->route_hist_cap < need) {
    HIP_TRY(hipStreamSynchronize(s));
    hipFree(t->route_hist);
    HIP_TRY(hipMalloc(&t->route_hist, need * sizeof(unsigned)));
    t->route_hist_cap = need;
  }
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)world * sizeof(long long), s));
    return KV_OK;
  }
  if (t->key_dtype == KV_DT_INT32) {
    k_owner_hist<int><<<ntiles, TB, 0, s>>>((const int*)ids, n, world, owner_rule, ntiles, t->route_hist, (const long long*)n_dev);
    k_owner_scan<<<1, 1024, 0, s>>>(t->route_hist, ntiles * world, ntiles, world, (long long*)counts_dev);
    k_owner_scatter<int><<<ntiles, TB, 0, s>>>((const int*)ids, n, world, owner_rule, ntiles, t->route_hist, (long long*)out_ids, perm,
                                               (const long long*)n_dev, id_counts, (long long*)pairs_out, pos_out);
  } else {
    k_owner_hist<long long><<<ntiles, TB, 0, s>>>((const long long*)ids, n, world, owner_rule, ntiles, t->route_hist,
                                                  (const long long*)n_dev);
    k_owner_scan<<<1, 1024, 0, s>>>(t->route_hist, ntiles * world, ntiles, world, (long long*)counts_dev);
    k_owner_scatter<long long><<<ntiles, TB, 0, s>>>((const long long*)ids, n, world, owner_rule, ntiles, t->route_hist,
                                                     (long long*)out_ids, perm, (const long long*)n_dev, id_counts,
                                                     (long long*)pairs_out, pos_out);
  }
  HIP_TRY(hipGetLastError());
  return KV_OK;
}

int kv_comm_unique_id(void* id128) {
  if (!id128) return fail(KV_INVALID_ARGUMENT, "id128 is null");
  if (!rccl()->ok) return fail(KV_UNIMPLEMENTED, "librccl.so.1 could not be loaded");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId");
  NCCL_TRY(rccl()->GetUniqueId(reinterpret_cast<ncclUniqueId*>(id128)));
  return KV_OK;
}

int kv_comm_create(int world, int rank, const void* id128, int device, kv_comm_t* out) {
  if (!out || world < 1 || world > MAXW || rank < 0 || rank >= world) return fail(KV_INVALID_ARGUMENT, "kv_comm_create: world %d rank %d", world, rank);
  DeviceGuard dg(device);
  kv_comm* c = new kv_comm();
  int rc = KV_OK;
  do {
    if (!comm_init(c, world, rank, device)) { rc = fail(KV_INTERNAL, "kv_comm_create: stream / events"); break; }
    if (world > 1 || id128) {   // a world of one needs no RCCL (the exchange is a device copy) unless asked for
      if (!id128) { rc = fail(KV_INVALID_ARGUMENT, "kv_comm_create: unique id is null"); break; }
      if (!rccl()->ok) { rc = fail(KV_UNIMPLEMENTED, "librccl.so.1 could not be loaded"); break; }
      ncclUniqueId id;
      std::memcpy(&id, id128, sizeof id);
      ncclResult_t r = rccl()->CommInitRank(&c->comm, world, id, rank);
      if (r != ncclSuccess) { rc = fail(KV_INTERNAL, "ncclCommInitRank: %s", nccl_err(r)); break; }
    }
  } while (0);
  if (rc) { kv_comm_destroy(c); return rc; }
  *out = c;
  return KV_OK;
}

int kv_comm_create_staged(int world, int rank, kv_comm_exchange_fn exchange, kv_comm_max_fn max_u32, void* user, int device,
                          kv_comm_t* out) {
  if (!out || !exchange || world < 1 || world > MAXW || rank < 0 || rank >= world)
    return fail(KV_INVALID_ARGUMENT, "kv_comm_create_staged: world %d rank %d", world, rank);
  DeviceGuard dg(device);
  kv_comm* c = new kv_comm();
  c->xfn = exchange; c->mfn = max_u32; c->user = user;
  if (!comm_init(c, world, rank, device)) { kv_comm_destroy(c); return fail(KV_INTERNAL, "kv_comm_create_staged: stream / events"); }
  *out = c;
  return KV_OK;
}

int kv_comm_set_self_via_rccl(kv_comm_t c, int on) {
  if (!c || !c->comm) return fail(KV_INVALID_ARGUMENT, "kv_comm_set_self_via_rccl: not an RCCL communicator");
  c->self_via_rccl = on != 0;
  return KV_OK;
}

int kv_comm_stream(kv_comm_t c, kv_stream_t* stream) {
  if (!c || !stream) return fail(KV_INVALID_ARGUMENT, "kv_comm_stream: null argument");
  *stream = (kv_stream_t)c->stream;
  return KV_OK;
}

int kv_forget_stream(kv_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hipStreamSynchronize(s) != hipSuccess) return fail(KV_INVALID_ARGUMENT, "kv_forget_stream: the stream cannot be synchronised");
  retire_stream(s);
  return KV_OK;
}

int kv_comm_destroy(kv_comm_t c) {
  if (!c) return KV_OK;
  DeviceGuard dg(c->device);
  if (c->stream) { hipStreamSynchronize(c->stream); retire_stream(c->stream); }   // no table keeps the stream as its last one
  if (c->comm && rccl()->ok) rccl()->CommDestroy(c->comm);
  if (c->ev_in) hipEventDestroy(c->ev_in);
  if (c->ev_out) hipEventDestroy(c->ev_out);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return KV_OK;
}

int kv_comm_all_to_all(kv_comm_t c, const void* send, void* recv, int64_t bytes_per_peer, kv_stream_t stream) {
  if (!c || !send || !recv || bytes_per_peer < 0) return fail(KV_INVALID_ARGUMENT, "kv_comm_all_to_all: bad arguments");
  DeviceGuard dg(c->device);
  const Seg all{send, recv, bytes_per_peer, false};
  return comm_exchange(c, 1, &all, (hipStream_t)stream);
}

int kv_shard_create(kv_handle_t local_table, int world, int rank, int owner_rule, int64_t max_ids, int64_t peer_capacity,
                    kv_shard_t* out) {
  int rc;
  if ((rc = check_table(local_table))) return rc;
  if (!out || world < 1 || world > MAXW || rank < 0 || rank >= world) return fail(KV_INVALID_ARGUMENT, "kv_shard_create: world %d rank %d", world, rank);
  if (owner_rule != KV_OWNER_HASH && owner_rule != KV_OWNER_MOD) return fail(KV_INVALID_ARGUMENT, "owner_rule %d", owner_rule);
  if (max_ids < 1 || max_ids > (1ll << 21)) return fail(KV_INVALID_ARGUMENT, "max_ids %lld: 1 .. 2^21 ids per sharded batch", (long long)max_ids);
  if (local_table->key_dtype == KV_DT_INT32) return fail(KV_UNIMPLEMENTED, "sharded tables carry int64 ids");
  if (!fused_ok(local_table->dim))   // (the route, the finish and the owners' serve side exist on the entry-list kernels alone)
    return fail(KV_UNIMPLEMENTED, "sharded tables: dim %d (multiples of 4 up to 256)", local_table->dim);
  if (local_table->occurrence_order)
    return fail(KV_UNIMPLEMENTED, "sharded tables: occurrence-order mode is a single-table notion (senders pre-sum, owners add the senders' sums in rank order)");
  DeviceGuard dg(local_table->device);
  kv_shard* sh = new kv_shard();
  sh->table = local_table; sh->world = world; sh->rank = rank; sh->rule = owner_rule; sh->max_ids = max_ids;
  local_table->shard_refs.fetch_add(1);
  do {
    if ((rc = kv_create(KV_DT_INT64, KV_DT_FLOAT, local_table->dim, 0, 0, local_table->device, &sh->route))) break;
    // default capacity: twice an even share of max_ids distinct ids (hashed ownership spreads them evenly), at least 1024
    long long C = peer_capacity > 0 ? peer_capacity : std::max<long long>(1024, 2 * ((max_ids + world - 1) / world));
    C = std::min<long long>(C, max_ids);
    const unsigned ntr = (unsigned)((max_ids + RT - 1) / RT);
    if (hipMalloc(&sh->uniq, (size_t)max_ids * 8) != hipSuccess || hipMalloc(&sh->ucnt, (size_t)max_ids * 4) != hipSuccess ||
        hipMalloc(&sh->slot_of, (size_t)max_ids * 4) != hipSuccess || hipMalloc(&sh->counts, (size_t)world * 8) != hipSuccess ||
        hipMalloc(&sh->hist, (size_t)ntr * world * 4) != hipSuccess ||
        hipMalloc(&sh->gcount, (MAXW + 1) * 4) != hipSuccess || hipMemset(sh->gcount, 0, (MAXW + 1) * 4) != hipSuccess ||
        hipHostMalloc(&sh->overflow, 2 * sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipMalloc(&sh->need, 2 * sizeof(unsigned)) != hipSuccess || hipMemset(sh->need, 0, 2 * sizeof(unsigned)) != hipSuccess ||
        hipHostMalloc(&sh->need_host, sizeof(unsigned), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&sh->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sh->ev_done, hipEventDisableTiming) != hipSuccess) {
      rc = fail(KV_RESOURCE_EXHAUSTED, "kv_shard_create: allocation failed");
      break;
    }
    sh->overflow[0] = 0; sh->overflow[1] = 0;   // [1]: the last routed batch's distinct ids (k_papply PA_UNIQUE)
    if ((rc = shard_alloc_buffers(sh, (unsigned)C))) break;
  } while (0);
  if (rc) { kv_shard_destroy(sh); return rc; }
  *out = sh;
  return KV_OK;
}

int kv_shard_destroy(kv_shard_t sh) {
  if (!sh) return KV_OK;
  DeviceGuard dg(sh->table->device);
  sh->table->shard_refs.fetch_sub(1);
  hipDeviceSynchronize();
  shard_free_buffers(sh);
  hipFree(sh->uniq); hipFree(sh->ucnt); hipFree(sh->slot_of); hipFree(sh->counts); hipFree(sh->hist); hipFree(sh->gcount);
  if (sh->overflow) hipHostFree(sh->overflow);
  if (sh->need) hipFree(sh->need);
  if (sh->need_host) hipHostFree(sh->need_host);
  if (sh->ev_fork) hipEventDestroy(sh->ev_fork);
  if (sh->ev_done) hipEventDestroy(sh->ev_done);
  for (hipEvent_t e : sh->pev) if (e) hipEventDestroy(e);
  if (sh->route) kv_destroy(sh->route);
  delete sh;
  return KV_OK;
}

int kv_shard_buffers(kv_shard_t sh, void** send_pairs, void** recv_pairs, void** send_rows, void** recv_rows,
                     int64_t* pair_bytes_per_peer, int64_t* row_bytes_per_peer) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  if (send_pairs) *send_pairs = sh->send_pairs;
  if (recv_pairs) *recv_pairs = sh->recv_pairs;
  if (send_rows) *send_rows = sh->send_rows;
  if (recv_rows) *recv_rows = sh->recv_rows;
  if (pair_bytes_per_peer) *pair_bytes_per_peer = shard_bytes(sh, false).pairs;
  if (row_bytes_per_peer) *row_bytes_per_peer = shard_bytes(sh, false).rows;
  return KV_OK;
}

// ids -> local unique ids with counts -> the owners' segments of the send buffer.  2 launches (deterministic mode: 6), no host sync.
int kv_shard_lookup_route(kv_shard_t sh, const void* ids, int64_t n, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "kv_shard_lookup_route: n %lld (max %lld)", (long long)n, 0ll);
  const unsigned seen = shard_take_flag(sh);
  sh->batch.exchanged_by_caller();   // all segments, this rank's own included, arrive in the receive buffers
  DeviceGuard dg(sh->table->device);
  if (int rc = route_impl("kv_shard_lookup_route", &sh, &ONLY, 1, &ids, &n, (hipStream_t)stream)) return rc;
  return shard_late_report(sh, seen);
}

// the owner's half: the ids the peers sent (recv_pairs) are looked up in this rank's table — frequency words count
// every occurrence — and their rows go to send_rows, record for record.  3 launches.
int kv_shard_lookup_serve(kv_shard_t sh, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  sh->batch.serve_begins();
  const SelfSegment self = shard_self(sh, false);
  kv_batch_token_t token = 0;   // (stays 0 where the lookup publishes nothing)
  const int rc = gather_or_insert_impl(sh->table, sh->recv_pairs, nullptr, shard_nrec(sh), sh->send_rows, stream, 1, &token, sh->C + 1, &self);
  sh->batch.served(token);
  return rc;
}

// the owner's half of a READ-ONLY lookup: the rows of the ids the peers sent as kv_gather_or_zeros reads them (zeros for a
// key the table does not hold, a blacklisted one, one under the enter threshold) to send_rows, record for record; the table
// is not changed in any way.  1 launch.
int kv_shard_lookup_serve_zeros(kv_shard_t sh, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  DeviceGuard dg(sh->table->device);
  return serve_zeros_impl(&sh, &ONLY, 1, (hipStream_t)stream);
}

// out[i] = the row that came back for ids[i].  1 launch.
int kv_shard_lookup_finish(kv_shard_t sh, float* out, kv_stream_t stream) {
  if (!sh || (sh->batch.n() > 0 && !out)) return fail(KV_INVALID_ARGUMENT, "kv_shard_lookup_finish: output pointer is null");
  if (sh->batch.n() == 0) return KV_OK;
  DeviceGuard dg(sh->table->device);
  return finish_impl("kv_shard_lookup_finish", &sh, &ONLY, 1, &out, (hipStream_t)stream);
}

// out[s] = the combiner over segment s of w_j * (the row that came back for ids[j]), in position order.  1 launch; an empty
// batch still writes its segments.
int kv_shard_lookup_finish_sparse(kv_shard_t sh, const void* segment_ids, int segment_dtype, const float* weights,
                                  int64_t num_segments, int combiner, float* out, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "kv_shard_lookup_finish_sparse: null shard");
  int rc;
  if ((rc = sparse_finish_check("kv_shard_lookup_finish_sparse", segment_ids, segment_dtype, sh->batch.n(), num_segments, combiner, out)))
    return rc;
  DeviceGuard dg(sh->table->device);
  const SparseArgs sp{&segment_ids, segment_dtype, &weights, &num_segments, combiner, true};
  return finish_sparse_impl("kv_shard_lookup_finish_sparse", &sh, &ONLY, 1, sp, &out, (hipStream_t)stream);
}

// backward: the gradient rows of the batch just looked up are summed per distinct id straight into the records their
// ids were sent in (the route index is still there: no ids, no sizes, no sync).  2 launches.
int kv_shard_apply_route(kv_shard_t sh, const float* grad, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_route: null shard");
  // (the refusal first: n is the read-only batch's, and a rank whose voided training batch was empty has no gradient to name)
  { int rc; if ((rc = shard_refuse_apply(sh, "kv_shard_apply_route"))) return rc; }
  if (sh->batch.n() > 0 && !grad) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_route: grad pointer is null");
  if (sh->batch.n() == 0) return KV_OK;
  DeviceGuard dg(sh->table->device);
  return presum_impl("kv_shard_apply_route", &sh, &ONLY, 1, &grad, (hipStream_t)stream);
}

// ... from the SEGMENT gradients of the batch's sparse lookup: the record of a distinct id receives the sum over its
// positions j of scale_j * seg_grad[segment of j] — each term the row kv_lookup_sparse_grad would have written, added in the
// order kv_shard_apply_route adds rows; the [n, dim] values never exist.  3 launches for the position records (2 without
// weighted denominators), then the 2 of the pre-sum.
int kv_shard_apply_route_sparse(kv_shard_t sh, const float* seg_grad, const void* segment_ids, int segment_dtype,
                                const float* weights, int64_t num_segments, int combiner, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_route_sparse: null shard");
  { int rc; if ((rc = shard_refuse_apply(sh, "kv_shard_apply_route_sparse"))) return rc; }
  if (sh->batch.n() == 0) return KV_OK;
  DeviceGuard dg(sh->table->device);
  const SparseArgs sp{&segment_ids, segment_dtype, &weights, &num_segments, combiner, true};
  return presum_sparse_impl("kv_shard_apply_route_sparse", &sh, &ONLY, 1, &seg_grad, sp, (hipStream_t)stream);
}

// the owner's half: recv_rows holds the peers' summed gradients, record for record as the lookup served them; the
// fused apply takes the index that lookup left in the table's workspace.  2 launches.  optimizer / hp: shard_opt_call
int kv_shard_apply_serve(kv_shard_t sh, int optimizer, kv_handle_t slot0, kv_handle_t slot1, const float* hp, kv_stream_t stream) {
  if (!sh || !hp) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_serve: bad arguments");
  const int64_t nrec = shard_nrec(sh);
  if (!sh->table->batch.holds(sh->batch.serve_token(), nrec))
    return fail(KV_FAILED_PRECONDITION, "kv_shard_apply_serve: another op used the table since this batch's lookup "
                                        "(the sharded apply takes over the lookup's index)");
  const SelfSegment self = shard_self(sh, true);
  const OptCall c = shard_opt_call(optimizer, hp);
  if (c.opt < 0) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_serve: optimizer %d", optimizer);
  return apply_one(c, sh->table, slot0, slot1, sh->recv_rows, sh->recv_pairs, nrec, sh->batch.serve_token(), stream, false, &self);
}

// whole ops: forked from `stream` onto the shard's own stream (the caller's stream is free for the dense tower);
// join != 0 makes `stream` wait for the result right away, else kv_shard_join does when the caller needs it
int kv_shard_join(kv_shard_t sh, kv_stream_t stream) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  DeviceGuard dg(sh->table->device);
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, sh->ev_done, 0));
  return KV_OK;
}

int kv_shard_profile(kv_shard_t sh, int every) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  DeviceGuard dg(sh->table->device);
  shard_prof_collect(sh, true); shard_prof_collect(sh, false);
  sh->prof_every = every > 0 ? every : 0;
  sh->prof_seq_l = sh->prof_seq_a = 0;
  for (int i = 0; i < KV_SHARD_PHASES; ++i) { sh->psum[i] = 0.0; sh->pcnt[i] = 0; }
  return KV_OK;
}

int kv_shard_profile_read(kv_shard_t sh, double* ms_sum, int64_t* samples, int n_phases, int64_t* info) {
  if (!sh || !ms_sum || !samples || n_phases < KV_SHARD_PHASES) return fail(KV_INVALID_ARGUMENT, "kv_shard_profile_read: bad arguments");
  DeviceGuard dg(sh->table->device);
  shard_prof_collect(sh, true); shard_prof_collect(sh, false);
  for (int i = 0; i < KV_SHARD_PHASES; ++i) { ms_sum[i] = sh->psum[i]; samples[i] = sh->pcnt[i]; }
  if (info) { info[0] = sh->ranks_seen; info[1] = (int64_t)sh->C; info[2] = (int64_t)sh->grows; info[3] = (int64_t)sh->overflows; }
  return KV_OK;
}

int kv_shard_set_lossless(kv_shard_t sh, int on) {
  if (!sh) return fail(KV_INVALID_ARGUMENT, "null shard");
  sh->lossless = on != 0;
  return KV_OK;
}

// the same agreement between shards that live in ONE process (see kv_shard_exchange_local): call it after every
// shard's kv_shard_lookup_route; *rerouted != 0 means the capacity was raised on all of them and the routes must run again
int kv_shard_agree_local(const kv_shard_t* shards, int world, int* rerouted, kv_stream_t stream) {
  if (!shards || world < 1 || !rerouted) return fail(KV_INVALID_ARGUMENT, "kv_shard_agree_local: bad arguments");
  *rerouted = 0;
  for (int p = 0; p < world; ++p)
    if (!shards[p] || shards[p]->world != world || shards[p]->C != shards[0]->C)
      return fail(KV_INVALID_ARGUMENT, "kv_shard_agree_local: shards differ in world / capacity");
  DeviceGuard dg(shards[0]->table->device);
  hipStream_t s = (hipStream_t)stream;
  unsigned need = 0;
  for (int p = 0; p < world; ++p)
    HIP_TRY(hipMemcpyAsync(shards[p]->need_host, shards[p]->need, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int p = 0; p < world; ++p) need = std::max(need, *shards[p]->need_host);
  if (need <= shards[0]->C) return KV_OK;
  for (int p = 0; p < world; ++p)
    if (int rc = shard_grow(shards[p], need, shards[0]->max_ids)) return rc;   // (one capacity for all of them)
  *rerouted = 1;
  return KV_OK;
}

int kv_shard_lookup(kv_shard_t sh, kv_comm_t comm, const void* ids, int64_t n, float* out, int join, kv_stream_t stream) {
  if (!sh || !comm || comm->world != sh->world) return fail(KV_INVALID_ARGUMENT, "kv_shard_lookup: shard / communicator mismatch");
  return shards_lookup("kv_shard_lookup", true, false, &sh, 1, comm, &ids, &n, &out, join, (hipStream_t)stream);
}

int kv_shard_lookup_zeros(kv_shard_t sh, kv_comm_t comm, const void* ids, int64_t n, float* out, int join, kv_stream_t stream) {
  if (!sh || !comm || comm->world != sh->world) return fail(KV_INVALID_ARGUMENT, "kv_shard_lookup_zeros: shard / communicator mismatch");
  return shards_lookup("kv_shard_lookup_zeros", true, true, &sh, 1, comm, &ids, &n, &out, join, (hipStream_t)stream);
}

int kv_shard_lookup_sparse(kv_shard_t sh, kv_comm_t comm, const void* ids, const void* segment_ids, int segment_dtype,
                           const float* weights, int64_t n, int64_t num_segments, int combiner, float* out, int join,
                           kv_stream_t stream) {
  return shard_lookup_sparse("kv_shard_lookup_sparse", false, sh, comm, ids, segment_ids, segment_dtype, weights, n, num_segments, combiner,
                             out, join, stream);
}

int kv_shard_lookup_sparse_zeros(kv_shard_t sh, kv_comm_t comm, const void* ids, const void* segment_ids, int segment_dtype,
                                 const float* weights, int64_t n, int64_t num_segments, int combiner, float* out, int join,
                                 kv_stream_t stream) {
  return shard_lookup_sparse("kv_shard_lookup_sparse_zeros", true, sh, comm, ids, segment_ids, segment_dtype, weights, n, num_segments,
                             combiner, out, join, stream);
}

int kv_multi_shard_lookup_sparse(const kv_shard_t* shards, int ntab, kv_comm_t comm, const void* const* ids,
                                 const void* const* segment_ids, int segment_dtype, const float* const* weights,
                                 const int64_t* n, const int64_t* num_segments, int combiner, float* const* outs,
                                 int join, kv_stream_t stream) {
  return multi_shard_lookup_sparse("kv_multi_shard_lookup_sparse", false, shards, ntab, comm, ids, segment_ids, segment_dtype, weights, n,
                                   num_segments, combiner, outs, join, stream);
}

int kv_multi_shard_lookup_sparse_zeros(const kv_shard_t* shards, int ntab, kv_comm_t comm, const void* const* ids,
                                       const void* const* segment_ids, int segment_dtype, const float* const* weights,
                                       const int64_t* n, const int64_t* num_segments, int combiner, float* const* outs,
                                       int join, kv_stream_t stream) {
  return multi_shard_lookup_sparse("kv_multi_shard_lookup_sparse_zeros", true, shards, ntab, comm, ids, segment_ids, segment_dtype, weights,
                                   n, num_segments, combiner, outs, join, stream);
}

int kv_shard_apply(kv_shard_t sh, kv_comm_t comm, int optimizer, kv_handle_t slot0, kv_handle_t slot1, const float* grad,
                   const float* hp, int join, kv_stream_t stream) {
  if (!sh || !comm || comm->world != sh->world) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply: shard / communicator mismatch");
  return shards_apply("kv_shard_apply", true, &sh, 1, comm, optimizer, &slot0, &slot1, &grad, hp, join, (hipStream_t)stream);
}

// kv_shard_apply whose pre-sum takes the SEGMENT gradients of the batch's sparse lookup (kv_shard_apply_route_sparse)
int kv_shard_apply_sparse(kv_shard_t sh, kv_comm_t comm, int optimizer, kv_handle_t slot0, kv_handle_t slot1, const float* seg_grad,
                          const void* segment_ids, int segment_dtype, const float* weights, int64_t num_segments, int combiner,
                          const float* hp, int join, kv_stream_t stream) {
  if (!sh || !comm || comm->world != sh->world) return fail(KV_INVALID_ARGUMENT, "kv_shard_apply_sparse: shard / communicator mismatch");
  const SparseArgs sp{&segment_ids, segment_dtype, &weights, &num_segments, combiner, true};
  return shards_apply("kv_shard_apply_sparse", true, &sh, 1, comm, optimizer, &slot0, &slot1, &seg_grad, hp, join, (hipStream_t)stream,
                      &sp);
}

int kv_multi_shard_lookup(const kv_shard_t* shards, int ntab, kv_comm_t comm, const void* const* ids, const int64_t* n,
                          float* const* outs, int join, kv_stream_t stream) {
  int rc;
  if ((rc = multi_shard_check(shards, ntab, comm, "kv_multi_shard_lookup"))) return rc;
  if (!ids || !n || !outs) return fail(KV_INVALID_ARGUMENT, "kv_multi_shard_lookup: null argument list");
  return shards_lookup("kv_multi_shard_lookup", false, false, shards, ntab, comm, ids, n, outs, join, (hipStream_t)stream);
}

int kv_multi_shard_lookup_zeros(const kv_shard_t* shards, int ntab, kv_comm_t comm, const void* const* ids, const int64_t* n,
                                float* const* outs, int join, kv_stream_t stream) {
  int rc;
  if ((rc = multi_shard_check(shards, ntab, comm, "kv_multi_shard_lookup_zeros"))) return rc;
  if (!ids || !n || !outs) return fail(KV_INVALID_ARGUMENT, "kv_multi_shard_lookup_zeros: null argument list");
  return shards_lookup("kv_multi_shard_lookup_zeros", false, true, shards, ntab, comm, ids, n, outs, join, (hipStream_t)stream);
}

// slot0 / slot1: one handle per table (slot1 only for the FTRL family, else nullptr); hp as in kv_shard_apply_serve
int kv_multi_shard_apply(const kv_shard_t* shards, int ntab, kv_comm_t comm, int optimizer, const kv_handle_t* slot0,
                         const kv_handle_t* slot1, const float* const* grads, const float* hp, int join, kv_stream_t stream) {
  int rc;
  if ((rc = multi_shard_check(shards, ntab, comm, "kv_multi_shard_apply"))) return rc;
  if (!slot0 || !grads || !hp) return fail(KV_INVALID_ARGUMENT, "kv_multi_shard_apply: null argument list");
  return shards_apply("kv_multi_shard_apply", false, shards, ntab, comm, optimizer, slot0, slot1, grads, hp, join, (hipStream_t)stream);
}

// kv_multi_shard_apply where grads[k] of a table with segment_ids[k] != nullptr holds its SEGMENT gradients
// [num_segments[k], dim_k] (the mixed form of kv_multi_shard_lookup_sparse); one exchange whatever the mix
int kv_multi_shard_apply_sparse(const kv_shard_t* shards, int ntab, kv_comm_t comm, int optimizer, const kv_handle_t* slot0,
                                const kv_handle_t* slot1, const float* const* grads, const void* const* segment_ids,
                                int segment_dtype, const float* const* weights, const int64_t* num_segments, int combiner,
                                const float* hp, int join, kv_stream_t stream) {
  int rc;
  if ((rc = multi_shard_check(shards, ntab, comm, "kv_multi_shard_apply_sparse"))) return rc;
  if (!slot0 || !grads || !hp || !segment_ids || !num_segments)
    return fail(KV_INVALID_ARGUMENT, "kv_multi_shard_apply_sparse: null argument list");
  const SparseArgs sp{segment_ids, segment_dtype, weights, num_segments, combiner, false};
  return shards_apply("kv_multi_shard_apply_sparse", false, shards, ntab, comm, optimizer, slot0, slot1, grads, hp, join,
                      (hipStream_t)stream, &sp);
}

// The exchange between shards that live in ONE process (all on one device): segment r of shard p's send buffer to
// segment p of shard r's receive buffer.  what: 0 = the (id, count) records, 1 = the rows.  This is how the
// phases are exercised with several ranks on a single GPU (RCCL refuses two ranks on one device).
int kv_shard_exchange_local(const kv_shard_t* shards, int world, int what, kv_stream_t stream) {
  if (!shards || world < 1) return fail(KV_INVALID_ARGUMENT, "kv_shard_exchange_local: bad arguments");
  for (int p = 0; p < world; ++p)
    if (!shards[p] || shards[p]->world != world || shards[p]->C != shards[0]->C || shards[p]->table->dim != shards[0]->table->dim)
      return fail(KV_INVALID_ARGUMENT, "kv_shard_exchange_local: shards differ in world / capacity / dim");
  DeviceGuard dg(shards[0]->table->device);
  const size_t rec = shards[0]->C + 1;
  const size_t bytes = rec * (what == 0 ? 16 : (size_t)shards[0]->table->dim * sizeof(float));
  for (int p = 0; p < world; ++p)
    for (int r = 0; r < world; ++r) {
      const char* src = what == 0 ? (const char*)shards[p]->send_pairs : (const char*)shards[p]->send_rows;
      char* dst = what == 0 ? (char*)shards[r]->recv_pairs : (char*)shards[r]->recv_rows;
      HIP_TRY(hipMemcpyAsync(dst + (size_t)p * bytes, src + (size_t)r * bytes, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
  return KV_OK;
}

}  // extern "C"
