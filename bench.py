#!/usr/bin/env python3
"""bench.py — KvVariable hot path on MI355X: embedding_lookup (GatherOrInsert) + fused sparse
GroupAdam-V4 apply over one batch of int64 ids, BASELINE.json config 2:
  50M-key KvVariable x dim 32, 1M ids/batch Zipf(1.2), fp32.

One "step" = one lookup of the batch + one fused apply of the batch's gradients (dedup +
segment-sum + row update).  Inputs (ids, grads) are resident in HBM before the timed region.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
                                                            (N > 1: launched by torch.distributed.run)

Prints ONE JSON line on rank 0: the headline (`metric`, `value`, `unit`, `ms_per_step`, ...) of the K
timed steps.  A plain run does only that: set-up, W warm-up steps, K timed steps.  `--full` adds
everything else, measured after the timed region: `roofline` for the dominant kernel (HIP events on
the op's own stream, kv_profile_*), the per-kernel table, the sub-records of `extras` and
`cpu_baseline` (the CPU oracle — a port of the reference algorithm — timed on this host on a
bounded sample).  `--dump-outputs DIR` writes what the last timed step computed (dump_outputs).
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEED = 20250211 + 2
SAMPLE_EVERY = int(os.environ.get("KV_BENCH_SAMPLE_EVERY", "0"))   # 0: the dominant kernel is bracketed by events on every 8th step of the timed region (a pair of markers costs ~4 us of stream time), every 5th / 2nd when the run has 64 / 24 steps or fewer (so that at least 8 launches are timed)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)


def splitmix64(x):
  """int64 tensor -> int64 tensor; keys = splitmix64(rank) spreads ranks over the int64 space."""
  def c(v):  # two's-complement constant
    return v - (1 << 64) if v >= (1 << 63) else v
  x = x + c(0x9E3779B97F4A7C15)
  # logical shifts on int64: mask off the sign-extended bits
  def lsr(v, s):
    return (v >> s) & ((1 << (64 - s)) - 1)
  x = (x ^ lsr(x, 30)) * c(0xBF58476D1CE4E5B9)
  x = (x ^ lsr(x, 27)) * c(0x94D049BB133111EB)
  return x ^ lsr(x, 31)


class Zipf(object):
  """Exact inverse-CDF Zipf(s) over ranks 1..K: tabulated head + Euler-Maclaurin tail."""

  def __init__(self, K, s, device, head=1 << 20):
    self.K, self.s = K, s
    M = min(head, K)
    self.M = M
    w = torch.arange(1, M + 1, dtype=torch.float64, device=device)**(-s)
    self.cdf = torch.cumsum(w, 0)
    self.head_mass = float(self.cdf[-1])
    a = 1.0 - s
    self.tail = lambda x: (x**a) / a  # antiderivative of x^-s
    self.tail_mass = float(self.tail(K + 0.5) - self.tail(M + 0.5)) if K > M else 0.0
    self.total = self.head_mass + self.tail_mass

  def sample(self, n, gen):
    u = torch.rand(n, dtype=torch.float64, device=self.cdf.device, generator=gen) * self.total
    r = torch.searchsorted(self.cdf, u.clamp(max=self.head_mass * (1 - 1e-15))) + 1
    if self.K > self.M:
      a = 1.0 - self.s
      t = (u - self.head_mass).clamp(min=0) + (self.M + 0.5)**a / a
      rt = torch.clamp(torch.round((t * a)**(1.0 / a)), self.M + 1, self.K).to(torch.int64)
      r = torch.where(u >= self.head_mass, rt, r)
    return r.to(torch.int64)


def cpu_baseline(args, D):
  """The oracle (a port of the reference's CPU algorithm: 1031-segment unordered_map, per-row heap buffers, rw spin
  locks, Shard-style contiguous blocks) on this host's cores, BASELINE.md section 3's protocol on a bounded sample:
  a table with --cpu-keys keys (configs[1]'s 50 M by default; the UNTIMED build fills it one hash segment per thread,
  --cpu-build-budget seconds at most: a host too slow for that times the baseline on the keys it got in, and says how
  many), warm-up steps, then
  --cpu-steps timed steps of the same 1 M-id Zipf batch shape; median and p95.  The lookup and the optimizer apply
  are sharded over the cores like the reference's ops; TF-core's Unique / UnsortedSegmentSum run on ONE thread, as
  they do in TF-core."""
  from oracle import kv_oracle as ko
  cores = os.cpu_count() or 1
  K = args.cpu_keys
  rng = np.random.default_rng(SEED)
  table = (rng.standard_normal((10000, D)) * 0.05).astype(np.float32)
  var = ko.OracleKv(D, 0, table, day=20000, picker=1, seed=1, threads=cores)
  slot = ko.OracleKv(3 * D, 0, np.zeros((16, 3 * D), np.float32), day=20000, picker=1, seed=1, threads=cores)
  z = Zipf(K, args.zipf, torch.device("cpu"))
  g = torch.Generator().manual_seed(SEED)
  # UNTIMED set-up: the 50 M-key table is filled by oracle.bulk_build (one thread per hash segment, no lock traffic) — the
  # state the ordinary lookup would leave, reached ~20 x faster (217 s of a 264 s run went into this build in round 4).
  # The timed steps below run the ordinary restated functions (gather_or_insert, dedup, apply) on it.
  t0 = time.perf_counter()
  built = 0
  CHB = 1 << 23
  for i in range(0, K, CHB):
    var.bulk_build(splitmix64(torch.arange(i + 1, min(i + CHB, K) + 1, dtype=torch.int64)).numpy())
    built = min(i + CHB, K)
    if time.perf_counter() - t0 > args.cpu_build_budget and built < K:
      break
  build_s = time.perf_counter() - t0
  if built < K:      # the Zipf ranks are drawn over the keys that exist
    K = built
    z = Zipf(K, args.zipf, torch.device("cpu"))
  N = args.batch

  def one_step(ph=None):
    ids = splitmix64(z.sample(N, g)).numpy()
    grad = rng.normal(0, 1e-2, (N, D)).astype(np.float32)
    t0 = time.perf_counter()
    var.gather_or_insert(ids)
    t1 = time.perf_counter()
    u, s, _ = ko.dedup_segment_sum(ids, grad)          # TF-core unique + unsorted_segment_sum (1 thread)
    t2 = time.perf_counter()
    ko.apply_group_adam(var, slot, s, u, 1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8)
    t3 = time.perf_counter()
    if ph is not None:
      ph.append((t1 - t0, t2 - t1, t3 - t2))
    return t3 - t0
  for _ in range(2):                                    # warm-up: the first steps insert the slot rows
    one_step()
  # the thread count that serves this workload best (on a 256-thread host all threads were 1.35 x one
  # thread): one warm + two timed steps per candidate, the timed steps below run at the best one.  The Zipf head puts a
  # fifth of the batch on ONE hash segment's spin lock and the dedup is one thread by construction (TF-core's Unique), so
  # more threads stop paying early.
  cand = sorted({c for c in (1, 2, 4, 8, 16, 32, 64, cores) if c <= cores})
  sweep = {}
  for c in cand:
    var.threads = slot.threads = c
    one_step()
    sweep[c] = min(one_step() for _ in range(2))
  best = min(sweep, key=lambda c: sweep[c])
  var.threads = slot.threads = best
  ph = []
  times = [one_step(ph) for _ in range(args.cpu_steps)]
  t, p95 = float(np.median(times)), float(np.percentile(times, 95))
  phases = {k: float(np.median([p[i] for p in ph])) for i, k in enumerate(("lookup", "dedup_1_thread", "apply"))}
  return {"value": N / t, "unit": "ids/s", "cores": best, "kind": "port", "value_1_thread": N / sweep[1],
          "host_cores": cores, "threads_sweep_ids_per_s": {str(c): N / v for c, v in sweep.items()},
          "median_s_per_step": t, "p95_s_per_step": p95, "phases_s": phases,
          "phases_what": "median seconds per step at `cores` threads: lookup (GatherOrInsert, sharded over the threads like the "
                         "reference's Shard()), dedup_1_thread (TF-core Unique + UnsortedSegmentSum: one thread whatever the "
                         "host), apply (GroupAdamV4, sharded); the dedup's share is why threads stop paying",
          "keys": K, "keys_asked": args.cpu_keys,
          "sample": "oracle/kv_oracle.cc, %d threads (the best of %s on this %d-core host; dedup on 1 like TF-core's Unique), "
                    "%d-key table, 2 warm-up + %d timed steps of %d Zipf(%.1f) ids: lookup + tf.unique/segment_sum + "
                    "GroupAdamV4; median %.3f s / p95 %.3f s per step; table build %.1f s"
                    % (best, cand, cores, K, args.cpu_steps, N, args.zipf, t, p95, build_s)}


def extras(args, ops, L, _lib, var, slot, dev, pool, out, K, N, D, gen, state):
  """Measurements next to the headline, all outside the timed region: what an unchanged TF graph would run (the op
  boundary: unique ids + pre-summed gradients; the apply without the lookup's token; every tensor staged through
  pinned host memory like the CPU-device shim does) and the step at other skews."""
  def st():
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

  def adam(ids_t, grad_t, n, tok):
    _lib.check(L.kv_apply_group_adam_tok(var.ptr, slot.ptr, grad_t.data_ptr(), ids_t.data_ptr(), n, 1e-3,
                                         float(state["b1p"]), float(state["b2p"]), 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 4, tok, st()))

  def lookup(ids_t, want_token):
    tok = ctypes.c_uint64(0)
    _lib.check(L.kv_gather_or_insert_tok(var.ptr, ids_t.data_ptr(), None, ids_t.numel(), out.data_ptr(),
                                         ctypes.byref(tok) if want_token else None, st()))
    return tok.value

  def timed(fn, steps=30, warm=5):   # (12 steps of a 45 us op are 0.5 ms: one host hiccup moved the record by 12 %)
    for k in range(warm):
      fn(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
      fn(warm + k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3

  res = {}
  # ---- the op boundary (training_ops.cc:7011-7021: what the optimizer op receives from TF-core in an unchanged graph):
  #      unique ids and their summed gradient rows, no token.  SURVEY 8(d): U * (8 + 4D + 16 + 2 * 4 * 4D) bytes.
  #      kv_apply_group_adam_unique (kvhip.h): one launch, the caller's promise of unique ids guarded on the device
  uni = []
  for ids, grad in [p[:2] for p in pool[:4]]:
    u, inv = torch.unique(ids, return_inverse=True)
    sm = torch.zeros((u.numel(), D), dtype=torch.float32, device=dev).index_add_(0, inv, grad)
    uni.append((u.contiguous(), sm))

  def adam_unique(ids_t, grad_t, n):
    _lib.check(L.kv_apply_group_adam_unique(var.ptr, slot.ptr, grad_t.data_ptr(), ids_t.data_ptr(), n, 1e-3,
                                            float(state["b1p"]), float(state["b2p"]), 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 4, st()))
  ms = timed(lambda k: adam_unique(uni[k % len(uni)][0], uni[k % len(uni)][1], uni[k % len(uni)][0].numel()))
  ms_batch = timed(lambda k: adam(uni[k % len(uni)][0], uni[k % len(uni)][1], uni[k % len(uni)][0].numel(), 0))
  Uu = float(np.mean([u.numel() for u, _ in uni]))
  byt = Uu * (8 + 4 * D + 16 + 2 * 4 * 4 * D)
  res["op_boundary"] = {"what": "kv_apply_group_adam_unique on unique ids + pre-summed gradient rows: ONE launch (k_uapply: probe, "
                                "state read-modify-write, duplicate guard)",
                        "unique_ids": Uu, "ms": ms, "algorithmic_bytes": byt, "GBps": byt / (ms * 1e-3) / 1e9,
                        "frac_of_peak": byt / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "unique_applies_per_s": Uu / (ms * 1e-3),
                        "batch_pipeline_ms": ms_batch,
                        "batch_pipeline_what": "the same input through kv_apply_group_adam (no promise: tile pass + tile sums + k_papply)"}
  del uni
  # ---- lookup + apply of the same batch WITHOUT the token (the apply builds its own index)
  def no_token(k):
    ids, grad = pool[k % len(pool)][:2]
    lookup(ids, False)
    adam(ids, grad, N, 0)
  ms = timed(no_token)
  res["no_token"] = {"what": "lookup + apply of the same 1 M ids, the apply rebuilding the batch index", "ms_per_step": ms,
                     "ids_per_s": N / (ms * 1e-3)}
  # ---- staged: ids / out / grad cross a pinned host ring as in the CPU-device TF shim (PCIe-inclusive; never `value`)
  ids_h = [p[0].cpu().pin_memory() for p in pool[:2]]
  grad_h = [p[1].cpu().pin_memory() for p in pool[:2]]
  out_h = torch.empty((N, D), dtype=torch.float32).pin_memory()
  ids_d = torch.empty(N, dtype=torch.int64, device=dev)
  grad_d = torch.empty((N, D), dtype=torch.float32, device=dev)

  def staged(k):
    ids_d.copy_(ids_h[k % 2], non_blocking=True)
    tok = lookup(ids_d, True)
    out_h.copy_(out, non_blocking=True)
    grad_d.copy_(grad_h[k % 2], non_blocking=True)
    adam(ids_d, grad_d, N, tok)
  ms = timed(staged, steps=6, warm=2)
  pcie = N * (8 + 4 * D) * 2
  res["staged"] = {"what": "the step with ids, output rows and gradients crossing pinned host memory (one stream, no overlap)",
                   "ms_per_step": ms, "pcie_bytes_per_step": pcie, "pcie_GBps": pcie / (ms * 1e-3) / 1e9, "ids_per_s": N / (ms * 1e-3)}
  del ids_h, grad_h, out_h, ids_d, grad_d
  # ---- what an UNCHANGED reference graph runs per step on the GPU kernels: the complete training
  #      lookup (no token: rows + its own bookkeeping pass), then TF-core's de-duplication of the gradient
  #      (variable_scope.py:1096-1106 -> _deduplicate_indexed_slices: Unique + UnsortedSegmentSum; kv_dedup_segment_sum
  #      stands in for those two TF-core ops, it returns the count to the host like TF's Unique fixes its output shape),
  #      then the optimizer op on unique ids + summed rows (training_ops.cc:7011-7021): ONE loop, one number
  def unchanged(k):
    ids, grad = pool[k % len(pool)][:2]
    lookup(ids, False)
    u, sm, _ = ops.kv_dedup_segment_sum(var, ids, grad)
    adam_unique(u, sm, u.numel())
  ms = timed(unchanged)
  # the same three calls timed one by one (each loop alone: the parts do not add up exactly to the loop above)
  ms_l = timed(lambda k: lookup(pool[k % len(pool)][0], False))
  ms_d = timed(lambda k: ops.kv_dedup_segment_sum(var, pool[k % len(pool)][0], pool[k % len(pool)][1]))
  res["unchanged_graph"] = {"what": "per step, no batch token and no processor patch: complete lookup (kv_gather_or_insert) + "
                                    "kv_dedup_segment_sum (in TF-core's Unique + UnsortedSegmentSum's place; synchronous like "
                                    "them) + kv_apply_group_adam_unique",
                            "ms_per_step": ms, "ids_per_s": N / (ms * 1e-3),
                            "parts_ms": {"lookup_complete": ms_l, "dedup_segment_sum": ms_d, "apply_unique": res["op_boundary"]["ms"]},
                            "vs_token_path": "the headline's ms_per_step is the same work with the lookup's batch token"}
  # ---- the sharded path at world 1: the N > 1 ops — route, the three exchanges (empty at world 1:
  #      a rank's own segment stays in place), serve, finish, pre-sum, apply — over the library's communicator on this one
  #      GPU, so that the mechanism's own cost is on the driver's N = 1 line.  Never `value`.
  try:
    comm = ops.KvComm(1, 0, ops.kv_comm_unique_id(), dev.index)
    cap = int(max(p[2] for p in pool) * 1.25) + 1024
    shard = ops.KvShard(var, 1, 0, ops.KV_OWNER_HASH, max_ids=N, peer_capacity=cap)
    shard.set_lossless(False)      # capacity sized from the pool: cannot overflow (as the N > 1 line does)
    cs = comm.stream()
    hp_t = ctypes.c_float * 9
    torch.cuda.synchronize()
    with torch.cuda.stream(cs):
      cst = ctypes.c_void_p(cs.cuda_stream)

      def sharded(k):
        ids, grad = pool[k % len(pool)][:2]
        _lib.check(L.kv_shard_lookup(shard.ptr, comm.ptr, ids.data_ptr(), N, out.data_ptr(), 1, cst))
        hp = hp_t(1e-3, float(state["b1p"]), float(state["b2p"]), 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
        _lib.check(L.kv_shard_apply(shard.ptr, comm.ptr, 0, slot.ptr, None, grad.data_ptr(), hp, 1, cst))
      ms = timed(sharded, steps=16, warm=4)
      shard.profile(1)
      for k in range(12):
        sharded(k)
      torch.cuda.synchronize()
      sp = shard.profile_read()
      shard.profile(0)
    res["sharded_world1"] = {"what": "kv_shard_lookup + kv_shard_apply of the same batches with world = 1 over the RCCL communicator "
                                     "(the N > 1 code path; exchanges carry nothing at world 1)",
                             "ms_per_step": ms, "ids_per_s": N / (ms * 1e-3), "phases_ms": sp["phases_ms"],
                             "phases_sum_ms": sum(v for v in sp["phases_ms"].values() if v),
                             "phases_samples": sp["samples"], "peer_capacity_records": cap,
                             "overflowed_batches": sp["overflows"]}
    torch.cuda.synchronize()
    _lib.check(L.kv_shard_destroy(shard.ptr)); shard.ptr = None
    _lib.check(L.kv_comm_destroy(comm.ptr)); comm.ptr = None
  except Exception as e:   # (a box without a usable RCCL: the headline must still print)
    res["sharded_world1"] = {"error": "%s: %s" % (type(e).__name__, e)}
  # ---- other skews (CTR tables are not all Zipf(1.2)): the same table, 1 M ids per batch.  (LAST: tools/prof_summary.py reads
  #      the last launches of each kernel of a profiled run as the headline's shape, and this sweep ends with Zipf 1.2)
  sweep = []
  for sk in (0.3, 0.8, 1.2):
    z = Zipf(K, sk, dev)
    bs = []
    NB = 6   # as many distinct batches as the headline's pool nearly: two alternating ones would stay warm in the 256 MB MALL
    for _ in range(NB):
      ids = splitmix64(z.sample(N, gen))
      bs.append((ids, torch.randn(N, D, device=dev, generator=gen) * 1e-2, int(torch.unique(ids).numel())))

    def full(k):
      ids, grad, _ = bs[k % NB]
      adam(ids, grad, N, lookup(ids, True))
    ms_step = timed(full, steps=24, warm=4)
    ms_look = timed(lambda k: lookup(bs[k % NB][0], True), steps=24, warm=3)
    # when the lookup's output rows are complete (a token lookup defers its partition pass): the tile kernel alone
    ops.kv_profile_enable(var, 64)
    for k in range(NB):
      full(k)
    torch.cuda.synchronize()
    pr = ops.kv_profile_read(var)
    ops.kv_profile_enable(var, 0)
    rows_ms = (pr["lookup_tile"][0] + pr["lookup_order"][0]) / max(pr["lookup_tile"][1], 1)
    U_sk = float(np.mean([b[2] for b in bs]))
    look_bytes = N * 8 + U_sk * (16 + 4 * D) + N * 4 * D        # ids + probe record and row per distinct id + output rows
    sweep.append({"zipf": sk, "unique_per_batch": U_sk, "ms_per_step": ms_step,
                  "lookup_ms": ms_look, "lookup_rows_ready_ms": rows_ms, "apply_ms": ms_step - ms_look,
                  "lookup_algorithmic_bytes": look_bytes,
                  "lookup_frac": look_bytes / (ms_look * 1e-3) / 1e9 / HBM_PEAK_GBS,
                  "lookup_rows_ready_frac": look_bytes / (rows_ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
    del bs
  res["skew_sweep"] = sweep
  # ---- the headline's own batches in occurrence-order mode (kv_set_deterministic(var, 2): a repeated id's gradient rows
  #      added one by one in input order, TF-core's unsorted_segment_sum chain — the reference's CPU bits).
  #      After the sweep: the mode takes the sorted-position kernels, so the entry-list kernels' last launches in a trace of
  #      this run stay the sweep's.
  try:
    ops.kv_set_deterministic(var, 2)

    def occ(k):
      ids, grad = pool[k % len(pool)][:2]
      adam(ids, grad, N, lookup(ids, True))
    ms_occ = timed(occ, steps=8, warm=2)
    res["occurrence_order"] = {"what": "lookup + GroupAdam on the headline's batches with kv_set_deterministic(var, 2): the summed "
                                       "gradient of a repeated id is TF-core's occurrence-ordered fp32 sum bit for bit (one chain "
                                       "per key, k_occ_sum), so every key meets the 1e-6 of the op boundary against the CPU path",
                               "ms_per_step": ms_occ, "ids_per_s": N / (ms_occ * 1e-3)}
  except Exception as e:   # (e.g. the table still serves the shard of a sharded_world1 leg that failed half way: refused)
    res["occurrence_order"] = {"error": "%s: %s" % (type(e).__name__, e)}
  finally:
    ops.kv_set_deterministic(var, 0)
  return res


DUMP_ROWS_BYTES = 32 << 20     # --dump-outputs: the sample of the lookup's output rows
DUMP_STATE_BYTES = 16 << 20    # ... and of the var + slot rows of the batch's distinct ids


def dump_outputs(dirname, out, ids, ops, var, slot):
  """--dump-outputs: what the last timed step handed its caller, as float32 .npy files under `dirname` (48 MiB at most):
  lookup_rows.npy, the lookup's output rows at a fixed, seeded sample of batch positions (all of them when they fit);
  var_rows.npy / slot_rows.npy, the rows the step's apply left in the var and its slot table for a fixed, seeded sample
  of the batch's distinct ids, in ascending id order (var None: the sharded path, whose tables hold a part of the keys
  each).  The inputs are seeded, so the same arguments give the same positions and ids from run to run; the values agree
  up to the order in which a repeated id's gradient rows are summed (not fixed outside deterministic mode: ~1e-6
  absolute after a few hundred steps of the default workload)."""
  os.makedirs(dirname, exist_ok=True)
  rng = np.random.default_rng(SEED)
  N, D = out.shape
  n = min(N, DUMP_ROWS_BYTES // (4 * D))
  pos = torch.from_numpy(np.sort(rng.choice(N, n, replace=False))).to(out.device)
  np.save(os.path.join(dirname, "lookup_rows.npy"), out[pos].cpu().numpy().astype(np.float32))
  if var is None:
    return
  u = torch.unique(ids)
  n = min(u.numel(), DUMP_STATE_BYTES // (4 * 4 * D))         # var row (D) + slot row (3 D) per id
  keys = u[torch.from_numpy(np.sort(rng.choice(u.numel(), n, replace=False))).to(u.device)]
  np.save(os.path.join(dirname, "var_rows.npy"), ops.kv_variable_gather_or_zeros_v2(var, keys).cpu().numpy().astype(np.float32))
  np.save(os.path.join(dirname, "slot_rows.npy"), ops.kv_variable_gather_or_zeros_v2(slot, keys).cpu().numpy().astype(np.float32))


def exchange_block(world, cap, D, distinct_per_batch, lossless, staged):
  """The `exchange` object of a sharded line: what one rank puts on the wire per step.  Every peer gets one segment of
  peer_capacity + 1 records per exchange — (id, count) pairs out, rows back, summed gradient rows out — whatever the
  segment holds (fixed sizes: no size negotiation); a rank's own segment never leaves its buffers."""
  seg = cap + 1
  return {"exchanges_per_step": 3, "peer_capacity_records": cap, "lossless": bool(lossless),
          "wire_bytes_per_rank_per_step": (world - 1) * seg * (16 + 2 * 4 * D),
          "payload_bytes_per_rank_per_step_estimate": int((world - 1) / world * distinct_per_batch * (16 + 2 * 4 * D)),
          "transport": "debug: host-staged through gloo (kv_comm_create_staged)" if staged else
                       "grouped ncclSend / ncclRecv (RCCL) on the communicator's stream; a rank's own segment stays in place"}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--gpus", type=int, default=1)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--keys", type=int, default=50_000_000)
  ap.add_argument("--batch", type=int, default=1_000_000)
  ap.add_argument("--dim", type=int, default=32)
  ap.add_argument("--zipf", type=float, default=1.2)
  ap.add_argument("--pool", type=int, default=8, help="distinct pre-generated batches cycled through")
  ap.add_argument("--full", action="store_true",
                  help="after the timed steps, measure everything besides the headline: roofline and per-kernel table, the "
                       "sub-records of extras(), the CPU baseline (a plain run prints the headline only)")
  ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                  help="write what the last timed step computed to DIR/*.npy (float32; see dump_outputs)")
  ap.add_argument("--cpu-keys", type=int, default=50_000_000,
                  help="keys of the CPU baseline's table (BASELINE.md section 3: configs[1] = 50 M)")
  ap.add_argument("--cpu-build-budget", type=float, default=240.0,
                  help="seconds the CPU table build may take; when it runs out the baseline is timed on the keys inserted so far (and says so)")
  ap.add_argument("--cpu-steps", type=int, default=10)
  ap.add_argument("--no-extras", action="store_true",
                  help="with --full: skip the measurements taken after the timed region (skew sweep, op boundary, no token, staged)")
  ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
  ap.add_argument("--no-kernel-events", action="store_true",
                  help="diagnostic, with --full: do not bracket kernels with HIP events in the timed region (no roofline)")
  ap.add_argument("--no-token", action="store_true",
                  help="diagnostic: the apply rebuilds the batch index instead of taking over the lookup's")
  ap.add_argument("--deterministic", action="store_true",
                  help="diagnostic: the tables' deterministic reduction mode (kv_set_deterministic)")
  ap.add_argument("--graph", action="store_true",
                  help="diagnostic: the timed steps replay HIP graphs (one captured step per pooled batch)")
  ap.add_argument("--lossless", action="store_true",
                  help="sharded path: keep the library's default lossless mode (capacity agreed before every exchange; a host round trip per lookup) instead of opting into the synchronisation-free mode")
  ap.add_argument("--debug-capacity-skew", type=int, default=0,
                  help="test hook: rank r creates its shard with peer_capacity + r * this (ranks that disagree must fail "
                       "with FAILED_PRECONDITION at the first exchange, not hang)")
  ap.add_argument("--force-sharded", action="store_true",
                  help="run the all_to_all exchange path even with one rank (exercises the N > 1 code on one GPU)")
  args = ap.parse_args()
  if args.steps < 1:
    ap.error("--steps must be at least 1")

  rank = int(os.environ.get("RANK", "0"))
  world = int(os.environ.get("WORLD_SIZE", "1"))
  local = int(os.environ.get("LOCAL_RANK", "0"))
  # This program's stdout is ONE JSON line.  RCCL prints a version banner to the process's stdout (fd 1) when its first
  # communicator is made — torch.distributed's at N > 1, the library's own in the sharded_world1 record at N = 1 — so fd 1
  # points at stderr from here on and the line goes out through the saved descriptor (emit below).
  sys.stdout.flush()
  real_stdout = os.dup(1)
  os.dup2(2, 1)

  def emit(line):
    os.write(real_stdout, (line + "\n").encode())
  if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
    # not under a launcher: start one rank per GPU as CHILD processes (nothing in this process has touched the GPU
    # yet; a process that has must never be replaced by another), relay rank 0's JSON line, exit with their status
    import socket
    import subprocess
    with socket.socket() as so:
      so.bind(("127.0.0.1", 0))
      port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if lines:
      emit(lines[-1])
    sys.exit(r.returncode if r.returncode or lines else 1)
  # KV_BENCH_ONE_GPU=1 (debugging only, never a measurement): every rank shares cuda:0 and the
  # collectives are staged through gloo on the host, so the N > 1 control flow of this file can be
  # exercised on a 1-GPU box (RCCL refuses two ranks on one device)
  one_gpu_debug = os.environ.get("KV_BENCH_ONE_GPU") == "1" and world > 1
  if one_gpu_debug:
    local = 0
  ndev = torch.cuda.device_count()
  if ndev > 0:
    local %= ndev          # a launcher that masks devices per rank leaves one visible GPU: index 0
  torch.cuda.set_device(local)
  dev = torch.device("cuda", local)
  shard_path = world > 1 or args.force_sharded
  if shard_path:
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    if one_gpu_debug:
      dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
      dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

  from tfplus_amd import _lib
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  from tfplus_amd.kv_variable.python.ops.sharded import owner_of as _owner_of
  L = _lib.lib()

  D, N = args.dim, args.batch
  # weak scaling: every rank owns ~args.keys keys of a table of args.keys * world keys, sharded by the hashed owner
  # rule (mix64(id) >> 32) % world (KV_OWNER_HASH; the reference's floor_mod rule is the library's other option),
  # and feeds its own batch of N ids
  K = args.keys * world
  K_local = args.keys if world == 1 else int(args.keys * 1.05) + 1024
  gen = torch.Generator(device=dev).manual_seed(SEED + rank)
  table = (torch.randn(10000, D, device=dev, generator=torch.Generator(device=dev).manual_seed(SEED)) * 0.05)
  var = ops.kv_variable([D], capacity_hint=K_local + 24 * N, device=local)
  slot = ops.kv_variable([3 * D], capacity_hint=K_local + 24 * N, device=local)
  ops.init_kv_variable_v2(var, table)
  ops.init_kv_variable_v2(slot, torch.zeros(16, 3 * D, device=dev))
  stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

  # ---- pre-insert K keys (ids = splitmix64(rank)); optimizer state rows too: steady state ----
  CH = 1 << 22
  buf = torch.empty((CH, 3 * D), dtype=torch.float32, device=dev)
  owned = 0
  for i in range(0, K, CH):
    r = torch.arange(i + 1, min(i + CH, K) + 1, dtype=torch.int64, device=dev)
    keys = splitmix64(r)
    if world > 1:
      keys = keys[_owner_of(keys, world) == rank].contiguous()      # hashed ownership: (mix64(id) >> 32) % world
    owned += keys.numel()
    if keys.numel() == 0:
      continue
    _lib.check(L.kv_gather_or_insert(var.ptr, keys.data_ptr(), None, keys.numel(), buf.data_ptr(), stream))
    _lib.check(L.kv_gather_or_insert(slot.ptr, keys.data_ptr(), None, keys.numel(), buf.data_ptr(), stream))
  torch.cuda.synchronize()
  del buf
  assert ops.kv_variable_shape_v2(var)[0] == owned, (ops.kv_variable_shape_v2(var), owned)
  # steady state of a trained table: every key the optimizer has applied has its slot row remembered in
  # the var's index entry (what GroupAdamOptimizer's first apply per key leaves behind)
  ops.kv_attach_slot(var, slot)
  if args.deterministic:
    ops.kv_set_deterministic(var, True); ops.kv_set_deterministic(slot, True)

  # ---- synthetic batches, resident in HBM ----
  z = Zipf(K, args.zipf, dev)
  pool = []
  for p in range(args.pool):
    ids = splitmix64(z.sample(N, gen))
    grad = torch.randn(N, D, device=dev, generator=gen) * 1e-2
    U = int(torch.unique(ids).numel())
    E = S1 = None
    if args.full:
      # entries of the batch = distinct (2048-id tile, id) pairs; S1 of them occur once in their tile (their gradient
      # row goes straight to the apply, the others' rows are summed per tile first): the roofline's byte model
      tl = torch.arange(N, device=dev, dtype=torch.int64) // 2048
      _, ec = torch.unique(torch.stack([tl, ids], 1), dim=0, return_counts=True)
      E, S1 = int(ec.numel()), int((ec == 1).sum())
      del tl, ec
    pool.append((ids, grad, U, E, S1))
  out = torch.empty((N, D), dtype=torch.float32, device=dev)
  U_mean = float(np.mean([p[2] for p in pool]))

  state = {"b1p": np.float32(0.9), "b2p": np.float32(0.999)}

  native_shard = shard_path   # (KV_BENCH_ONE_GPU=1: the same ops over a host-staged communicator)

  def peer_capacity():
    """The records one rank may send one owner per batch — a deployment constant: both ends of every send / recv
    must agree on it without talking, so it is the SAME number on every rank (max over ranks here).  Sized from
    the workload: the most distinct ids any pooled batch holds, shared evenly by the hash, plus a quarter."""
    m = torch.tensor([max(p[2] for p in pool)], dtype=torch.int64, device="cpu" if (one_gpu_debug or world == 1) else dev)
    if world > 1:
      dist.all_reduce(m, op=dist.ReduceOp.MAX)
    return int(int(m.item()) / world * 1.25) + 1024
  if native_shard:
    # the production path: kvhip.h kv_shard_* over a kv_comm (RCCL grouped send / recv on its own stream; a world of
    # one still goes through RCCL here so that --force-sharded prices the whole mechanism).
    # Debugging mode (KV_BENCH_ONE_GPU=1): the SAME ops, every rank on cuda:0, over a communicator whose segments are
    # staged through gloo on the host (kv_comm_create_staged; RCCL refuses two ranks on one device) — the agreement,
    # verification and failure protocol of the N > 1 path run for real, only the wire differs.
    if one_gpu_debug:
      comm = ops.KvCommStaged(local)
    else:
      comm = ops.kv_comm_from_torch_distributed(local) if world > 1 else ops.KvComm(1, 0, ops.kv_comm_unique_id(), local)
    cap = peer_capacity() + args.debug_capacity_skew * rank
    shard = ops.KvShard(var, world, rank, ops.KV_OWNER_HASH, max_ids=N, peer_capacity=cap)
    # the library's default is lossless (ranks agree on the capacity before every exchange: one all-reduce + one host
    # round trip per lookup); the bench sizes peer_capacity from its own batches (peer_capacity() above: cannot overflow)
    # and OPTS INTO the synchronisation-free mode unless --lossless is given
    shard.set_lossless(bool(args.lossless))
    hp_t = ctypes.c_float * 9
    # this step has no dense tower to overlap with: queue it on the communicator's own stream, so the ops fork and
    # join nothing (with a tower on another stream each op pays one event hop in and one out, hidden behind it)
    comm_stream = comm.stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(comm_stream)
    stream = ctypes.c_void_p(comm_stream.cuda_stream)

  def teardown():
    """The library's communicator goes first (every rank past its last exchange), then torch's group."""
    torch.cuda.synchronize()
    if world > 1:
      dist.barrier()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))   # the communicator's stream is about to go
    held = [x for x in ("shard", "comm") if x in live]
    for x in held:
      obj = live.pop(x)
      if x == "comm":
        _lib.check(L.kv_comm_destroy(obj.ptr)); obj.ptr = None
      else:
        _lib.check(L.kv_shard_destroy(obj.ptr)); obj.ptr = None
    dist.destroy_process_group()

  live = {}
  if shard_path:
    live["shard"] = shard
    if native_shard:
      live["comm"] = comm

  def step(k):
    ids, grad = pool[k % len(pool)][:2]
    if not shard_path:
      st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)   # (the capture stream inside a graph capture)
      # the lookup names the batch; the apply of the same ids takes its index over (kvhip.h: batch token)
      tok = ctypes.c_uint64(0)
      _lib.check(L.kv_gather_or_insert_tok(var.ptr, ids.data_ptr(), None, N, out.data_ptr(), ctypes.byref(tok), st))
      _lib.check(L.kv_apply_group_adam_tok(var.ptr, slot.ptr, grad.data_ptr(), ids.data_ptr(), N, 1e-3,
                                           float(state["b1p"]), float(state["b2p"]), 0.9, 0.999, 1e-8, 0.0, 0.0,
                                           0.0, 4, tok.value if not args.no_token else 0, st))
    else:
      # ids -> owners (grouped send / recv over xGMI) -> rows back; summed gradients -> owners -> fused apply
      _lib.check(L.kv_shard_lookup(shard.ptr, comm.ptr, ids.data_ptr(), N, out.data_ptr(), 1, stream))
      hp = hp_t(1e-3, float(state["b1p"]), float(state["b2p"]), 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
      _lib.check(L.kv_shard_apply(shard.ptr, comm.ptr, 0, slot.ptr, None, grad.data_ptr(), hp, 1, stream))
    state["b1p"] = np.float32(state["b1p"] * np.float32(0.9))      # TF-core Adam _finish
    state["b2p"] = np.float32(state["b2p"] * np.float32(0.999))

  def barrier():
    torch.cuda.synchronize()
    if world > 1:
      dist.barrier()
      torch.cuda.synchronize()

  # A hipEvent pair around a kernel costs a few microseconds of stream time (five pairs per step
  # are ~16 % of this step), so only ONE kernel — the slowest one, found during the warm-up steps,
  # where every kernel is bracketed — carries events inside the timed region; that is the launch
  # `roofline` is computed from.  The per-kernel table (`kernels_ms`) comes from `steps` further
  # fully bracketed steps after the clock has stopped.  (--full only: a plain run brackets nothing.)
  if args.full:
    ops.kv_profile_enable(var, 16 * args.warmup + 8)
  for k in range(args.warmup):
    step(k)
  torch.cuda.synchronize()
  # the kernel to bracket in the timed region: the slowest one of three further untimed steps (the first warm-up
  # steps still allocate and insert).  A plain run takes the same three steps, unbracketed: the timed steps start
  # from the same state either way.
  dom = sample_every = None
  if args.full:
    ops.kv_profile_enable(var, 64)
  for k in range(3):
    step(args.warmup + k)
  torch.cuda.synchronize()
  if args.full:
    warm = ops.kv_profile_read(var)
    dom = max(warm, key=lambda k: warm[k][0] / max(warm[k][1], 1))
  graphs = None
  if args.graph and not shard_path:
    # one graph per pooled batch: no launch gaps.  (The Adam powers b1p / b2p are arguments by value: a replay uses
    # the ones of its capture.)
    ops.kv_profile_enable(var, 0)
    torch.cuda.synchronize()
    for h in (var, slot):
      ops.kv_prepare_capture(h, (len(pool) + 2) * N)
    graphs = []
    for p in range(len(pool)):
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g):
        step(p)
      graphs.append(g)
    for g in graphs:           # untimed: every graph once
      g.replay()
    torch.cuda.synchronize()
  if args.full:
    ops.kv_profile_enable(var, 0 if (args.no_kernel_events or graphs) else args.steps + 8)
    ops.kv_profile_select(var, [dom])
    sample_every = SAMPLE_EVERY if SAMPLE_EVERY > 0 else (2 if args.steps <= 24 else 5 if args.steps <= 64 else 8)   # >= 8 launches timed
    ops.kv_profile_sample(var, sample_every)     # a pair of event markers costs ~4 us of stream time per launch
  barrier()
  t0 = time.perf_counter()
  if graphs:
    for k in range(args.steps):
      graphs[(args.warmup + k) % len(graphs)].replay()
  else:
    for k in range(args.steps):
      step(args.warmup + k)
  torch.cuda.synchronize()
  t1 = time.perf_counter()
  dt = t1 - t0
  if world > 1:
    tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if one_gpu_debug else dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
  if args.full:
    timed = ops.kv_profile_read(var)
    ops.kv_profile_select(var, None)
    ops.kv_profile_sample(var, 1)
  if args.dump_outputs and rank == 0:     # before anything else runs on the tables
    last = (args.warmup + args.steps - 1) % len(pool)
    dump_outputs(args.dump_outputs, out, pool[last][0], ops, None if shard_path else var, slot)
    torch.cuda.synchronize()

  ms_per_step = dt / args.steps * 1e3
  value = N * world / (dt / args.steps)
  head = {
      "metric": "lookups+GroupAdam-applies/sec and HBM GB/s, 1M int64 ids x dim32",
      "value": value,
      "unit": "ids/s (each id: 1 embedding lookup + 1 fused GroupAdam-V4 apply)",
      "n_gpus": world,
      "steps": args.steps,
      "warmup": args.warmup,
      "ms_per_step": ms_per_step,
      "higher_is_better": True,
      "scaling": "weak",
      "vs_baseline": None,
      "dtype": "f32",
      "data": "synthetic",
      "config": {"workload": "configs[1]: %dM-key KvVariable x dim%d per GPU, %d ids/batch per GPU Zipf(%.1f), "
                             "lookup + sparse GroupAdam apply" % (args.keys // 1_000_000, D, N, args.zipf),
                 "keys": K, "dim": D, "batch": N, "zipf": args.zipf, "global_batch": N * world, "unique_per_batch": U_mean,
                 "parallelism": ("table sharded over %d GPUs by (mix64(id) >> 32) %% G, fixed-capacity id/row/grad exchange, "
                                 "grouped ncclSend/ncclRecv over RCCL" % world) if world > 1 else "single GPU"},
  }
  if not args.full:
    if rank == 0:
      emit(json.dumps(head))
    if shard_path:
      teardown()
    return

  prof = timed
  if not args.no_kernel_events:
    ops.kv_profile_enable(var, 8 * args.steps + 8)
    for k in range(args.steps):
      step(args.warmup + args.steps + k)
    torch.cuda.synchronize()
    prof = ops.kv_profile_read(var)
  ops.kv_profile_enable(var, 0)
  # sharded path: where the step's time goes, phase by phase (events on the communicator's stream at the phase
  # boundaries of the whole ops, kvhip.h kv_shard_profile) — `steps` further untimed steps, every one sampled
  shard_prof = None
  if shard_path:
    shard.profile(1)
    for k in range(args.steps):
      step(args.warmup + 2 * args.steps + k)
    torch.cuda.synchronize()
    shard_prof = shard.profile_read()
    shard.profile(0)
  # the COMPLETE lookup — output rows and the op's own bookkeeping (frequency words, day stamps, rows of new keys): a
  # token lookup defers that half to the head of the apply, where k_papply does it in the same pass as the update; a
  # lookup that is followed by another lookup runs it itself.  Timed here as a lookup-only loop (every lookup settles
  # the one before it), events on the op's stream, outside the timed region.
  lookup_complete_ms = None
  if not shard_path:
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    def look(k):
      tok = ctypes.c_uint64(0)
      _lib.check(L.kv_gather_or_insert_tok(var.ptr, pool[k % len(pool)][0].data_ptr(), None, N, out.data_ptr(), ctypes.byref(tok), st))
    for k in range(3):
      look(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(12):
      look(3 + k)
    e1.record()
    torch.cuda.synchronize()
    lookup_complete_ms = e0.elapsed_time(e1) / 12

  if args.no_kernel_events or graphs:
    if rank == 0:
      emit(json.dumps({"ms_per_step": ms_per_step, "value": value, "note": "diagnostic run without kernel events"}))
    if shard_path:
      teardown()
    return

  # ---- roofline of the dominant kernel: algorithmic bytes per launch / mean launch time ----
  # SURVEY.md §8(d) per-step figures, split over the kernels of each op by which kernel moves the
  # bytes: ids are read by the tile pass; the index probe and the output rows belong to
  # the partition pass (its gather blocks copy the rows); the apply reads every gradient row once and
  # reads + writes the optimizer state of every unique key in k_apply_sorted.
  Ub = U_mean
  E_mean = float(np.mean([p[3] for p in pool]))
  S1_mean = float(np.mean([p[4] for p in pool]))
  fused = prof["apply_tsum"][1] > 0 or prof["apply_tile"][1] > 0     # the entry-list pipeline ran (kv_fused.h)
  if fused:
    alg = {
        "lookup_tile": N * 8 + Ub * (16 + 4 * D) + N * 4 * D,   # k_ltile: ids, one probe + one row per key, output rows
        "apply_unique": 0,
        "lookup_part": 0,                                     # k_part2: row records only (not in SURVEY 8d's figure)
        "lookup_order": 0,
        "apply_index": N * 8 + Ub * 16,
        "apply_tsum": (N - S1_mean) * 4 * D,                   # k_tsum: gradient rows of ids repeated inside their tile
        "apply_tile": N * 8 + (N - S1_mean) * 4 * D,           # k_ltsum: the ids again (tile pass) + those gradient rows
        "apply_sorted": S1_mean * 4 * D + Ub * (16 + 4 * 4 * D) + Ub * 4 * 4 * D,   # k_papply: the other gradient rows + state r/w
        "apply_span": 0,
    }
  else:
    alg = {
        "lookup_tile": N * 8,
        "apply_unique": 0,
        "lookup_part": Ub * 16,
        "lookup_order": Ub * 4 * D + N * 4 * D + N * 4,
        "apply_index": N * 8 + Ub * 16,
        "apply_tsum": 0,
        "apply_tile": 0,
        "apply_sorted": N * 4 * D + Ub * (4 * 4 * D) + Ub * 4 * 4 * D,
        "apply_span": 0,
    }
  kern = {k: (ms / max(c, 1)) for k, (ms, c) in prof.items()}
  dom_ms = timed[dom][0] / max(timed[dom][1], 1)      # the dominant kernel, inside the timed region
  achieved = alg[dom] / (dom_ms * 1e-3) / 1e9
  # entry-list pipeline: a lookup that hands out a batch token returns when its rows are written (k_ltile); its
  # partition pass (k_part2: frequency words, key records) is deferred to the head of the apply of that batch
  lookup_ms = kern["lookup_tile"] + kern["lookup_order"] + (0.0 if fused and not args.no_token else kern["lookup_part"])
  apply_ms = kern["apply_index"] + kern["apply_sorted"] + kern["apply_span"] + kern["apply_tsum"] + kern["apply_tile"] + \
      (kern["lookup_part"] if fused and not args.no_token else 0.0)
  lookup_bytes = N * (8 + 4 * D) + Ub * (16 + 4 * D)
  apply_bytes = N * (8 + 4 * D) + Ub * (16 + 4 * 4 * D) + Ub * 4 * 4 * D

  # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process, so the
  # figure is the one collected by scripts_prof.sh (rocprofv3 --pmc passes of this same command) and
  # committed under profiles/; null when that file is absent or was taken on another workload.
  traffic, traffic_src, traffic_raw = None, None, None
  tj = None
  try:
    tj = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r06_traffic.json")))
    if tj.get("workload") == [K, N, D, args.zipf] and dom in tj["kernels"]:
      traffic = tj["kernels"][dom]["hbm_bytes"]
      traffic_raw = tj["kernels"][dom]["fetch_size_kib_raw"] * 1024 + tj["kernels"][dom]["write_bytes"]
      traffic_src = ("profiles/r06_traffic.json, a COMMITTED profile of this command taken on the builder's box (PMC counters "
                     "cannot be read from inside this process; not measured in this run): " + tj["source"])
    else:
      tj = None
  except (OSError, ValueError, KeyError):
    tj = None

  res = dict(head)
  res["config"].update({"tile_entries_per_batch": E_mean, "tile_entries_single": S1_mean})
  res.update({
      "roofline": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_fetch_uncorrected": traffic_raw,
                   "traffic_source": traffic_src,
                   "algorithmic_bytes_per_launch": alg[dom], "avg_launch_ms": dom_ms,
                   "launches_timed": int(timed[dom][1]),
                   "measured": "hipEvent pairs on the op's stream around every %dth launch of this kernel inside "
                               "the timed region" % sample_every},
      "kernels_ms": kern,
      "kernels": {k: {"ms": kern[k], "algorithmic_bytes": alg[k], "GBps": alg[k] / (kern[k] * 1e-3) / 1e9,
                      "frac": alg[k] / (kern[k] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "ceiling_frac": alg[k] / (kern[k] * 1e-3) / 1e9 / 5000.0,
                      "traffic": (tj["kernels"][k]["hbm_bytes"] if tj and k in tj["kernels"] else None)}
                  for k in kern if kern[k] > 0 and alg.get(k, 0) > 0},
      "kernels_ms_measured": "%d further steps after the timed region with every kernel bracketed" % args.steps,
      "ops": {"lookup": {"gpu_ms": lookup_ms, "rows_ready_ms": lookup_ms, "complete_ms": lookup_complete_ms,
                         "what": "rows_ready_ms (= gpu_ms): kernels until the output rows are complete" +
                         ("; the batch's bookkeeping runs inside its apply (k_papply)" if fused and not args.no_token else "") +
                         "; complete_ms: a lookup-only loop, every lookup running its own bookkeeping pass",
                         "algorithmic_bytes": lookup_bytes,
                         "GBps": lookup_bytes / (lookup_ms * 1e-3) / 1e9,
                         "frac_of_peak": lookup_bytes / (lookup_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "complete_frac_of_peak": (lookup_bytes / (lookup_complete_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if lookup_complete_ms else None,
                         "lookups_per_s": N / (lookup_ms * 1e-3)},
              "group_adam_apply": {"gpu_ms": apply_ms, "algorithmic_bytes": apply_bytes,
                                   "GBps": apply_bytes / (apply_ms * 1e-3) / 1e9,
                                   "frac_of_peak": apply_bytes / (apply_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                   "applies_per_s": N / (apply_ms * 1e-3),
                                   "unique_applies_per_s": Ub / (apply_ms * 1e-3)}},
  })
  if shard_path:
    # On the sharded path every rank runs the same kernels on what the exchange hands it (unique
    # ids per source rank; sizes change with every batch), so the per-launch byte model above does
    # not describe those launches: the kernels are characterised by the N = 1 line, this line
    # carries the measured launch time only.
    res["roofline"].update({"achieved": None, "frac": None, "traffic": None, "traffic_source": None,
                            "algorithmic_bytes_per_launch": None,
                            "note": "sharded path: kernel byte model is reported on the single-GPU line "
                                    "(launch sizes here depend on the exchanged unique ids)"})
    res.pop("ops", None)
    # xGMI traffic is reported apart from HBM: three fixed-size exchanges per step, every rank sends
    # every peer one segment of peer_capacity + 1 records — (id, count) pairs, rows back, summed gradient rows
    res["exchange"] = exchange_block(world, cap, D, Ub, bool(args.lossless), one_gpu_debug)
    # phase by phase (partition -> gather -> stitch, embedding_ops.py:115-204, and the gradient's way back): mean ms over
    # `steps` sampled steps taken after the timed region; the markers themselves cost stream time, so the sum runs a
    # few per cent over ms_per_step
    ph = shard_prof["phases_ms"]
    res["phases_ms"] = ph
    res["phases_sum_ms"] = sum(v for v in ph.values() if v)
    res["phases_samples"] = shard_prof["samples"]
    res["rccl_ranks_seen"] = shard_prof["rccl_ranks_seen"]
    seg = cap + 1
    wire = {"exchange_ids": (world - 1) * seg * 16, "exchange_rows": (world - 1) * seg * 4 * D, "exchange_grads": (world - 1) * seg * 4 * D}
    res["exchange"]["wire_GBps"] = {k: (b / (ph[k] * 1e-3) / 1e9 if ph.get(k) else None) for k, b in wire.items()}
    res["exchange"]["wire_bytes_per_exchange"] = wire
    res["exchange"]["capacity_grows"] = shard_prof["grows"]
    res["exchange"]["overflowed_batches"] = shard_prof["overflows"]
  # the calibrated ceiling of this access pattern (tools/calib_r03.hip, profiles/r03_calibration.txt): 1 M random
  # 128-B rows of a table far larger than the caches are read at 4.9-5.6 TB/s on this chip, whatever their order
  RANDOM_ROW_CEILING_GBS = 5000.0
  if res["roofline"].get("achieved"):
    res["roofline"]["ceiling"] = RANDOM_ROW_CEILING_GBS
    res["roofline"]["ceiling_frac"] = res["roofline"]["achieved"] / RANDOM_ROW_CEILING_GBS
    res["roofline"]["ceiling_source"] = "profiles/r03_calibration.txt: random 128-B row reads, 128 MB .. 32 GB footprints"
  res["step_GBps"] = (lookup_bytes + apply_bytes) / (ms_per_step * 1e-3) / 1e9
  res["step_frac_of_peak"] = res["step_GBps"] / HBM_PEAK_GBS
  res["repeated_id_tolerance"] = ("fp32 state within 1e-6 relative of the reference given the same summed gradient (the op "
                                  "boundary: unique ids + pre-summed rows); an id repeated in the batch is summed in tile / "
                                  "entry order, not TF-core's occurrence order: bounded per element by the reorder bound of "
                                  "tests/_reorder.py (typically a few 1e-6 relative), bit-reproducible in deterministic mode")
  if not shard_path and not args.no_extras:
    res.update(extras(args, ops, L, _lib, var, slot, dev, pool, out, K, N, D, gen, state))
    if tj and "apply_unique" in tj["kernels"]:      # HBM bytes of one k_uapply launch (committed profile, as roofline.traffic)
      res["op_boundary"]["traffic"] = tj["kernels"]["apply_unique"]["hbm_bytes"]
  if rank == 0 and world == 1 and not args.no_cpu_baseline and args.cpu_steps > 0:
    res["cpu_baseline"] = cpu_baseline(args, D)
  if rank == 0:
    emit(json.dumps(res))
  if shard_path:
    teardown()


if __name__ == "__main__":
  main()
