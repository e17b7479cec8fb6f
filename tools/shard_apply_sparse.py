"""The backward of embedding_lookup_sparse on SHARDED tables, at world 1 (a communicator without RCCL: the exchange is skipped,
this rank's segment stays in place), on tools/shard_sparse.py's two shapes — 26 tables (dims 64 / 128) x 2048 segments and
8 tables x 50 000 segments, 1-8 ids per segment, Zipf(1.2) ids over filled tables — and one single-table row: 1 M positions
at dim 32.  Per step, after the training lookup of the batch (not timed):
  (f) kv_[multi_]shard_apply_sparse           the gradient pre-sum reads the segment gradients [num_segments, dim] through
                                              per-position records; the [n, dim] values are never written
  (c) the composition available before it     kv_[multi_]lookup_sparse_grad expands them into [n, dim] values (one call per
                                              dim), kv_[multi_]shard_apply reads those back to pre-sum them
Both run the same exchange and the same owners' GroupAdam apply; they differ in the pre-sum and what feeds it.  The two
alternate, REPS repetitions each in one process, every repetition timed on the host clock around a device synchronise.
Prints the median, the spread (standard deviation over the repetitions) and the bytes each side's pre-sum moves, computed from
the shapes (and, for the single table, the pre-sum phases alone: kv_shard_apply_route_sparse against kv_lookup_sparse_grad +
kv_shard_apply_route on one routed batch).
Expectation, checked at the end: (f)'s median is not above (c)'s by more than (c)'s own spread, in every row.
python tools/shard_apply_sparse.py [other.so]"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)
REPS = 24
HP = (1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
OPT = ops.OPT_GROUP_ADAM_V4


def one(fn):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e6


def table(D, keys):
  h = ops.kv_variable([D], capacity_hint=keys + 1024)
  s = ops.kv_variable([3 * D], capacity_hint=keys + 1024)
  ops.init_kv_variable_v2(h, torch.randn(256, D, device=dev))
  ops.init_kv_variable_v2(s, torch.zeros(4, 3 * D, device=dev))
  for j in range(0, keys, 1 << 20):
    ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), keys), device=dev))
  return h, s


def presum_bytes(idl, segl, hs, nsegs, weighted):
  """(fused, composition) bytes of the pre-sum and what feeds it, from the shapes: both read the segment gradients once, the
  segment ids (8) and weights (4), the source words of the sums (4 per position), and write one row per distinct id; the
  composition also writes the [n, dim] values and reads them back, the fused form writes and reads 8 bytes of position
  records"""
  f = c = 0
  for i, h, m in zip(idl, hs, nsegs):
    n, row = i.numel(), h.dim * 4
    common = m * row + n * (8 + (4 if weighted else 0) + 4) + int(torch.unique(i).numel()) * row
    f += common + 2 * n * 8
    c += common + 2 * n * row
  return f, c


def timed(fused, comp, lookup):
  for _ in range(3):                                         # every shape of the timed window, both sides
    lookup(); fused(); lookup(); comp()
  tf, tc = [], []
  for _ in range(REPS):                                      # the paths alternate
    lookup(); tf.append(one(fused))
    lookup(); tc.append(one(comp))
  return statistics.median(tf), statistics.stdev(tf), statistics.median(tc), statistics.stdev(tc)


def report(label, mf, sf, mc, sc, fb, cb):
  met = mf <= mc + sc
  print("  %-22s (f) fused %9.1f us (spread %6.1f)   (c) composition %9.1f us (spread %6.1f)   (c) / (f) = %.2fx   "
        "pre-sum bytes: (f) %.1f MB, (c) %.1f MB   %s" % (label, mf, sf, mc, sc, mc / mf, fb / 1e6, cb / 1e6, "MET" if met else "NOT MET"))
  return met


ok = True
comm = ops.KvComm(1, 0, None)
for ntab, nseg, keys in ((26, 2048, 200_000), (8, 50_000, 2_000_000)):
  hs, ss, shs, idl, segl, wl, sgl = [], [], [], [], [], [], []
  z = bench.Zipf(keys, 1.2, dev)
  for i in range(ntab):
    D = 64 if i % 2 == 0 else 128
    h, s = table(D, keys)
    lens = torch.randint(1, 9, (nseg,), device=dev, generator=g)
    seg = torch.repeat_interleave(torch.arange(nseg, device=dev), lens)
    hs.append(h); ss.append(s); segl.append(seg)
    shs.append(ops.KvShard(h, 1, 0, max_ids=seg.numel()))
    idl.append(z.sample(seg.numel(), g) - 1)
    wl.append(torch.rand(seg.numel(), device=dev, generator=g) + 0.5)
    sgl.append(torch.randn(nseg, D, device=dev, generator=g) * 1e-2)
  nsegs = [nseg] * ntab
  nids = sum(i.numel() for i in idl)
  slots = [[s] for s in ss]
  by_dim = [[k for k in range(ntab) if hs[k].dim == D] for D in (64, 128)]
  print("%d sharded tables (world 1) x %d segments, %d ids in all (1-8 per segment), Zipf(1.2) over %d keys per table, dims 64 / 128"
        % (ntab, nseg, nids, keys))
  for combiner, weighted in (("sum", False), ("mean", True)):
    ws = wl if weighted else None
    lookup = lambda: ops.kv_multi_shard_lookup_sparse(shs, comm, idl, segl, ws, nsegs, combiner)
    fused = lambda: ops.kv_multi_shard_apply_sparse(shs, comm, OPT, slots, sgl, segl, ws, nsegs, combiner, HP)

    def comp():
      values = [None] * ntab
      for grp in by_dim:                                     # (the batched expand takes tables of one dim)
        out = ops.kv_multi_lookup_sparse_grad([hs[k] for k in grp], [sgl[k] for k in grp], [segl[k] for k in grp],
                                              None if ws is None else [ws[k] for k in grp], [nseg] * len(grp), combiner)
        for k, v in zip(grp, out):
          values[k] = v
      ops.kv_multi_shard_apply(shs, comm, OPT, slots, values, HP)
    fb, cb = presum_bytes(idl, segl, hs, nsegs, weighted)
    ok = report("%s %s" % (combiner, "weighted" if weighted else "unweighted"), *timed(fused, comp, lookup), fb, cb) and ok
  del hs, ss, shs, slots

# one table: 1 M positions at dim 32
D, keys, n = 32, 2_000_000, 1 << 20
h, s = table(D, keys)
lens = torch.randint(1, 9, (n // 4,), device=dev, generator=g)
seg = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens)[:n]
nseg = int(seg[-1]) + 1
ids = bench.Zipf(keys, 1.2, dev).sample(n, g) - 1
w = torch.rand(n, device=dev, generator=g) + 0.5
sg = torch.randn(nseg, D, device=dev, generator=g) * 1e-2
sh = ops.KvShard(h, 1, 0, max_ids=n)
print("1 sharded table (world 1), dim %d: %d positions in %d segments (1-8 per segment), Zipf(1.2) over %d keys" % (D, n, nseg, keys))
for combiner, weighted in (("sum", False), ("mean", True)):
  ww = w if weighted else None
  lookup = lambda: sh.lookup_sparse(comm, ids, seg, ww, nseg, combiner)
  # (the native op through its entry point: whatever KvShard.apply_sparse is wired to, this row times kv_shard_apply_sparse)
  fused = lambda: _lib.check(_lib.lib().kv_shard_apply_sparse(
      sh.ptr, comm.ptr, OPT, s.ptr, None, sg.data_ptr(), seg.data_ptr(), _lib.KV_DT_INT64, None if ww is None else ww.data_ptr(), nseg,
      ops._COMBINERS[combiner], ops._hp_array(HP), 1, ops._stream(h)))
  comp = lambda: sh.apply(comm, OPT, [s], ops.kv_variable_lookup_sparse_grad(h, sg, seg, ww, nseg, combiner), HP)
  fb, cb = presum_bytes([ids], [seg], [h], [nseg], weighted)
  label = "%s %s" % (combiner, "weighted" if weighted else "unweighted")
  ok = report(label, *timed(fused, comp, lookup), fb, cb) and ok
  # the pre-sum phases alone, on one routed batch (the route index stays: the phases can run again and again); the two leave
  # the same sums in send_rows (another order of the same terms in the default mode)
  sh.lookup_route(ids)
  rows = sh.buffers()["send_rows"].view(torch.float32)
  pf = lambda: sh.apply_route_sparse(sg, seg, ww, nseg, combiner)
  pc = lambda: sh.apply_route(ops.kv_variable_lookup_sparse_grad(h, sg, seg, ww, nseg, combiner))
  rows.zero_()
  pc(); torch.cuda.synchronize(); want = rows.clone()
  pf(); torch.cuda.synchronize()
  torch.testing.assert_close(rows, want, rtol=1e-4, atol=1e-6)
  report(label + ", pre-sum alone", *timed(pf, pc, lambda: None), fb, cb)      # (information: the expectation is on the whole op)
print("expectation ((f) not above (c) by more than (c)'s spread over %d repetitions, every row): %s" % (REPS, "MET" if ok else "NOT MET"))
sys.exit(0 if ok else 1)
