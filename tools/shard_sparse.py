"""embedding_lookup_sparse on SHARDED tables outside training, at world 1 (a communicator without RCCL: the exchanges are
skipped, this rank's segment stays in place), on tools/serving_sparse.py's two shapes: 26 tables (dims 64 / 128) x 2048
segments and 8 tables x 50 000 segments, 1-8 ids per segment, Zipf(1.2) ids over filled tables.  Per step over all tables:
  (f) kv_multi_shard_lookup_sparse_zeros      the finish combines into segments: [num_segments, dim] is written once
  (c) the composition available before it     kv_multi_shard_lookup_zeros writes the [n, dim] rows, then per table
                                              kv_unsorted_segment_sum (sum, unweighted) or the torch combine (weighted mean:
                                              multiply, index_add x 2, divide)
Both run route, serve and the lossless agreement alike; they differ in the finish and what follows it.  The two alternate,
REPS repetitions each in one process, every repetition timed on the host clock around a device synchronise.  Prints the
median, the spread (standard deviation over the repetitions) and the bytes each side's finish moves, computed from the shapes.
Expectation, checked at the end: (f)'s median is not above (c)'s by more than (c)'s own spread, in every row.
python tools/shard_sparse.py [other.so]"""
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


def one(fn):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e6


def torch_mean(rows, seg, w, nseg):
  wts = w.reshape(-1, 1)
  summed = torch.zeros((nseg, rows.shape[1]), device=dev).index_add(0, seg, rows * wts)
  return summed / torch.zeros((nseg, 1), device=dev).index_add(0, seg, wts)


ok = True
comm = ops.KvComm(1, 0, None)
for ntab, nseg, keys in ((26, 2048, 200_000), (8, 50_000, 2_000_000)):
  hs, shs, idl, segl, wl = [], [], [], [], []
  z = bench.Zipf(keys, 1.2, dev)
  for i in range(ntab):
    D = 64 if i % 2 == 0 else 128
    h = ops.kv_variable([D], capacity_hint=keys + 1024)
    ops.init_kv_variable_v2(h, torch.randn(256, D, device=dev))
    for j in range(0, keys, 1 << 20):
      ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), keys), device=dev))
    lens = torch.randint(1, 9, (nseg,), device=dev, generator=g)
    seg = torch.repeat_interleave(torch.arange(nseg, device=dev), lens)
    hs.append(h); segl.append(seg)
    shs.append(ops.KvShard(h, 1, 0, max_ids=seg.numel()))
    idl.append(z.sample(seg.numel(), g) - 1)
    wl.append(torch.rand(seg.numel(), device=dev, generator=g) + 0.5)
  nsegs = [nseg] * ntab
  nids = sum(i.numel() for i in idl)
  seg32 = [s.to(torch.int32) for s in segl]
  print("%d sharded tables (world 1) x %d segments, %d ids in all (1-8 per segment), Zipf(1.2) over %d keys per table, dims 64 / 128"
        % (ntab, nseg, nids, keys))
  # bytes of the finish and what follows it, from the shapes: the rows read from the receive buffer, the index chain
  # (pos_ent 2 + ent_u 4 + slot_of 4 per position), segment ids (8) and weights (4), the output
  row_b = sum(i.numel() * h.dim * 4 for i, h in zip(idl, hs))
  out_b = sum(nseg * h.dim * 4 for h in hs)
  idx_b = nids * 10
  for combiner, weighted in (("sum", False), ("mean", True)):
    ws = wl if weighted else None
    fused = lambda: ops.kv_multi_shard_lookup_sparse_zeros(shs, comm, idl, segl, ws, nsegs, combiner)
    if combiner == "sum":
      comp = lambda: [ops.kv_unsorted_segment_sum(h, r, s, nseg)
                      for h, r, s in zip(hs, ops.kv_multi_shard_lookup_zeros(shs, comm, idl), seg32)]
    else:
      comp = lambda: [torch_mean(r, s, w, nseg) for r, s, w in zip(ops.kv_multi_shard_lookup_zeros(shs, comm, idl), segl, wl)]
    a, b = fused(), comp()                                   # the two compute the same thing
    for x, y in zip(a, b):
      torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6)
    for _ in range(3):
      fused(); comp()
    tf, tc = [], []
    for _ in range(REPS):                                    # the paths alternate
      tf.append(one(fused)); tc.append(one(comp))
    mf, mc, sf, sc = statistics.median(tf), statistics.median(tc), statistics.stdev(tf), statistics.stdev(tc)
    fb = row_b + idx_b + nids * (8 + (4 if weighted else 0)) + out_b
    # the composition: the plain finish writes the rows, the combine reads them back (the torch mean also writes and reads
    # their product with the weights), segment ids as the combine takes them
    cb = row_b + idx_b + 2 * row_b * (2 if weighted else 1) + nids * ((8 + 4) if weighted else 4) + out_b
    met = mf <= mc + sc
    ok = ok and met
    print("  %-4s %-10s (f) fused %9.1f us (spread %6.1f)   (c) composition %9.1f us (spread %6.1f)   (c) / (f) = %.2fx   "
          "finish bytes: (f) %.1f MB, (c) %.1f MB   %s" % (combiner, "weighted" if weighted else "unweighted", mf, sf, mc, sc, mc / mf,
                                                          fb / 1e6, cb / 1e6, "MET" if met else "NOT MET"))
  del hs, shs, a, b
print("expectation ((f) not above (c) by more than (c)'s spread over %d repetitions, every row): %s" % (REPS, "MET" if ok else "NOT MET"))
sys.exit(0 if ok else 1)
