"""embedding_lookup_sparse outside training at two serving shapes: 26 tables (dims 64 / 128) x 2048 segments and 8 tables x
50 000 segments, 1-8 ids per segment, Zipf(1.2) ids over filled tables, weighted mean.  Times, per step over all tables:
  (a) kv_batch_lookup_sparse_zeros      one launch for all tables
  (b) kv_lookup_sparse_zeros            table by table
  (c) the op chain, table by table      what embedding_lookup_sparse ran in inference mode before the fused op: unique ->
                                        GatherOrZeros -> index_select -> multiply -> index_add x 2 -> divide, and the host
                                        sync for the segment count; restated here with plain torch ops
  (d) kv_batch_gather_or_zeros          over the same id lists: the bytes reference (it WRITES the [n, dim] rows (a) only sums)
Expectation, checked at the end: on the 26-table shape (a) is below (c) by a wide factor (here: at least 3x) — (a) is one
launch, (c) at least eight launches and a host sync per feature.  python tools/serving_sparse.py [other.so]"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)


def chain(h, ids, seg, w):
  nseg = int(seg.max().item()) + 1
  uniq, idx, _ = torch.unique(ids, return_inverse=True, return_counts=True)
  emb = ops.kv_variable_gather_or_zeros_v2(h, uniq).index_select(0, idx)
  wts = w.reshape(-1, 1)
  summed = torch.zeros((nseg, emb.shape[1]), device=dev).index_add(0, seg, emb * wts)
  return summed / torch.zeros((nseg, 1), device=dev).index_add(0, seg, wts)


def timed(fn, reps):
  for _ in range(3): fn()
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(reps): fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e6


verdict = None
for ntab, nseg, keys, reps in ((26, 2048, 200_000, 50), (8, 50_000, 2_000_000, 20)):
  hs, idl, segl, wl = [], [], [], []
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
    idl.append(z.sample(seg.numel(), g) - 1)
    wl.append(torch.rand(seg.numel(), device=dev, generator=g) + 0.5)
  nsegs = [nseg] * ntab
  nids = sum(i.numel() for i in idl)
  # the three paths compute the same thing
  a = ops.batch_kv_variable_lookup_sparse_zeros(hs, idl, segl, wl, nsegs, "mean")
  for k in range(ntab):
    assert torch.equal(a[k], ops.kv_variable_lookup_sparse_zeros(hs[k], idl[k], segl[k], wl[k], nseg, "mean"))
    torch.testing.assert_close(a[k], chain(hs[k], idl[k], segl[k], wl[k]), rtol=1e-5, atol=1e-6)
  runs = (("(a) batched op, one launch", lambda: ops.batch_kv_variable_lookup_sparse_zeros(hs, idl, segl, wl, nsegs, "mean")),
          ("(b) single-table op x tables", lambda: [ops.kv_variable_lookup_sparse_zeros(h, i, s, w, nseg, "mean")
                                                    for h, i, s, w in zip(hs, idl, segl, wl)]),
          ("(c) op chain x tables", lambda: [chain(h, i, s, w) for h, i, s, w in zip(hs, idl, segl, wl)]),
          ("(d) batched gather_or_zeros", lambda: ops.batch_kv_variable_gather_or_zeros_v2(hs, idl)))
  print("%d tables x %d segments, %d ids in all (1-8 per segment), Zipf(1.2) over %d keys per table, dims 64 / 128" %
        (ntab, nseg, nids, keys))
  best = {}
  for rnd in range(3):                                   # the paths alternate: three rounds each
    for name, fn in runs:
      t = timed(fn, reps)
      best[name] = min(best.get(name, t), t)
      print("  round %d  %-30s %9.1f us per step" % (rnd, name, t))
  ta, tc = best[runs[0][0]], best[runs[2][0]]
  print("  best of 3: (a) %.1f us, (b) %.1f us, (c) %.1f us, (d) %.1f us; (c) / (a) = %.1fx" %
        (ta, best[runs[1][0]], tc, best[runs[3][0]], tc / ta))
  if ntab == 26:
    verdict = tc / ta
  del hs, a
print("expectation (26 tables: (a) at least 3x below (c)): %s (%.1fx)" % ("MET" if verdict >= 3.0 else "NOT MET", verdict))
sys.exit(0 if verdict >= 3.0 else 1)
