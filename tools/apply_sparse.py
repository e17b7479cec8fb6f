"""The backward of embedding_lookup_sparse on a PLAIN table: 1 M Zipf(1.2) ids over a filled table of 2 M keys, segments of
1, 8 and 64 ids, GroupAdam V4 and Adagrad at dims 32 and 128, weighted mean.  Per step (no lookup in the timed window: both
sides index the ids themselves, as the training sparse lookup leaves no token):
  (f) kv_apply_sparse                         tile sums and partition pass + update read the segment gradients
                                              [num_segments, dim] through per-position records; no [n, dim] values exist
  (c) the composition available before it     kv_lookup_sparse_grad expands them into [n, dim] values, the plain
                                              kv_apply_<optimizer> reads those back (k_ltsum, k_papply)
The two alternate, REPS windows each in one process; a window is CALLS back-to-back calls (4 - 10 ms of device work) timed on
the host clock around a device synchronise, reported per call.  Prints the median, the spread (standard deviation over the
windows), whether the two medians lie inside each other's spread, and the bytes that differ between the
sides, from the shapes: (c) writes and reads n * dim * 4 of values; (f) writes 8 n of records and reads them in both sum
launches.  No expectation is asserted: nobody has measured this before.
python tools/apply_sparse.py [other.so] > profiles/apply_sparse.txt"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)
REPS, CALLS, KEYS, N = 12, 20, 2_000_000, 1 << 20
FAMILIES = {"GroupAdam V4": ("group_adam", 3, 0.0, (1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 4)),
            "Adagrad": ("adagrad", 1, 0.1, (0.05, True))}


def one(fn):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(CALLS):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e6 / CALLS


def tables(D, mult, fill):
  h = ops.kv_variable([D], capacity_hint=KEYS + 1024)
  s = ops.kv_variable([mult * D], capacity_hint=KEYS + 1024)
  ops.init_kv_variable_v2(h, torch.randn(256, D, device=dev))
  ops.init_kv_variable_v2(s, torch.full((4, mult * D), fill, device=dev))
  for j in range(0, KEYS, 1 << 20):
    ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), KEYS), device=dev))
  return h, s


ids = bench.Zipf(KEYS, 1.2, dev).sample(N, g) - 1
w = torch.rand(N, device=dev, generator=g) + 0.5
print("1 table, %d ids Zipf(1.2) over %d keys (%d distinct), weighted mean, %d windows of %d calls per side, alternating"
      % (N, KEYS, int(torch.unique(ids).numel()), REPS, CALLS))
for name, (stem, mult, fill, sc) in FAMILIES.items():
  for D in (32, 128):
    # one pair of tables per side: the sides do not share rows, each step starts from what its own last step left
    (hf, sf), (hc, sc_) = tables(D, mult, fill), tables(D, mult, fill)
    for L in (1, 8, 64):
      nseg = (N + L - 1) // L
      seg = torch.arange(N, device=dev) // L
      sg = torch.randn(nseg, D, device=dev, generator=g) * 1e-2
      fused = lambda: ops.kv_variable_apply_sparse(stem, (hf, sf), sc, sg, ids, seg, w, nseg, "mean")
      comp = lambda: ops._apply(stem, (hc, sc_), ops.kv_variable_lookup_sparse_grad(hc, sg, seg, w, nseg, "mean"), ids, sc, False)
      for _ in range(3):
        fused(); comp()
      tf, tc = [], []
      for _ in range(REPS):
        tf.append(one(fused)); tc.append(one(comp))
      mf, mc = statistics.median(tf), statistics.median(tc)
      noise = abs(mf - mc) <= max(statistics.stdev(tf), statistics.stdev(tc))
      print("  %-12s dim %3d  %2d ids / segment   (f) fused %8.1f us (spread %5.1f)   (c) composition %8.1f us (spread %5.1f)   "
            "(c) / (f) = %.2fx%s   values avoided %.0f MB, records added %.0f MB"
            % (name, D, L, mf, statistics.stdev(tf), mc, statistics.stdev(tc), mc / mf, " (inside the spread)" if noise else "",
               2 * N * D * 4 / 1e6, 3 * N * 8 / 1e6))
    del hf, sf, hc, sc_
