"""Plain RectifiedAdam's sparse step, fused against the composition: 1 M Zipf(1.2) ids over a filled table of 2 M keys, dim 32
and 128, without and with amsgrad (tractable, nesterov off, no weight decay).  Per step, no lookup in the timed window:
  (f) fused        kv_apply_rectified_adam on the raw ids and gradient rows: one slot table m | v | vhat, the duplicate sum,
                   the row arithmetic and the bookkeeping in the apply kernels
  (c) composition  RectifiedAdamOptimizer(fused=False)'s chain on separate m / v / vhat tables: kv_dedup_segment_sum
                   (synchronous), two or three gather_or_insert, the torch arithmetic, two or three scatter_update, scatter_sub
The two alternate, REPS windows each in one process; a window is as many back-to-back steps as fill a quarter of a second
(counted once, from a trial window), timed on the host clock around a device synchronise, reported per step.  Prints the
median, the spread (standard deviation over the windows) and whether the two medians lie inside each other's spread.  No
expectation is asserted: nobody has measured this before.
python tools/rectified_adam_step.py [other.so] > profiles/radam_step.txt"""
import os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)
REPS, WINDOW, KEYS, N = 12, 0.25, 2_000_000, 1 << 20
f = np.float32
B1, B2, B1P, B2P, EPS, LR, RT = f(0.9), f(0.999), f(0.9) ** 20, f(0.999) ** 20, f(1e-7), f(1e-3), f(0.4)


def window(fn, calls):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e6 / calls


def table(dim, fill=None):
  h = ops.kv_variable([dim], capacity_hint=KEYS + 1024)
  ops.init_kv_variable_v2(h, torch.randn(256, dim, device=dev) if fill is None else torch.full((4, dim), fill, device=dev))
  for j in range(0, KEYS, 1 << 20):
    ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), KEYS), device=dev))
  return h


def composed(var, m_tab, v_tab, vh_tab, ids, grad):
  """RectifiedAdamOptimizer._resource_apply_sparse (fused=False) with this script's scalars"""
  u, s, _ = ops.kv_dedup_segment_sum(var, ids, grad)
  m = float(B1) * ops.kv_variable_gather_or_insert_v2(m_tab, u) + s * float(f(1) - B1)
  ops.kv_variable_scatter_update_v2(m_tab, u, m)
  m_corr = m / float(f(1) - B1P)
  v = float(B2) * ops.kv_variable_gather_or_insert_v2(v_tab, u) + (s * s) * float(f(1) - B2)
  ops.kv_variable_scatter_update_v2(v_tab, u, v)
  if vh_tab is not None:
    v = torch.maximum(v, ops.kv_variable_gather_or_insert_v2(vh_tab, u))
    ops.kv_variable_scatter_update_v2(vh_tab, u, v)
  upd = float(RT) * m_corr / (torch.sqrt(v / float(f(1) - B2P)) + float(EPS))
  ops.kv_variable_scatter_sub_v2(var, u, upd * float(LR))


ids = bench.Zipf(KEYS, 1.2, dev).sample(N, g) - 1
print("1 table, %d ids Zipf(1.2) over %d keys (%d distinct), %d windows of %.2f s per side, alternating"
      % (N, KEYS, int(torch.unique(ids).numel()), REPS, WINDOW))
for D in (32, 128):
  grad = torch.randn(N, D, device=dev, generator=g) * 1e-2
  for ams in (0, 1):
    # one set of tables per side: the sides do not share rows, each step starts from what its own last step left
    vf, sf = table(D), table(3 * D, 0.0)
    vc, mc_, vv, vh = table(D), table(D, 0.0), table(D, 0.0), (table(D, 0.0) if ams else None)
    fused = lambda: ops.kv_variable_sparse_apply_rectified_adam(vf, sf, grad, ids, LR, B1P, B2P, B1, B2, EPS, 0.0, RT, 1, ams, 0)
    comp = lambda: composed(vc, mc_, vv, vh, ids, grad)
    for _ in range(3):
      fused(); comp()
    nf, nc = (max(1, int(WINDOW * 1e6 / window(fn, 3))) for fn in (fused, comp))
    tf, tc = [], []
    for _ in range(REPS):
      tf.append(window(fused, nf)); tc.append(window(comp, nc))
    mf, mc = statistics.median(tf), statistics.median(tc)
    noise = abs(mf - mc) <= max(statistics.stdev(tf), statistics.stdev(tc))
    print("  dim %3d  amsgrad %d   (f) fused %8.1f us (spread %5.1f, %3d steps / window)   (c) composition %8.1f us (spread %5.1f, "
          "%3d steps / window)   (c) / (f) = %.2fx%s" % (D, ams, mf, statistics.stdev(tf), nf, mc, statistics.stdev(tc), nc, mc / mf,
                                                        " (inside the spread)" if noise else ""))
    del vf, sf, vc, mc_, vv, vh
