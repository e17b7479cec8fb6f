"""Group Momentum's and group Adadelta's sparse step beside group AMSGrad's: 1 M Zipf(1.2) ids over a filled table of 2 M keys, dim
32 and 128.  Four sides per dim — group AMSGrad, group Momentum, group Momentum with use_nesterov, group Adadelta — each the
family's plain op on the raw ids and gradient rows, no lookup in the timed window.  The three variants of OPT_GROUP_ACC3 move
the var row and a slot row of three blocks where group AMSGrad moves four; Momentum's arithmetic is one root and one division
per element, Adadelta's four roots and three divisions.  The sides alternate, REPS windows each in one process; a window is as
many back-to-back steps as fill a quarter of a second (counted once, from a trial window), timed on the host clock around a
device synchronise, reported per step: median and spread (standard deviation over the windows).  No expectation is asserted.
python tools/group_acc3_step.py [other.so] > profiles/group_acc3_step.txt"""
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
HP4 = (f(1e-3), f(0.9) ** 20, f(0.999) ** 20, f(0.9), f(0.999), f(1e-7), 0.0, 0.0, 0.0)   # lr ... epsilon, l1, l2, l21


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


ids = bench.Zipf(KEYS, 1.2, dev).sample(N, g) - 1
print("1 table, %d ids Zipf(1.2) over %d keys (%d distinct), %d windows of %.2f s per side, alternating"
      % (N, KEYS, int(torch.unique(ids).numel()), REPS, WINDOW))
# (name, slot blocks, the op on (var, slot, grad))
SIDES = [("group_amsgrad", 4, lambda v, s, gr: ops.kv_variable_group_sparse_apply_amsgrad(v, s, gr, ids, *HP4)),
         ("group_momentum", 3, lambda v, s, gr: ops.kv_variable_group_sparse_apply_momentum(v, s, gr, ids, 1e-3, 0.9, 0.0, 0.0, 0.0)),
         ("group_nesterov", 3, lambda v, s, gr: ops.kv_variable_group_sparse_apply_momentum(v, s, gr, ids, 1e-3, 0.9, 0.0, 0.0, 0.0, True)),
         ("group_adadelta", 3, lambda v, s, gr: ops.kv_variable_group_sparse_apply_adadelta(v, s, gr, ids, 1e-3, 0.95, 1e-6, 0.0, 0.0, 0.0))]
for D in (32, 128):
  grad = torch.randn(N, D, device=dev, generator=g) * 1e-2
  # one (var, slot) pair per side: the sides share no rows, each step starts from what its own last step left
  fns = [(lambda fn=fn, v=table(D), s=table(b * D, 0.0): fn(v, s, grad)) for _, b, fn in SIDES]
  for fn in fns:
    for _ in range(3):
      fn()
  calls = [max(1, int(WINDOW * 1e6 / window(fn, 3))) for fn in fns]
  times = [[] for _ in fns]
  for _ in range(REPS):
    for t, fn, c in zip(times, fns, calls):
      t.append(window(fn, c))
  base = statistics.median(times[0])
  for (name, b, _), t, c in zip(SIDES, times, calls):
    print("  dim %3d  %-14s %d slot blocks  %8.1f us (spread %5.1f, %3d steps / window)   %.2fx group AMSGrad"
          % (D, name, b, statistics.median(t), statistics.stdev(t), c, statistics.median(t) / base))
  del fns
