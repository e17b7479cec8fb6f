"""The sparse lookup's backward and its batched form, each against what the Python layer did before them.

Backward: 1 M Zipf(1.2) ids, dim 32, mean combiner, segment lengths 1 / 4 / 16 / 64 — the torch glue (restated below
exactly as _SparseLookupGrad.backward ran it: ones, index_add_, index_select, a division, a second index_select, a
broadcast multiply, .contiguous()) against kv_lookup_sparse_grad.
Batched: 26 tables x 2048 ids x segment length 4, dim 32, forward plus backward — kv_lookup_sparse and
kv_lookup_sparse_grad table by table against kv_multi_lookup_sparse and kv_multi_lookup_sparse_grad.

The two sides of a pair alternate round by round inside one process; the figure is the median round, by device events.
python tools/sparse_step.py [other.so]"""
import os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
D = 32


def glue_backward(grad, seg, w, nseg, combiner):
  """the gradient rows as the torch glue built them"""
  seg = seg.to(torch.int64)
  n = seg.numel()
  wj = torch.ones(n, dtype=grad.dtype, device=grad.device) if w is None else w.to(grad.dtype)
  if combiner == "mean":
    den = torch.zeros(nseg, dtype=grad.dtype, device=grad.device).index_add_(0, seg, wj)
    scale = wj / den.index_select(0, seg)
  elif combiner == "sqrtn":
    den = torch.zeros(nseg, dtype=grad.dtype, device=grad.device).index_add_(0, seg, wj * wj).sqrt()
    scale = wj / den.index_select(0, seg)
  else:
    scale = wj
  vals = grad.reshape(nseg, -1).index_select(0, seg) * scale.unsqueeze(1)
  return vals.contiguous()


def pair(fa, fb, rounds=15, inner=10):
  """median microseconds per call of fa and of fb, alternating"""
  for f in (fa, fb):
    for _ in range(3): f()
  ta, tb = [], []
  for _ in range(rounds):
    for f, t in ((fa, ta), (fb, tb)):
      torch.cuda.synchronize()
      s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      s.record()
      for _ in range(inner): f()
      e.record(); torch.cuda.synchronize()
      t.append(s.elapsed_time(e) / inner * 1e3)
  return statistics.median(ta), statistics.median(tb)


def backward_lines():
  N = 1_000_000
  gen = torch.Generator(device=dev).manual_seed(1)
  h = ops.kv_variable([D])
  ops.init_kv_variable_v2(h, torch.randn(16, D, device=dev))
  for L in (1, 4, 16, 64):
    seg = (torch.arange(N, device=dev) // L).to(torch.int64)
    nseg = (N + L - 1) // L
    g = torch.randn(nseg, D, device=dev, generator=gen)
    a, b = glue_backward(g, seg, None, nseg, "mean"), ops.kv_variable_lookup_sparse_grad(h, g, seg, None, nseg, "mean")
    same = bool(torch.equal(a, b))      # (unweighted: the glue's index_add_ of ones is exact, so the two agree bit for bit)
    tg, tn = pair(lambda: glue_backward(g, seg, None, nseg, "mean"),
                  lambda: ops.kv_variable_lookup_sparse_grad(h, g, seg, None, nseg, "mean"))
    print("backward  segment length %2d: torch glue %7.1f us, kv_lookup_sparse_grad %7.1f us per 1M-id call (x%.2f)%s"
          % (L, tg, tn, tg / tn, "" if same else "  VALUES DIFFER"))


def batched_lines():
  T, n, L = 26, 2048, 4
  gen = torch.Generator(device=dev).manual_seed(2)
  hs = []
  for k in range(T):
    h = ops.kv_variable([D], capacity_hint=1 << 18)
    ops.kv_set_seed(h, k)
    ops.init_kv_variable_v2(h, torch.randn(1000, D, device=dev))
    hs.append(h)
  zipf = bench.Zipf(100_000, 1.2, dev)
  ids = [bench.splitmix64(zipf.sample(n, gen)) for _ in range(T)]
  seg = [(torch.arange(n, device=dev) // L).to(torch.int64) for _ in range(T)]
  nseg = [n // L] * T
  g = [torch.randn(n // L, D, device=dev, generator=gen) for _ in range(T)]

  def loop():
    for k in range(T):
      ops.kv_variable_lookup_sparse(hs[k], ids[k], seg[k], None, nseg[k], "mean")
    for k in range(T):
      ops.kv_variable_lookup_sparse_grad(hs[k], g[k], seg[k], None, nseg[k], "mean")

  def batched():
    ops.kv_multi_lookup_sparse(hs, ids, seg, None, nseg, "mean")
    ops.kv_multi_lookup_sparse_grad(hs, g, seg, None, nseg, "mean")

  tl, tb = pair(loop, batched, rounds=15, inner=5)
  print("batched   %d tables x %d ids x segment length %d, forward + backward: per-table loop %7.1f us, batched calls %7.1f us "
        "per step (x%.2f)" % (T, n, L, tl, tb, tl / tb))


backward_lines()
batched_lines()
