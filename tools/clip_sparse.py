"""embedding_lookup_sparse with max_norm on one table: the fused clip ops against the unclipped fused ops and the torch chain
they replace.  Two shapes — DCN-like training (2048 segments) and the large serving shape of tools/serving_sparse.py (50 000
segments) — 1-8 ids per segment, Zipf(1.2) ids over filled tables, weighted mean, dims 64 and 128, max_norm = the middle of the
looked-up rows' distinct norms (about half the rows are clipped).  Timed per direction in windows of
about a quarter of a second, the three paths alternating, best of five rounds, with the rounds' spread:
  (a) the fused clip op         kv_lookup_sparse_clip / kv_lookup_sparse_clip_grad / kv_lookup_sparse_zeros_clip
  (b) the unclipped fused op    kv_lookup_sparse / kv_lookup_sparse_grad / kv_lookup_sparse_zeros on the same call
  (c) the torch chain           unique -> gather -> norm, clamp, multiply -> index_select -> multiply -> index_add x 2 -> divide
                                (and the host sync for the segment count); its backward is torch.autograd through it
Prints the three times and the ratios (c) / (a) and (a) / (b).  python tools/clip_sparse.py [other.so]"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(5)


def chain(h, ids, seg, w, c, training):
  """-> (out, the looked-up unique rows: the leaf the chain's backward ends at)"""
  nseg = int(seg.max().item()) + 1
  uniq, idx = torch.unique(ids, return_inverse=True)
  rows = (ops.kv_variable_gather_or_insert_v2 if training else ops.kv_variable_gather_or_zeros_v2)(h, uniq).requires_grad_(training)
  norm = torch.linalg.vector_norm(rows, dim=-1, keepdim=True)
  emb = (rows * torch.clamp(c / torch.clamp(norm, min=1e-30), max=1.0)).index_select(0, idx)
  wts = w.reshape(-1, 1)
  summed = torch.zeros((nseg, emb.shape[1]), device=dev).index_add(0, seg, emb * wts)
  return summed / torch.zeros((nseg, 1), device=dev).index_add(0, seg, wts), rows


WINDOW = 0.25   # seconds per timed window: a call of tens of microseconds is repeated thousands of times


def timed(fn, reps):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(reps): fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e6


def race(title, runs):
  reps = {name: max(20, int(WINDOW * 1e6 / timed(fn, 20))) for name, fn in runs if timed(fn, 5)}   # (warm-up, then the window's length)
  t = {name: [] for name, _ in runs}
  for rnd in range(5):                                   # the paths alternate: five rounds each
    for name, fn in runs:
      t[name].append(timed(fn, reps[name]))
  a, b, c = (min(t[name]) for name, _ in runs)
  print("  %-18s (a) %7.1f us (b) %7.1f us (c) %7.1f us  (c)/(a) %5.1fx  (a)/(b) %4.2fx  spread of the rounds (max/min - 1): %s"
        % (title, a, b, c, c / a, a / b, "  ".join("(%s) %.1f%%" % (name, 100 * (max(v) / min(v) - 1)) for name, v in t.items())))


for nseg, keys in ((2048, 200_000), (50_000, 2_000_000)):
  z = bench.Zipf(keys, 1.2, dev)
  for D in (64, 128):
    h = ops.kv_variable([D], capacity_hint=keys + 1024)
    ops.init_kv_variable_v2(h, torch.randn(256, D, device=dev))
    for j in range(0, keys, 1 << 20):
      ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), keys), device=dev))
    lens = torch.randint(1, 9, (nseg,), device=dev, generator=gen)
    seg = torch.repeat_interleave(torch.arange(nseg, device=dev), lens)
    ids = z.sample(seg.numel(), gen) - 1
    w = torch.rand(seg.numel(), device=dev, generator=gen) + 0.5
    g = torch.randn(nseg, D, device=dev, generator=gen)
    looked = ops.kv_variable_gather_or_zeros_v2(h, ids)
    norms = torch.unique(torch.linalg.vector_norm(looked, dim=-1))
    c = float((norms[norms.numel() // 2 - 1] + norms[norms.numel() // 2]) / 2)   # between two rows' norms: the clip's kink is at none
    print("%d segments, %d ids (1-8 per segment), Zipf(1.2) over %d keys, dim %d, max_norm %.3f: %.0f%% of the looked-up rows clipped"
          % (nseg, ids.numel(), keys, D, c, 100.0 * float((torch.linalg.vector_norm(looked, dim=-1) > c).float().mean())))
    # the paths compute the same thing
    out_a, saved = ops.kv_variable_lookup_sparse_clip(h, ids, seg, w, nseg, "mean", False, c)
    out_c, leaf = chain(h, ids, seg, w, c, True)
    torch.testing.assert_close(out_a, out_c.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ops.kv_variable_lookup_sparse_zeros_clip(h, ids, seg, w, nseg, "mean", c), out_a, rtol=1e-5, atol=1e-6)
    vals = ops.kv_variable_lookup_sparse_clip_grad(h, g, seg, w, saved, nseg, "mean", c)
    uniq, idx = torch.unique(ids, return_inverse=True)
    (leaf_grad,) = torch.autograd.grad(out_c, leaf, g, retain_graph=True)
    # (a hot key's gradient is a float32 sum of tens of thousands of rows in the chain: held against the sum of magnitudes)
    per_key = lambda v: torch.zeros_like(leaf_grad, dtype=torch.float64).index_add(0, idx, v.double())
    assert bool(((per_key(vals) - leaf_grad).abs() <= 1e-4 * per_key(vals.abs()) + 1e-5).all())
    race("training forward", (("a", lambda: ops.kv_variable_lookup_sparse_clip(h, ids, seg, w, nseg, "mean", False, c)),
                              ("b", lambda: ops.kv_variable_lookup_sparse(h, ids, seg, w, nseg, "mean", False)),
                              ("c", lambda: chain(h, ids, seg, w, c, True))))
    race("training backward", (("a", lambda: ops.kv_variable_lookup_sparse_clip_grad(h, g, seg, w, saved, nseg, "mean", c)),
                               ("b", lambda: ops.kv_variable_lookup_sparse_grad(h, g, seg, w, nseg, "mean")),
                               ("c", lambda: torch.autograd.grad(out_c, leaf, g, retain_graph=True))))
    race("serving", (("a", lambda: ops.kv_variable_lookup_sparse_zeros_clip(h, ids, seg, w, nseg, "mean", c)),
                     ("b", lambda: ops.kv_variable_lookup_sparse_zeros(h, ids, seg, w, nseg, "mean")),
                     ("c", lambda: chain(h, ids, seg, w, c, False))))
    del h, out_c, leaf
