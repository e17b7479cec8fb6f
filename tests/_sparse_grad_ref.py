"""float32 restatement of kv_lookup_sparse_grad (include/kvhip.h): the yardstick of the GPU tests, checked on the CPU
against torch autograd by tests/test_sparse_grad_ref.py.

  values[j, :] = scale_j * seg_grad[seg[j], :]
  scale_j = w_j (sum) | w_j / sum_s(w) (mean) | w_j / sqrtf(sum_s(w^2)) (sqrtn);  w_j = 1 without weights

A segment's denominator is summed in float32 from +0 in position order — an explicit loop: np.sum and np.add.reduceat
sum pairwise, another rounding sequence — the scale is one float32 division, each element one float32 multiply."""
import numpy as np

COMBINERS = ("sum", "mean", "sqrtn")


def denominators(seg, weights, nseg, combiner):
  """[nseg] float32: sum_s(w) (mean) or sqrtf(sum_s(w^2)) (sqrtn), position order; w = 1 without weights."""
  assert combiner in ("mean", "sqrtn")
  w = np.ones(len(seg), np.float32) if weights is None else np.asarray(weights, np.float32)
  acc = [np.float32(0.0)] * nseg
  for j, s in enumerate(np.asarray(seg).tolist()):
    wj = w[j]
    acc[s] = np.float32(acc[s] + (wj if combiner == "mean" else np.float32(wj * wj)))
  den = np.asarray(acc, np.float32).reshape(nseg)
  return den if combiner == "mean" else np.sqrt(den, dtype=np.float32)


def scales(seg, weights, nseg, combiner):
  """[n] float32 scale of every position."""
  assert combiner in COMBINERS
  seg = np.asarray(seg).astype(np.int64)
  w = np.ones(len(seg), np.float32) if weights is None else np.asarray(weights, np.float32)
  if combiner == "sum":
    return w.copy()
  den = denominators(seg, weights, nseg, combiner)
  with np.errstate(divide="ignore", invalid="ignore"):
    return (w / den[seg]).astype(np.float32)


def lookup_sparse_grad(seg_grad, seg, weights, nseg, combiner, scale=None):
  """[n, dim] float32 values; `scale`: scales(...) computed before (it does not depend on the dim)."""
  seg = np.asarray(seg).astype(np.int64)
  g = np.asarray(seg_grad, np.float32).reshape(nseg, -1)
  sc = scales(seg, weights, nseg, combiner) if scale is None else scale
  with np.errstate(invalid="ignore", over="ignore"):
    return (g[seg] * sc[:, None]).astype(np.float32)


def same_bits(a, b, nan_ok=False):
  """a and b hold the same float32 bit patterns; nan_ok: a NaN matches a NaN whatever its payload (the zero-denominator case)."""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  if a.shape != b.shape:
    return False
  if not nan_ok:
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))
  na, nb = np.isnan(a), np.isnan(b)
  return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
