"""The yardstick of the sparse lookup's backward (tests/_sparse_grad_ref.py) against torch autograd on the CPU, through the
definition of embedding_lookup_sparse itself: gather -> * w -> index_add segment sum -> divide.  No code under test runs.

Weighted inputs (and unweighted sqrtn) agree to rtol 1e-6: autograd divides the segment's gradient by the denominator and
multiplies by w_j, the restatement multiplies by w_j / den — two roundings each, in another order.  Unweighted `sum` is
exact for any segment lengths.  Unweighted `mean` is exact where it can be: autograd computes g / len, the restatement
g * (1 / len), and the two are the same float32 for every g exactly when 1 / len is a float32, so the exact comparison
runs over power-of-two segment lengths (1, 2, 4, 8, 16 and empty segments); ragged lengths are held to rtol 1e-6 with the
rest."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sparse_grad_ref as R  # noqa: E402


def _autograd(rows, seg, w, nseg, combiner, G):
  x = torch.tensor(rows, requires_grad=True)
  segt = torch.as_tensor(seg, dtype=torch.int64)
  wt = torch.ones(len(seg)) if w is None else torch.tensor(w)
  summed = torch.zeros(nseg, rows.shape[1]).index_add(0, segt, x * wt[:, None])
  if combiner == "sum":
    out = summed
  elif combiner == "mean":
    out = summed / torch.zeros(nseg).index_add(0, segt, wt)[:, None]
  else:
    out = summed / torch.sqrt(torch.zeros(nseg).index_add(0, segt, wt * wt))[:, None]
  out.backward(torch.tensor(G))
  return x.grad.numpy()


def _case(lens, D, weighted, seed):
  rng = np.random.default_rng(seed)
  lens = np.asarray(lens)
  seg = np.repeat(np.arange(lens.size), lens)
  rows = rng.standard_normal((seg.size, D)).astype(np.float32)
  G = rng.standard_normal((lens.size, D)).astype(np.float32)
  w = rng.uniform(0.5, 1.5, seg.size).astype(np.float32) if weighted else None
  return seg, rows, G, w


RAGGED = [0, 0, 1, 5, 7, 600, 0, 3, 2, 9, 1, 1, 0, 33, 0]
POW2 = [0, 1, 2, 4, 0, 8, 16, 1, 4, 0]


@pytest.mark.parametrize("combiner", R.COMBINERS)
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_matches_autograd(combiner, weighted):
  seg, rows, G, w = _case(RAGGED, 12, weighted, 3)
  got = R.lookup_sparse_grad(G, seg, w, len(RAGGED), combiner)
  want = _autograd(rows, seg, w, len(RAGGED), combiner, G)
  assert got.dtype == np.float32 and got.shape == rows.shape
  np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("combiner,lens", [("sum", RAGGED), ("sum", POW2), ("mean", POW2)])
def test_restatement_unweighted_is_exact(combiner, lens):
  seg, rows, G, _ = _case(lens, 12, False, 5)
  got = R.lookup_sparse_grad(G, seg, None, len(lens), combiner)
  want = _autograd(rows, seg, None, len(lens), combiner, G)
  assert R.same_bits(got, want)


def test_denominators_are_summed_in_position_order():
  """Sequential float32 sums, not pairwise ones: a segment where the two differ."""
  w = np.array([1.0] + [2.0 ** -24] * 4, np.float32)   # sequentially every small term is lost; pairwise two of them survive
  den = R.denominators(np.zeros(5, np.int64), w, 1, "mean")
  assert den[0] == np.float32(1.0)
  assert np.sum(w[1:], dtype=np.float32) + np.float32(1.0) != np.float32(1.0)
  # unweighted: the segment's length, exactly
  lens = [3, 0, 600]
  seg = np.repeat(np.arange(3), lens)
  np.testing.assert_array_equal(R.denominators(seg, None, 3, "mean"), np.array(lens, np.float32))
  np.testing.assert_array_equal(R.denominators(seg, None, 3, "sqrtn"), np.sqrt(np.array(lens, np.float32)))


def test_zero_denominator_is_ieee():
  seg = np.array([0, 0, 1], np.int64)
  w = np.array([1.0, -1.0, 2.0], np.float32)
  G = np.array([[3.0, 0.0], [1.0, 1.0]], np.float32)
  v = R.lookup_sparse_grad(G, seg, w, 2, "mean")
  assert np.isposinf(v[0, 0]) and np.isnan(v[0, 1]) and np.isneginf(v[1, 0]) and np.isnan(v[1, 1])
  np.testing.assert_array_equal(v[2], [1.0, 1.0])
  assert R.same_bits(v, v.copy(), nan_ok=True) and not R.same_bits(v, np.zeros_like(v), nan_ok=True)
