"""Reference value and error bound of kv_lookup_sparse_zeros (include/kvhip.h): a float64 combine over the rows that
kv_variable_gather_or_zeros_v2 returns for the same ids, and the sequential-summation bound of the float32 kernel.

Clamping as the op documents it: negative segment ids count towards segment 0, ids >= num_segments towards none.
"""
import numpy as np

EPS = 2.0 ** -24      # unit roundoff of float32


def combine(rows, seg, w, nseg, combiner):
  """(want, tol), both [nseg, D] float64.  rows [n, D] float32 as gathered, seg [n] ascending, w [n] float32 or None.
  want[s] = sum_j w_j x_j / den, den = 1 (sum), sum w (mean), sqrt(sum w^2) (sqrtn); an empty segment is a zero row
  without weights and 0/0 = NaN with them (mean / sqrtn).
  tol[s] = (2 L + 4) 2^-24 sum_j |w_j x_j| / |den| for a segment of L positions: one rounding per product, one per
  addition, the denominator's own sum, and the division."""
  rows = np.asarray(rows, np.float64)
  seg = np.asarray(seg, np.int64)
  n, D = rows.shape
  ww = np.ones(n, np.float64) if w is None else np.asarray(w, np.float32).astype(np.float64)
  s = np.maximum(seg, 0)
  keep = s < nseg
  s, x, ww = s[keep], rows[keep], ww[keep]
  num = np.zeros((nseg, D))
  mag = np.zeros((nseg, D))
  np.add.at(num, s, x * ww[:, None])
  np.add.at(mag, s, np.abs(x * ww[:, None]))
  L = np.bincount(s, minlength=nseg).astype(np.float64)
  if combiner == "sum":
    den = np.ones(nseg)
  elif combiner == "mean":
    den = np.bincount(s, weights=ww, minlength=nseg)
  else:
    den = np.sqrt(np.bincount(s, weights=ww * ww, minlength=nseg))
  empty = L == 0
  with np.errstate(invalid="ignore", divide="ignore"):
    want = num / den[:, None]
    tol = (2 * L + 4)[:, None] * EPS * mag / np.abs(den)[:, None]
  if combiner != "sum":
    want[empty] = 0.0 if w is None else np.nan
  tol[empty] = 0.0
  return want, tol


def check(got, want, tol, what=""):
  """NaN positions match; every other element within its own bound."""
  got = np.asarray(got, np.float64)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
  err = np.abs(np.where(nan, 0.0, got - want))
  bad = err > np.where(nan, 0.0, tol)
  assert not bad.any(), "%s: %d elements outside the bound, worst %g x the bound" % (
      what, int(bad.sum()), float((err[bad] / np.maximum(tol[bad], 1e-300)).max()))
