"""NumPy float32 restatement of the reference's FTRL-V2 ops, per unique id (what the ops receive after TF-core's
de-duplication), in the reference kernels' operation order:

  ftrl_v2        KvVariableSparseApplyFtrlOp, has_l2_shrinkage (tfplus kernels/training_ops.cc:457-484)
  group_ftrl_v2  KvVariableGroupSparseApplyFtrlOp, has_l2_shrinkage (:977-1019)

Both evaluate Eigen's lazy expressions as the reference does: grad_to_use = grad + 2 l2_shrinkage var is re-read with the
UPDATED var by the final `accum += grad_to_use.square()` (twice in the group op).  Every operation is one IEEE float32
rounding, like the kernels built with -ffp-contract=off; the group op's row norm is summed in NumPy's order (the
reference sums in Eigen's), so it is good to a tolerance, not bit for bit.  On the group op's blacklist branch the
accum update keeps the pre-blacklist var.

Rows are [U, D] float32 arrays: x = var, a = accum, z = linear, g = the summed gradient rows.
"""
import numpy as np

F = np.float32
CUTOFF = F(1e-20)


def _hp(lr, l1, l2, l2s, lr_power):
  return F(lr), F(l1), F(2) * F(l2), F(2) * F(l2s), F(lr_power)


def _p(v, lrp):
  with np.errstate(all="ignore"):
    return np.sqrt(v) if lrp == F(-0.5) else np.power(v, -lrp).astype(F)


def _linear(x, a, z, g, lr, two_l2s, lrp):
  gs = g + two_l2s * x
  na = a + gs * gs
  pn, po = _p(na, lrp), _p(a, lrp)
  return pn, z + (gs - ((pn - po) / lr) * x)


def ftrl_v2(x, a, z, g, lr, l1, l2, l2_shrinkage, lr_power):
  """-> (var, accum, linear) after one KvVariableSparseApplyFtrlV2 step."""
  x, a, z, g = (np.asarray(t, F) for t in (x, a, z, g))
  lr, l1, two_l2, two_l2s, lrp = _hp(lr, l1, l2, l2_shrinkage, lr_power)
  with np.errstate(all="ignore"):
    pn, z1 = _linear(x, a, z, g, lr, two_l2s, lrp)
    adj = np.maximum(np.minimum(z1, l1), -l1)
    x1 = (adj - z1) / (pn / lr + two_l2)
    gs2 = g + two_l2s * x1
    a1 = a + gs2 * gs2
  return x1.astype(F), a1.astype(F), z1.astype(F)


def group_ftrl_v2(x, a, z, g, lr, l1, l2, l2_shrinkage, lr_power, dtype=F):
  """-> (var, accum, linear, updated) after one KvVariableGroupSparseApplyFtrlV2 step; updated[i] is False where row i
  was blacklisted (its var reads as zeros).  dtype = np.float64: the same step in double precision (the hyperparameters
  still start from their float32 values)."""
  T = dtype
  x, a, z, g = (np.asarray(t, T) for t in (x, a, z, g))
  lr, l1, two_l2, two_l2s, lrp = (T(v) for v in _hp(lr, l1, l2, l2_shrinkage, lr_power))
  with np.errstate(all="ignore"):
    gs = g + two_l2s * x
    na = a + gs * gs
    pn, po = (np.sqrt(v) if lrp == T(-0.5) else np.power(v, -lrp).astype(T) for v in (na, a))
    z1 = z + (gs - ((pn - po) / lr) * x)
    norm = np.sqrt((z1 * z1).sum(axis=1, dtype=T)).astype(T)[:, None]
    upd = norm > l1
    coef = (l1 - norm) / ((pn / lr + two_l2) * norm)
    x1 = np.where(upd, coef * z1, T(0))
    xa = np.where(upd, x1, x)
    gs2 = g + two_l2s * xa
    g2 = gs2 * gs2
    a1 = (a + g2) + g2
  return x1.astype(T), a1.astype(T), z1.astype(T), upd[:, 0]


def under_threshold(rows):
  """UpdateUnderThreshold: every |element| below the cutoff (kv_variable_interface.h:55)."""
  return np.all(np.abs(rows) < CUTOFF, axis=1)
