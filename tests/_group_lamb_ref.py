"""Group LAMB on de-duplicated ids, restated once in NumPy from the reference's row math (kernels/training_ops.cc:3618-3661,
COMPUTE_LAMB): the checker of tests/test_gpu_group_lamb.py."""
import numpy as np

HP_NAMES = ("lr", "beta1_power", "beta2_power", "beta1", "beta2", "epsilon", "l1", "l2", "l21")


def step(x, slot, g, hp, dt=np.float64, sequential=False):
  """One step on rows: x [n, D] the var, slot [n, 4 D] = m | v | linear | accum, g the summed gradient, hp in HP_NAMES' order
  (the op's float32 scalars).  Every operation is one rounding of dtype dt, in the reference's order; the three row sums are
  NumPy's pairwise sum, or one running sum left to right with sequential=True.
  -> (new var, new slot rows, upd: the row norm passed l21 sqrt(D) — else the var is blacklisted and zero —, the l21 row norms,
  the trust ratios)"""
  lr, b1p, b2p, b1, b2, eps, l1, l2, l21 = [dt(np.float32(v)) for v in hp]
  D, one = g.shape[1], dt(1)
  total = (lambda w: np.cumsum(w, axis=1, dtype=dt)[:, -1]) if sequential else (lambda w: w.sum(axis=1, dtype=dt))
  x, g, m, v, z, acc = [a.astype(dt) for a in (x, g, slot[:, :D], slot[:, D:2 * D], slot[:, 2 * D:3 * D], slot[:, 3 * D:])]
  m1 = b1 * m + (one - b1) * g
  v1 = b2 * v + (one - b2) * (g * g)
  nm, na = m1 / (one - b1p), v1 / (one - b2p)
  sq = np.sqrt(na)
  r = nm / (sq + eps)
  rn, xn = np.sqrt(total(r * r)), np.sqrt(total(x * x))
  ratio = np.where((rn > 0) & (xn > 0), xn / (rn + dt(np.float32(1e-8))), one)
  z1 = z + (nm * ratio[:, None] - ((sq - np.sqrt(acc)) / lr) * x)
  u = np.minimum(np.maximum(z1, -l1), l1) - z1
  norm = np.sqrt(total(u * u))
  thr = l21 * np.sqrt(dt(D))
  upd = norm > thr
  with np.errstate(all="ignore"):
    x1 = (u * (one - thr / norm)[:, None]) / ((sq + eps) / lr + dt(2) * l2)
  return np.where(upd[:, None], x1, dt(0)), np.concatenate([m1, v1, z1, na], axis=1), upd, norm, ratio
