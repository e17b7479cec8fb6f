"""Group AMSGrad / group AdaBelief on de-duplicated ids, restated once in NumPy from the reference's row math
(kernels/training_ops.cc:1742-1775, 3189-3222): the checker of tests/test_gpu_group_adam4.py."""
import numpy as np

HP_NAMES = ("lr", "beta1_power", "beta2_power", "beta1", "beta2", "epsilon", "l1", "l2", "l21")


def step(variant, x, slot, g, hp, dt=np.float64):
  """One step on rows: x [n, D] the var, slot [n, 4 D] = m | v | linear | acc, g the summed gradient, hp in HP_NAMES' order
  (the op's float32 scalars).  Every operation is one rounding of dtype dt, in the reference's order.
  -> (new var, new slot rows, upd: the row norm passed l21 sqrt(D) — else the var is blacklisted and zero —, the row norms)"""
  lr, b1p, b2p, b1, b2, eps, l1, l2, l21 = [dt(np.float32(v)) for v in hp]
  D, one = g.shape[1], dt(1)
  x, g, m, v, z, acc = [a.astype(dt) for a in (x, g, slot[:, :D], slot[:, D:2 * D], slot[:, 2 * D:3 * D], slot[:, 3 * D:])]
  m1 = b1 * m + (one - b1) * g
  d = g - m1 if variant == "adabelief" else g
  v1 = b2 * v + (one - b2) * (d * d)
  vc = v1 / (one - b2p)
  acc1 = vc if variant == "adabelief" else np.maximum(acc, vc)
  z1 = z + (m1 / (one - b1p) - ((np.sqrt(acc1) - np.sqrt(acc)) / lr) * x)
  u = np.minimum(np.maximum(z1, -l1), l1) - z1
  norm = np.sqrt((u * u).sum(axis=1, dtype=dt))
  thr = l21 * np.sqrt(dt(D))
  upd = norm > thr
  with np.errstate(all="ignore"):
    x1 = (u * (one - thr / norm)[:, None]) / ((np.sqrt(acc1) + eps) / lr + dt(2) * l2)
  return np.where(upd[:, None], x1, dt(0)), np.concatenate([m1, v1, z1, acc1], axis=1), upd, norm
