"""Group Momentum / group Adadelta on de-duplicated ids, restated once in NumPy from the reference's row math
(kernels/training_ops.cc:2451-2482 COMPUTE_MOMENTUM, 2193-2226 COMPUTE_ADADELTA): the checker of tests/test_gpu_group_acc3.py."""
import numpy as np

VARIANTS = ("momentum", "nesterov", "adadelta")      # the codes 0, 1, 2 of optimizer 11's hp[6]
HP_NAMES = ("lr", "decay", "epsilon", "l1", "l2", "l21")   # decay = momentum or rho; Momentum ignores epsilon


def step(variant, x, slot, g, hp, dtype=np.float64, sequential=False):
  """One step on rows: x [n, D] the var, slot [n, 3 D] = accum | linear | m (Momentum) or accum | linear | accum_update
  (Adadelta), g the summed gradient, hp in HP_NAMES' order (the op's float32 scalars).  Every operation is one rounding of
  dtype, in the reference's order; the row sum is NumPy's pairwise sum, or one running sum left to right with sequential=True.
  Two aliasing facts of the source: nesterov's second update writes through into m (the stored m is the twice-updated one),
  and Adadelta's accum_update divides by new_accum evaluated AFTER accum = new_accum (the decay applied a second time).
  -> (new var, new slot rows, upd: the row norm passed l21 sqrt(D) — else the var is blacklisted and zero —, the row norms)"""
  dt = dtype
  lr, dec, eps, l1, l2, l21 = [dt(np.float32(v)) for v in hp]
  D, one = g.shape[1], dt(1)
  x, g, acc, z, third = [a.astype(dt) for a in (x, g, slot[:, :D], slot[:, D:2 * D], slot[:, 2 * D:])]
  if variant == "adadelta":
    t = (one - dec) * (g * g)
    na = acc * dec + t
    M = np.sqrt(third + eps) * g
    y = np.sqrt(na + eps) / lr + dt(2) * l2
    na2 = na * dec + t
    third1 = third * dec + ((one - dec) * (M * M)) / (na2 + eps)
  else:
    M = third * dec + g
    if variant == "nesterov":
      M = M * dec + g
    na, third1 = np.ones_like(acc), M
    y = one / lr + dt(2) * l2
  z1 = z + (M - ((np.sqrt(na) - np.sqrt(acc)) / lr) * x)
  u = np.minimum(np.maximum(z1, -l1), l1) - z1
  w = u * u
  norm = np.sqrt(np.cumsum(w, axis=1, dtype=dt)[:, -1] if sequential else w.sum(axis=1, dtype=dt))
  thr = l21 * np.sqrt(dt(D))
  upd = norm > thr
  with np.errstate(all="ignore"):
    x1 = (u * (one - thr / norm)[:, None]) / y
  return np.where(upd[:, None], x1, dt(0)), np.concatenate([na, z1, third1], axis=1), upd, norm
