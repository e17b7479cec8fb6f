"""NumPy float32 restatement of ONE plain-Adam step (kvhip.h kv_apply_adam) on a dict-of-rows table model: the definition
the GPU tests compare against.

The reference has no op for the step: its AdamOptimizer composes it (tfplus python/training/adam.py:93-163) from TF-core's
de-duplication and three generic table ops.  What is restated here is that chain:

  unique ids in order of first occurrence, a repeated id's gradient rows added one by one in occurrence order;
  GatherOrInsert on the slot table m_v (kv_variable.h:263-380), count 1 per distinct id;
  m = beta1 m + g (1 - beta1);  v = beta2 v + (g g) (1 - beta2);  ScatterUpdate(m_v, [m | v]) (:616-734);
  ScatterSub(var, (lr_t m) / (epsilon + sqrt(v))),  lr_t = (lr sqrt(1 - beta2_power)) / (1 - beta1_power).

Every operation is one IEEE float32 rounding, like the kernels built with -ffp-contract=off.  lr_t, 1 - beta1 and
1 - beta2 are computed once in float32, as the host does.

Bookkeeping (the chain's, not the group optimizers'):
  slot table  row found, or inserted with the init rule and frequency word day << 16 | 1; an existing row's word gets one hit
              and the day; a blacklisted row reads as zeros and is left unwritten; flags from the row written;
  var table   row found, or inserted with the init rule and frequency word 1; an existing row's word is untouched; no
              enter-threshold filter; a blacklisted row is neither written nor un-blacklisted; flags from the row written.
"""
import numpy as np

import _kv_model
from _kv_model import CUTOFF, F, M64, Row, Table, _mix64, dedup_sum  # noqa: F401  (the table model grew into tests/_kv_model.py)


def host_scalars(lr, beta1_power, beta2_power, beta1, beta2):
  """-> (lr_t, 1 - beta1, 1 - beta2) as kv_apply_adam computes them (fp32, in this order)."""
  lr_t = F(F(lr) * np.sqrt(F(1) - F(beta2_power))) / F(F(1) - F(beta1_power))
  return F(lr_t), F(F(1) - F(beta1)), F(F(1) - F(beta2))


def row_math(x, m, v, g, lr, beta1_power, beta2_power, beta1, beta2, epsilon):
  """The arithmetic on arrays of rows -> (var, m, v), one float32 rounding per operation."""
  x, m, v, g = (np.asarray(t, F) for t in (x, m, v, g))
  lr_t, omb1, omb2 = host_scalars(lr, beta1_power, beta2_power, beta1, beta2)
  b1, b2, eps = F(beta1), F(beta2), F(epsilon)
  m1 = b1 * m + g * omb1
  v1 = b2 * v + (g * g) * omb2
  x1 = x - (lr_t * m1) / (eps + np.sqrt(v1))
  return x1.astype(F), m1.astype(F), v1.astype(F)


def adam_step(var, slot, ids, grad, lr, beta1_power, beta2_power, beta1, beta2, epsilon):
  """One step on the two Table models, in place.  -> the unique ids in first-occurrence order.  The bookkeeping is
  tests/_kv_model.py apply_step's "adam" (the chain's rules, stated once there); the arithmetic is row_math above."""
  assert slot.dim == 2 * var.dim
  uniq, sums = dedup_sum(ids, grad)
  _kv_model.apply_step("adam", var, [slot], uniq, sums, (lr, beta1_power, beta2_power, beta1, beta2, epsilon))
  return uniq
