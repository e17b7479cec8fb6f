"""NumPy float32 restatement of the reference's group RectifiedAdam op, per unique id (what the op receives after
TF-core's de-duplication), in the kernel's operation order:

  group_radam  KvVariableGroupSparseApplyRectifiedAdamOp (tfplus kernels/training_ops.cc:6883-6936)

Every operation is one IEEE float32 rounding, like the kernels built with -ffp-contract=off.  alpha = sqrt(1 - beta2_power)
and c1 = 1 - beta1_power are computed once in float32, as the host does.  The nesterov form assigns through m_corr, a copy
of m's TensorMap, so it writes m itself.  The row norm is summed in NumPy's order (the kernel sums per lane,
then across lanes), so with l21 > 0 the var is good to a tolerance; with l21 = 0 the scale is exactly 1, the norm only
gates the update, and every output is the kernel's bit for bit.

Rows are [U, D] float32 arrays: x = var, g = the summed gradient rows; the slot row is [U, 5 D] = m | v | linear | vhat |
vamsgrad.
"""
import numpy as np

F = np.float32
CUTOFF = F(1e-20)


def host_scalars(beta1_power, beta2_power):
  """-> (alpha, c1) as kv_apply_group_rectified_adam computes them."""
  return np.sqrt(F(1) - F(beta2_power)).astype(F), F(1) - F(beta1_power)


def group_radam(x, slot, g, lr, beta1_power, beta2_power, beta1, beta2, epsilon, l1, l2, l21, r_t, tractable, amsgrad,
                use_nesterov, dtype=F):
  """-> (var, slot, updated) after one KvVariableGroupSparseApplyRectifiedAdam step; updated[i] is False where row i was
  blacklisted (its var reads as zeros).  dtype = np.float64: the same step in double precision (the hyperparameters
  still start from their float32 values) — what the reorder bound of the repeated-ids tests is evaluated with."""
  T = dtype
  x, slot, g = (np.asarray(t, T) for t in (x, slot, g))
  D = x.shape[1]
  m, v, z, vh, va = (slot[:, k * D:(k + 1) * D] for k in range(5))
  lr, b1, b2, eps, l1, l2, l21, r_t = (T(F(t)) for t in (lr, beta1, beta2, epsilon, l1, l2, l21, r_t))
  alpha, c1 = (T(t) for t in host_scalars(beta1_power, beta2_power))
  omb1, omb2 = T(F(1) - F(beta1)), T(F(1) - F(beta2))
  with np.errstate(all="ignore"):
    m1 = b1 * m + omb1 * g
    nv = b2 * v + omb2 * (g * g)
    if use_nesterov:
      m1 = g * omb1 + b1 * m1
    va1 = va
    if not tractable:
      rm = m1 / c1
      rv = np.broadcast_to(T(1) / lr, x.shape).astype(T)
    else:
      if amsgrad:
        va1 = np.maximum(nv, va)
      rm = (r_t * m1) / c1
      rv = (np.sqrt(va1 if amsgrad else nv) / alpha + eps) / lr
    z1 = z + (rm - (rv - vh) * x)
    u = np.maximum(np.minimum(z1, l1), -l1) - z1
    norm = np.sqrt((u * u).sum(axis=1, dtype=T)).astype(T)[:, None]
    thr = l21 * np.sqrt(T(D)).astype(T)
    upd = norm > thr
    scale = T(1) - thr / norm
    x1 = np.where(upd, (u * scale) / (rv + T(2) * l2), T(0))
  return x1.astype(T), np.concatenate([m1, nv, z1, rv, va1], axis=1).astype(T), upd[:, 0]


def row_norms(x, slot, g, *hp):
  """|clamp(linear', -l1, l1) - linear'|_2 per row in float64 on the float32 step's linear': what the op compares with
  l21 sqrt(D).  It does not depend on l21."""
  x = np.asarray(x, F)
  D = x.shape[1]
  l1 = float(F(hp[6]))
  z1 = group_radam(x, slot, g, *hp)[1][:, 2 * D:3 * D].astype(np.float64)
  u = np.clip(z1, -l1, l1) - z1
  return np.sqrt((u * u).sum(axis=1))


def norm_over_threshold(x, slot, g, *hp):
  """norm / (l21 sqrt(D)) per row in float64 (inf when l21 = 0): how far each key is from the blacklist decision."""
  D = np.asarray(x).shape[1]
  with np.errstate(all="ignore"):
    return row_norms(x, slot, g, *hp) / (float(F(hp[8])) * np.sqrt(D))


def under_threshold(rows):
  """UpdateUnderThreshold: every |element| below the cutoff (kv_variable_interface.h:55)."""
  return np.all(np.abs(rows) < CUTOFF, axis=1)


def composite_radam(x, m, v, vmax, g, lr_t, beta1_power, beta2_power, beta1, beta2, epsilon, r_t, tractable, amsgrad,
                    use_nesterov):
  """One step of the composite RectifiedAdamOptimizer (training/rectified_adam.py) without weight decay, in float32 and
  in its operation order -> (var, m, v, vmax)."""
  x, m, v, vmax, g = (np.asarray(t, F) for t in (x, m, v, vmax, g))
  lr_t, b1p, b2p, b1, b2, eps, r_t = (F(t) for t in (lr_t, beta1_power, beta2_power, beta1, beta2, epsilon, r_t))
  m1 = b1 * m + g * (F(1) - b1)
  mc = g * (F(1) - b1) + b1 * m1 if use_nesterov else m1
  m_corr = mc / (F(1) - b1p)
  v1 = b2 * v + (g * g) * (F(1) - b2)
  if amsgrad:
    vmax = np.maximum(v1, vmax)
  v_corr = np.sqrt((vmax if amsgrad else v1) / (F(1) - b2p))
  upd = r_t * m_corr / (v_corr + eps) if tractable else m_corr
  return (x - upd * lr_t).astype(F), m1.astype(F), v1.astype(F), vmax


# Roundings that separate one fused step from one composite step, per element, in units of 2^-24 (half an ulp, relative):
#   on the var's scale — the fused op carries linear = -vhat x and forms x' = -(linear + rm - (rv - vhat) x) / rv:
#     the stored linear is -vhat x only to the rounding of the division that produced x (1), rv - vhat (1), times x (1),
#     rm - that (1): four roundings of magnitude up to max(rv, vhat) |x|, i.e. max(rv, vhat) / rv on x's scale — the
#     cancellation of the step where rv jumps from 1 / lr to sqrt(v) / (alpha lr); the sum linear + ... (1), the division by
#     rv (1), the composite's x - upd (1): three of magnitude |x'| <= |x| + |dx|;
#   on the step's scale |dx| = |rm / rv|: fused rm (2: r_t m, / c1) and its part in rm - ... (1), rv (4: sqrt, / alpha,
#     + eps, / lr); composite m_corr, v / (1 - b2p), sqrt, + eps, r_t m_corr, the division, times lr (7).
# 4 R + 3 <= 7 R on |x| with R = max(rv, vhat) / rv >= 1, and 3 + 2 + 1 + 4 + 7 = 17 on |dx|: 17 covers both.
COMPOSITE_ROUNDINGS = 17


def composite_step_tolerance(x, x_new, rv, vhat):
  """How far one fused step may move away from one composite step (float64 array): COMPOSITE_ROUNDINGS 2^-24
  (max(rv, vhat) |x| / rv + |x_new - x|).  The steps' tolerances add up: the step is x - rm / rv with rm, rv independent of
  x, so an earlier difference is carried, not amplified."""
  x, x_new, rv, vhat = (np.asarray(t, np.float64) for t in (x, x_new, rv, vhat))
  return COMPOSITE_ROUNDINGS * 2.0 ** -24 * (np.maximum(rv, vhat) * np.abs(x) / rv + np.abs(x_new - x))
