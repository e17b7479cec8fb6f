"""FtrlOptimizer / GroupFtrlOptimizer — tf.compat.v1.train.FtrlOptimizer's constructor over the KvVariable ops
KvVariableSparseApplyFtrlV2 and KvVariableGroupSparseApplyFtrlV2 (ops/training_ops.cc:103-133): slots "accum"
(initial_accumulator_value, default 0.1) and "linear" (zeros), as SparseGroupFtrlOptimizer.  The op receives TF-core's
*adjusted* l2 = l2 + beta / (2 lr) (FtrlOptimizer._prepare)."""
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.optimizer import Optimizer


class FtrlOptimizer(Optimizer):
  """Per-coordinate FTRL-Proximal on KvVariables (kvhip.h kv_apply_ftrl_v2)."""

  _apply_op = staticmethod(gen_kv_variable_ops.kv_variable_sparse_apply_ftrl_v2)

  def __init__(self, learning_rate, learning_rate_power=-0.5, initial_accumulator_value=0.1,
               l1_regularization_strength=0.0, l2_regularization_strength=0.0, use_locking=False, name="Ftrl",
               accum_name=None, linear_name=None, l2_shrinkage_regularization_strength=0.0, beta=None):
    super(FtrlOptimizer, self).__init__(use_locking, name)
    if initial_accumulator_value < 0.0:
      raise ValueError("initial_accumulator_value %f needs to be positive or zero" % initial_accumulator_value)
    if learning_rate_power > 0.0:
      raise ValueError("learning_rate_power %f needs to be negative or zero" % learning_rate_power)
    if l1_regularization_strength < 0.0:
      raise ValueError("l1_regularization_strength %f needs to be positive or zero" % l1_regularization_strength)
    if l2_regularization_strength < 0.0:
      raise ValueError("l2_regularization_strength %f needs to be positive or zero" % l2_regularization_strength)
    if l2_shrinkage_regularization_strength < 0.0:
      raise ValueError("l2_shrinkage_regularization_strength %f needs to be positive or zero" %
                       l2_shrinkage_regularization_strength)
    self._learning_rate = learning_rate
    self._learning_rate_power = learning_rate_power
    self._initial_accumulator_value = initial_accumulator_value
    self._l1, self._l2 = l1_regularization_strength, l2_regularization_strength
    self._beta = 0.0 if beta is None else beta
    self._l2_shrinkage = l2_shrinkage_regularization_strength
    self._accum_name, self._linear_name = accum_name, linear_name

  def _adjusted_l2(self):
    # TF-core FtrlOptimizer._prepare: l2 + beta / (2 * learning_rate)
    return self._l2 + self._beta / (2.0 * self._learning_rate)

  def _create_slots(self, var_list):
    for v in var_list:
      self._get_or_make_slot_with_value(v, self._initial_accumulator_value, "accum", self._accum_name or self._name)
      self._zeros_slot(v, "linear", self._linear_name or (self._name + "_1"))

  def _resource_apply_sparse(self, grad, var, indices):
    accum, linear = self.get_slot(var, "accum"), self.get_slot(var, "linear")
    return self._apply_op(var.handle, accum.handle, linear.handle, grad, indices, self._learning_rate, self._l1,
                          self._adjusted_l2(), self._l2_shrinkage, self._learning_rate_power, use_locking=True)


class GroupFtrlOptimizer(FtrlOptimizer):
  """FTRL with a group-lasso threshold l1 on each key's whole linear row (kvhip.h kv_apply_group_ftrl_v2)."""

  _apply_op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_ftrl_v2)

  def __init__(self, learning_rate, learning_rate_power=-0.5, initial_accumulator_value=0.1,
               l1_regularization_strength=0.0, l2_regularization_strength=0.0, use_locking=False, name="GroupFtrl",
               accum_name=None, linear_name=None, l2_shrinkage_regularization_strength=0.0, beta=None):
    super(GroupFtrlOptimizer, self).__init__(learning_rate, learning_rate_power, initial_accumulator_value,
                                             l1_regularization_strength, l2_regularization_strength, use_locking, name,
                                             accum_name, linear_name, l2_shrinkage_regularization_strength, beta)
