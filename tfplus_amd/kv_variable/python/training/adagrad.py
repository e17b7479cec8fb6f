"""AdagradOptimizer — tfplus/kv_variable/python/training/adagrad.py:31-51 over
tf.compat.v1.train.AdagradOptimizer: slot "accumulator" initialised to
initial_accumulator_value (TF default 0.1), KvVariableSparseApplyAdagrad with use_locking=True."""
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.optimizer import Optimizer


class AdagradOptimizer(Optimizer):

  def __init__(self, learning_rate, initial_accumulator_value=0.1, use_locking=False, name="Adagrad"):
    if initial_accumulator_value <= 0.0:
      raise ValueError("initial_accumulator_value must be positive: %s" % initial_accumulator_value)
    super(AdagradOptimizer, self).__init__(use_locking, name)
    self._learning_rate = learning_rate
    self._initial_accumulator_value = initial_accumulator_value

  def _create_slots(self, var_list):
    for v in var_list:
      self._get_or_make_slot_with_value(v, self._initial_accumulator_value, "accumulator", self._name)

  def _resource_apply_sparse(self, grad, var, indices):
    acc = self.get_slot(var, "accumulator")
    return gen_kv_variable_ops.kv_variable_sparse_apply_adagrad(
        var.handle, acc.handle, self._learning_rate, grad, indices, use_locking=True)

  def _native_step(self, var):
    return "adagrad", (self.get_slot(var, "accumulator"),), (self._learning_rate, True)
