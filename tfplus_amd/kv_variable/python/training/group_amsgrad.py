"""GroupAMSGradOptimizer and GroupAdaBeliefOptimizer — Adam's two usual repairs, with group lasso, on KvVariables, through the
fused ops KvVariableGroupSparseApplyAMSGrad and KvVariableGroupSparseApplyAdaBelief (kernels/training_ops.cc:1523-1805,
2982-3251).

The reference registers both ops but ships no Python caller for them.  These classes are the callers the ops' inputs
describe, modelled on GroupAdamOptimizer: one zero-initialised slot table "opt" of dim 4*D where the reference keeps four
slot variables (m | v | linear | vhat for AMSGrad, m | v | linear | accum for AdaBelief), beta1_power / beta2_power starting
at beta and multiplied after the apply, in float32.  The two classes differ in the op they call — one kernel family, a
run-time flag apart."""
import numpy as np

from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.optimizer import Optimizer


class GroupAMSGradOptimizer(Optimizer):
  _stem = "group_amsgrad"
  _op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_amsgrad)

  def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, l1_regularization_strength=0.0,
               l2_regularization_strength=0.0, l21_regularization_strength=0.0, use_locking=False, name=None, opt_name=None):
    super(GroupAMSGradOptimizer, self).__init__(use_locking, name or type(self).__name__[:-len("Optimizer")])
    if l1_regularization_strength < 0.0:
      raise ValueError("l1_regularization_strength %f needs to be positive or zero" % l1_regularization_strength)
    if l2_regularization_strength < 0.0:
      raise ValueError("l2_regularization_strength %f needs to be positive or zero" % l2_regularization_strength)
    if l21_regularization_strength < 0.0:
      raise ValueError("l21_regularization_strength %f needs to be positive or zero" % l21_regularization_strength)
    self._lr, self._beta1, self._beta2, self._epsilon = learning_rate, beta1, beta2, epsilon
    self._l1, self._l2, self._l21 = l1_regularization_strength, l2_regularization_strength, l21_regularization_strength
    self._opt_name = opt_name
    self._beta1_power = self._beta2_power = None

  def _create_slots(self, var_list):
    if self._beta1_power is None:
      self._beta1_power = np.float32(self._beta1)
      self._beta2_power = np.float32(self._beta2)
    for v in var_list:
      v.num_concat_opt_vars = 4
      self._zeros_slot(v, "opt", self._opt_name or (self._name + "_4"))

  def _get_beta_accumulators(self):
    return self._beta1_power, self._beta2_power

  def _scalars(self):
    return (self._lr, self._beta1_power, self._beta2_power, self._beta1, self._beta2, self._epsilon, self._l1, self._l2,
            self._l21)

  def _resource_apply_sparse(self, grad, var, indices):
    return self._op(var.handle, self.get_slot(var, "opt").handle, grad, indices, *self._scalars(), use_locking=False)

  def _native_step(self, var):
    return (self._stem, (self.get_slot(var, "opt"),), self._scalars())

  def _finish(self):
    self._beta1_power = np.float32(self._beta1_power * np.float32(self._beta1))
    self._beta2_power = np.float32(self._beta2_power * np.float32(self._beta2))


class GroupAdaBeliefOptimizer(GroupAMSGradOptimizer):
  _stem = "group_adabelief"
  _op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_adabelief)
