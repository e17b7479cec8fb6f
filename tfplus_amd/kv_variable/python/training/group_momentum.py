"""GroupMomentumOptimizer and GroupAdadeltaOptimizer — momentum SGD (optionally Nesterov) and Adadelta, with group lasso, on
KvVariables, through the fused ops KvVariableGroupSparseApplyMomentum and KvVariableGroupSparseApplyAdadelta
(kernels/training_ops.cc:2274-2508, 2005-2253).

The reference registers both ops but ships no Python caller for them.  These classes are the callers the ops' inputs
describe, modelled on GroupAMSGradOptimizer: one zero-initialised slot table "opt" of dim 3*D where the reference keeps three
slot variables (accum | linear | m for Momentum, accum | linear | accum_update for Adadelta), no state besides it, and
_native_step, so that fused_backward=True reaches kv_apply_sparse.  The two classes differ in the op they call and its
scalars — one kernel family, a run-time variant apart."""
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.optimizer import Optimizer


class GroupMomentumOptimizer(Optimizer):
  _stem = "group_momentum"
  _op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_momentum)

  def __init__(self, learning_rate, momentum=0.9, use_nesterov=False, l1_regularization_strength=0.0,
               l2_regularization_strength=0.0, l21_regularization_strength=0.0, use_locking=False, name=None, opt_name=None):
    super(GroupMomentumOptimizer, self).__init__(use_locking, name or type(self).__name__[:-len("Optimizer")])
    self._lr, self._decay, self._use_nesterov = learning_rate, momentum, bool(use_nesterov)
    self._set_strengths(l1_regularization_strength, l2_regularization_strength, l21_regularization_strength, opt_name)

  def _set_strengths(self, l1, l2, l21, opt_name):
    for name, value in (("l1", l1), ("l2", l2), ("l21", l21)):
      if value < 0.0:
        raise ValueError("%s_regularization_strength %f needs to be positive or zero" % (name, value))
    self._l1, self._l2, self._l21, self._opt_name = l1, l2, l21, opt_name

  def _create_slots(self, var_list):
    for v in var_list:
      v.num_concat_opt_vars = 3
      self._zeros_slot(v, "opt", self._opt_name or (self._name + "_3"))

  def _scalars(self):
    return (self._lr, self._decay, self._l1, self._l2, self._l21, self._use_nesterov)

  def _resource_apply_sparse(self, grad, var, indices):
    return self._op(var.handle, self.get_slot(var, "opt").handle, grad, indices, *self._scalars(), use_locking=False)

  def _native_step(self, var):
    return (self._stem, (self.get_slot(var, "opt"),), self._scalars())


class GroupAdadeltaOptimizer(GroupMomentumOptimizer):
  _stem = "group_adadelta"
  _op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_adadelta)

  def __init__(self, learning_rate=0.001, rho=0.95, epsilon=1e-8, l1_regularization_strength=0.0,
               l2_regularization_strength=0.0, l21_regularization_strength=0.0, use_locking=False, name=None, opt_name=None):
    Optimizer.__init__(self, use_locking, name or type(self).__name__[:-len("Optimizer")])
    self._lr, self._decay, self._epsilon = learning_rate, rho, epsilon
    self._set_strengths(l1_regularization_strength, l2_regularization_strength, l21_regularization_strength, opt_name)

  def _scalars(self):
    return (self._lr, self._decay, self._epsilon, self._l1, self._l2, self._l21)
