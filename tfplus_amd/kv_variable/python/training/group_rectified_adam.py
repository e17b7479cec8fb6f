"""GroupRectifiedAdamOptimizer — RAdam with group lasso on KvVariables, through the fused op
KvVariableGroupSparseApplyRectifiedAdam (ops/training_ops.cc:1194-1217, kernels/training_ops.cc:6694-6978).

The reference registers that op but ships no Python caller for it: its RectifiedAdamOptimizer (rectified_adam.py:26-390)
composes the step from generic ops and has no group lasso.  This class is the caller the op's inputs describe: one slot
table "opt" of dim 5*D (m | v | linear | vhat | vamsgrad), and the host scalars — step, beta powers, the learning rate's
warm-up / decay, sma_inf, sma_t, r_t and tractable = sma_t >= sma_threshold — computed exactly as RectifiedAdamOptimizer
computes them (its _step_scalars).  l1 / l2 / l21, amsgrad and use_nesterov go to the op as they are.  The op has no weight
decay, so a non-zero weight_decay is refused."""
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.rectified_adam import RectifiedAdamOptimizer


class GroupRectifiedAdamOptimizer(RectifiedAdamOptimizer):

  def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-7, decay=0.0, weight_decay=0.0,
               amsgrad=False, sma_threshold=5.0, total_steps=0, warmup_proportion=0.1, min_lr=0.0,
               l1_regularization_strength=0.0, l2_regularization_strength=0.0, l21_regularization_strength=0.0,
               use_locking=False, use_nesterov=False, name="GroupRectifiedAdam", opt_name=None):
    if weight_decay != 0.0:
      raise ValueError("weight_decay %f: KvVariableGroupSparseApplyRectifiedAdam has no weight decay" % weight_decay)
    if l1_regularization_strength < 0.0:
      raise ValueError("l1_regularization_strength %f needs to be positive or zero" % l1_regularization_strength)
    if l2_regularization_strength < 0.0:
      raise ValueError("l2_regularization_strength %f needs to be positive or zero" % l2_regularization_strength)
    if l21_regularization_strength < 0.0:
      raise ValueError("l21_regularization_strength %f needs to be positive or zero" % l21_regularization_strength)
    super(GroupRectifiedAdamOptimizer, self).__init__(learning_rate, beta1, beta2, epsilon, decay, 0.0, amsgrad,
                                                      sma_threshold, total_steps, warmup_proportion, min_lr, use_locking,
                                                      use_nesterov, name)
    self._l1, self._l2, self._l21 = l1_regularization_strength, l2_regularization_strength, l21_regularization_strength
    self._opt_name = opt_name

  def _create_slots(self, var_list):
    self._init_accumulators()
    for v in var_list:
      v.num_concat_opt_vars = 5
      self._zeros_slot(v, "opt", self._opt_name or (self._name + "_5"))

  def _resource_apply_sparse(self, grad, var, indices):
    lr_t, _, _, tractable, r_t = self._step_scalars()
    return gen_kv_variable_ops.kv_variable_group_sparse_apply_rectified_adam(
        var.handle, self.get_slot(var, "opt").handle, grad, indices, lr_t, self._beta1_power, self._beta2_power,
        self._beta1, self._beta2, self._epsilon, self._l1, self._l2, self._l21, r_t, tractable, self._amsgrad,
        self._use_nesterov, use_locking=False)
