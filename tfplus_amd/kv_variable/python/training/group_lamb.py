"""GroupLambOptimizer — LAMB (layer-wise adaptation, here per embedding row) with group lasso on KvVariables, through the
fused op KvVariableGroupSparseApplyLamb (kernels/training_ops.cc:3400-3683).

The reference registers the op but ships no Python caller for it.  This class is the caller the op's inputs describe, and
it is GroupAMSGradOptimizer in everything but the op it calls: one zero-initialised slot table "opt" of dim 4*D where the
reference keeps four slot variables (m | v | linear | accum), beta1_power / beta2_power starting at beta and multiplied
after the apply, in float32, and _native_step, so that fused_backward=True reaches kv_apply_sparse.  The op scales each
row's bias-corrected step by that row's trust ratio |var| / |m_hat / (sqrt(v_hat) + epsilon)| before it enters linear; a row
whose var is all zeros (a new or blacklisted key) takes ratio 1."""
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops
from tfplus_amd.kv_variable.python.training.group_amsgrad import GroupAMSGradOptimizer


class GroupLambOptimizer(GroupAMSGradOptimizer):
  _stem = "group_lamb"
  _op = staticmethod(gen_kv_variable_ops.kv_variable_group_sparse_apply_lamb)
