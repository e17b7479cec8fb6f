"""CPU checks of the group RectifiedAdam op (KvVariableGroupSparseApplyRectifiedAdam): the C ABI declares, binds and
exports it; the TF shim that registers it type-checks and carries the reference's schema; GroupRectifiedAdamOptimizer
refuses what the op cannot do; and the NumPy restatement the GPU tests measure against (tests/_radam_ref.py) agrees with
the closed forms of RAdam and tracks the composite RectifiedAdamOptimizer's formulas."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tfplus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _radam_ref as R  # noqa: E402
import test_tf_shim_schema as S  # noqa: E402

F = np.float32
NEW = ["kv_apply_group_rectified_adam", "kv_apply_group_rectified_adam_tok", "kv_apply_group_rectified_adam_unique",
       "kv_multi_apply_group_rectified_adam", "kv_multi_apply_group_rectified_adam_tok",
       "kv_multi_apply_group_rectified_adam_unique"]
SHIM = os.path.join(ROOT, "tfplus_amd", "tf_shim", "kv_radam_ops_hip.cc")
OP = "KvVariableGroupSparseApplyRectifiedAdam"
SCALARS = ["lr", "beta1_power", "beta2_power", "beat1", "beta2", "epsilon", "l1", "l2", "l21", "r_t", "tractable", "amsgrad",
           "use_nesterov"]


def _declared():
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kvhip.h")).read(), flags=re.S)
  return set(re.findall(r"\b(kv_[a-z0-9_]+)\s*\(", text))


def test_entry_points_declared_bound_and_exported():
  so = ctypes.CDLL(_lib.build())
  decl = _declared()
  for n in NEW:
    assert n in decl, n
    assert n in _lib.SIGNATURES, n
    assert hasattr(so, n), n
  # GroupAdam's argument lists with r_t and the three flags in place of `version`
  for n in NEW:
    r_ret, r_args = _lib.SIGNATURES[n.replace("group_rectified_adam", "group_adam")]
    ret, args = _lib.SIGNATURES[n]
    assert ret == r_ret and len(args) == len(r_args) + 3, n
    assert args.count(ctypes.c_float) == r_args.count(ctypes.c_float) + 1, n


def test_python_ops_and_sharded_code():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  assert g.OPT_GROUP_RADAM == 6
  assert callable(g.kv_variable_group_sparse_apply_rectified_adam) and callable(g.kv_multi_group_sparse_apply_rectified_adam)


def test_optimizer_class_arguments():
  from tfplus_amd.kv_variable.python import training
  o = training.GroupRectifiedAdamOptimizer(0.01, l21_regularization_strength=1e-3, amsgrad=True)
  assert isinstance(o, training.RectifiedAdamOptimizer) and o.get_name() == "GroupRectifiedAdam"
  for bad in ({"weight_decay": 0.1}, {"l1_regularization_strength": -1.0}, {"l2_regularization_strength": -1.0},
              {"l21_regularization_strength": -1.0}):
    with pytest.raises(ValueError):
      training.GroupRectifiedAdamOptimizer(0.01, **bad)
  assert "no Python caller" in training.group_rectified_adam.__doc__


def test_shim_type_checks_against_the_mock():
  if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include/hip"):
    pytest.skip("needs g++ and the HIP headers")
  r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I",
                      os.path.join(ROOT, "tests", "tf_mock"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", SHIM],
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-3000:]


def test_shim_schema_equals_the_reference():
  rec = json.load(open(os.path.join(HERE, "golden", "tf_reference_radam_ops.json")))
  ours = S._schemas(open(SHIM).read())
  assert sorted(ours) == [OP]
  assert S._digest(OP) in rec["op_names_sha256"]
  assert S._digest(ours[OP]) == rec["schemas_sha256"][OP], ours[OP]


def test_shim_gpu_registrations():
  regs = S._expand_macros(open(SHIM).read())
  rs = [r for n, r in regs if n == OP]
  assert len(rs) == 3 and all(".Device(DEVICE_GPU)" in r for r in rs)        # int32 / int64 / uint64 indices
  for t in ("int32", "int64_t", "uint64"):
    assert any('TypeConstraint<%s>("Tindices")' % t in r for r in rs), t
  for r in rs:
    for h in ["var", "opt"] + SCALARS:
      assert 'HostMemory("%s")' % h in r, h
    assert 'HostMemory("grad")' not in r and 'HostMemory("indices")' not in r, r


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _fresh(rng, U, D):
  return (rng.standard_normal((U, D)) * 0.3).astype(F), np.zeros((U, 5 * D), F), rng.normal(0, 0.1, (U, D)).astype(F)


@pytest.mark.parametrize("nesterov", [False, True])
def test_first_step_closed_forms(nesterov):
  """From fresh state (m = v = linear = vhat = 0) with l1 = l2 = l21 = 0 one step is x - lr m_hat while not tractable and
  x - lr r_t m_hat / (sqrt(v_hat) + eps) once tractable (float64 closed forms; m_hat = m / (1 - beta1_power),
  v_hat = v / (1 - beta2_power))."""
  rng = np.random.default_rng(1)
  x, slot, g = _fresh(rng, 64, 8)
  lr, b1, b2, eps, r_t = 1e-2, 0.9, 0.999, 1e-7, 0.37
  b1p, b2p = b1, b2
  g64, x64 = g.astype(np.float64), x.astype(np.float64)
  m = (1 - b1) * g64
  if nesterov:
    m = g64 * (1 - b1) + b1 * m
  m_hat = m / (1 - float(F(b1p)))
  v_hat = (1 - float(F(b2))) * g64 * g64 / (1 - float(F(b2p)))
  x1, s1, upd = R.group_radam(x, slot, g, lr, b1p, b2p, b1, b2, eps, 0, 0, 0, r_t, False, False, nesterov)
  assert upd.all()
  # each of the ~10 float32 operations contributes 2^-24 of |x| or of the step: 1e-6 of both is a loose cover
  np.testing.assert_allclose(x1, x64 - lr * m_hat, rtol=0, atol=1e-6 * (np.abs(x64) + lr * np.abs(m_hat)).max())
  for ams in (False, True):
    x1, s1, upd = R.group_radam(x, slot, g, lr, b1p, b2p, b1, b2, eps, 0, 0, 0, r_t, True, ams, nesterov)
    step = lr * r_t * m_hat / (np.sqrt(v_hat) + eps)
    assert upd.all()
    np.testing.assert_allclose(x1, x64 - step, rtol=0, atol=1e-6 * (np.abs(x64) + np.abs(step)).max())
    np.testing.assert_array_equal(s1[:, 32:40] != 0, np.full((64, 8), ams))          # vamsgrad: the amsgrad branch only
    np.testing.assert_array_equal(s1[:, 24:32], ((np.sqrt(s1[:, 32:40] if ams else s1[:, 8:16]) /
                                                  R.host_scalars(b1p, b2p)[0] + F(eps)) / F(lr)).astype(F))


def test_eight_steps_track_the_composite_formulas():
  """The fused step with all regularisers 0 is the composite optimizer's x - lr_t upd in other operations.  D = 8, 64 keys,
  default betas: not tractable on steps 1-5, tractable from step 6, where rv drops from 1 / lr to sqrt(v) / (alpha lr) and
  linear = rm - (rv - vhat) x cancels.  Tolerance: tests/_radam_ref.py composite_step_tolerance — 17 roundings times
  2^-24 (max(rv, vhat) |x| / rv + |dx|) per step, summed over the steps."""
  from tfplus_amd.kv_variable.python import training
  rng = np.random.default_rng(2)
  U, D = 64, 8
  x, slot, _ = _fresh(rng, U, D)
  opt = training.RectifiedAdamOptimizer(1e-3)
  opt._init_accumulators()
  xc, m, v, vm = x.copy(), np.zeros((U, D), F), np.zeros((U, D), F), np.zeros((U, D), F)
  tol = np.zeros((U, D))
  tract = []
  for t in range(8):
    g = rng.normal(0, 0.1, (U, D)).astype(F)
    lr_t, _, _, tractable, r_t = opt._step_scalars()
    b1p, b2p = opt._beta1_power, opt._beta2_power
    tract.append(tractable)
    vh = slot[:, 3 * D:4 * D].copy()
    x1, slot, upd = R.group_radam(x, slot, g, lr_t, b1p, b2p, 0.9, 0.999, 1e-7, 0, 0, 0, r_t, tractable, False, False)
    assert upd.all()
    tol += R.composite_step_tolerance(x, x1, slot[:, 3 * D:4 * D], vh)
    x = x1
    xc, m, v, vm = R.composite_radam(xc, m, v, vm, g, lr_t, b1p, b2p, 0.9, 0.999, 1e-7, r_t, tractable, False, False)
    diff = np.abs(x.astype(np.float64) - xc)
    print("step %d tractable %d: max |fused - composite| %.3g, tolerance there %.3g, max |x| %.3g"
          % (t + 1, tractable, diff.max(), tol.flat[diff.argmax()], np.abs(x).max()))
    assert (diff <= tol).all(), (t, diff.max())
    np.testing.assert_array_equal(slot[:, :D], m)          # the moments are the same operations: the same bits
    np.testing.assert_array_equal(slot[:, D:2 * D], v)
    opt._finish()
  assert tract == [False] * 5 + [True] * 3


def test_rows_at_or_below_the_lasso_threshold_are_blacklisted():
  """norm = |clamp(linear, -l1, l1) - linear|_2 against l21 sqrt(D): a row that stays at or below it is blacklisted (its var
  reads as zeros, its slot row is updated all the same), one above it is scaled by 1 - l21 sqrt(D) / norm."""
  D = 4
  x = np.zeros((3, D), F)
  slot = np.zeros((3, 5 * D), F)
  lr, l21 = 0.5, 0.1                            # not tractable: linear = g (1 - b1) / (1 - b1p) = g, rv = 1 / lr = 2
  g = np.array([[0.05] * D, [0.1] * D, [1.0] * D], F)      # norms 0.1, 0.2 (= l21 sqrt(D) in float32: not above), 2
  x1, s1, upd = R.group_radam(x, slot, g, lr, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.0, 0.0, l21, 0.0, False, False, False)
  z1 = s1[:, 2 * D:3 * D]
  np.testing.assert_allclose(z1, g, rtol=1e-6)
  norm = np.sqrt((z1.astype(np.float64) ** 2).sum(axis=1))
  thr = float(F(l21) * np.sqrt(F(D)))
  assert list(norm > thr) == [False, False, True] == list(upd)
  np.testing.assert_array_equal(x1[:2], 0)
  np.testing.assert_allclose(x1[2], -z1[2] * (1 - thr / norm[2]) / 2.0, rtol=1e-6)
  np.testing.assert_array_equal(s1[:, 3 * D:4 * D], F(2))          # vhat = rv, blacklisted or not
  assert np.isinf(R.norm_over_threshold(x, slot, g, lr, 0.9, 0.999, 0.9, 0.999, 1e-7, 0.0, 0.0, 0.0, 0.0, False, False,
                                        False)).all()
