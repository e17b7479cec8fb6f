"""CPU checks of the FTRL-V2 / group FTRL-V2 ops (KvVariableSparseApplyFtrlV2, KvVariableGroupSparseApplyFtrlV2): the C ABI
declares, binds and exports them; the TF shim that registers them type-checks and carries the reference's schemas; and
the NumPy restatement the GPU tests measure against (tests/_ftrl_ref.py) reproduces the reference test's known answer."""
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
import _ftrl_ref as R  # noqa: E402
import test_tf_shim_schema as S  # noqa: E402

NEW = ["kv_apply_ftrl_v2", "kv_apply_ftrl_v2_unique", "kv_apply_ftrl_v2_tok",
       "kv_apply_group_ftrl_v2", "kv_apply_group_ftrl_v2_unique", "kv_apply_group_ftrl_v2_tok",
       "kv_multi_apply_ftrl_v2", "kv_multi_apply_ftrl_v2_tok", "kv_multi_apply_ftrl_v2_unique",
       "kv_multi_apply_group_ftrl_v2", "kv_multi_apply_group_ftrl_v2_tok", "kv_multi_apply_group_ftrl_v2_unique"]
SHIM = os.path.join(ROOT, "tfplus_amd", "tf_shim", "kv_ftrl_ops_hip.cc")
OPS = ["KvVariableSparseApplyFtrlV2", "KvVariableGroupSparseApplyFtrlV2"]


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
  # the FTRL-V2 argument lists are SparseGroupFtrl's without l21
  for n in NEW:
    ref = n.replace("group_ftrl_v2", "sparse_group_ftrl").replace("ftrl_v2", "sparse_group_ftrl")
    r_ret, r_args = _lib.SIGNATURES[ref]
    ret, args = _lib.SIGNATURES[n]
    assert ret == r_ret and len(args) == len(r_args) - 1, n


def test_sharded_optimizer_codes():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  assert (g.OPT_FTRL_V2, g.OPT_GROUP_FTRL_V2) == (4, 5)
  assert callable(g.kv_variable_sparse_apply_ftrl_v2) and callable(g.kv_variable_group_sparse_apply_ftrl_v2)
  assert callable(g.kv_multi_sparse_apply_ftrl_v2) and callable(g.kv_multi_group_sparse_apply_ftrl_v2)


def test_optimizer_classes():
  from tfplus_amd.kv_variable.python import training
  o = training.FtrlOptimizer(0.1, l2_regularization_strength=0.01, beta=0.2)
  assert abs(o._adjusted_l2() - (0.01 + 0.2 / 0.2)) < 1e-12        # TF-core FtrlOptimizer._prepare
  assert isinstance(training.GroupFtrlOptimizer(0.1), training.FtrlOptimizer)
  for bad in ({"learning_rate_power": 0.5}, {"l1_regularization_strength": -1.0}, {"initial_accumulator_value": -1.0},
              {"l2_regularization_strength": -1.0}, {"l2_shrinkage_regularization_strength": -1.0}):
    with pytest.raises(ValueError):
      training.FtrlOptimizer(0.1, **bad)


def test_shim_type_checks_against_the_mock():
  if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include/hip"):
    pytest.skip("needs g++ and the HIP headers")
  r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I",
                      os.path.join(ROOT, "tests", "tf_mock"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", SHIM],
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-3000:]


def test_shim_schemas_equal_the_reference():
  rec = json.load(open(os.path.join(HERE, "golden", "tf_reference_ftrl_ops.json")))
  ours = S._schemas(open(SHIM).read())
  assert sorted(ours) == sorted(OPS)
  for name, items in ours.items():
    assert S._digest(name) in rec["op_names_sha256"], name
    assert S._digest(items) == rec["schemas_sha256"][name], (name, items)


def test_shim_gpu_registrations():
  regs = S._expand_macros(open(SHIM).read())
  for op in OPS:
    rs = [r for n, r in regs if n == op]
    assert len(rs) == 3 and all(".Device(DEVICE_GPU)" in r for r in rs), op        # int32 / int64 / uint64 indices
    for t in ("int32", "int64_t", "uint64"):
      assert any('TypeConstraint<%s>("Tindices")' % t in r for r in rs), (op, t)
    for r in rs:
      for h in ("var", "accum", "linear", "lr", "l1", "l2", "l2_shrinkage", "lr_power"):
        assert 'HostMemory("%s")' % h in r, (op, h)
      assert 'HostMemory("grad")' not in r and 'HostMemory("indices")' not in r, r


def test_restatement_reproduces_A4(golden_dir):
  """test_training_ops.py:68-205's FTRL-V2 step, at tests/test_oracle_golden.py's bars for A4."""
  g = np.load(os.path.join(golden_dir, "A4_ftrl_v2.npz"))
  n, D = g["grad"].shape
  x, a, z = np.full((n, D), 0.03, np.float32), np.full((n, D), 0.1, np.float32), np.zeros((n, D), np.float32)
  x1, a1, z1 = R.ftrl_v2(x, a, z, g["grad"], 0.01, 0.0, 0.0, 0.0, -0.5)
  np.testing.assert_allclose(x1, g["expect_var"], rtol=1e-5, atol=1e-8)
  np.testing.assert_allclose(a1, g["expect_accum"], rtol=1e-6)
  np.testing.assert_allclose(z1, g["expect_linear"], rtol=1e-5, atol=1e-6)


def test_group_restatement_thresholds_the_row():
  """Closed form of training_ops.cc:977-1019: a row whose linear norm stays at or below l1 is blacklisted (var 0, accum
  += 2 grad^2 with the old var); above it the var is (l1 - norm) / ((sqrt(new_accum)/lr + 2 l2) norm) * linear."""
  D = 4
  x = np.zeros((2, D), np.float32)
  a = np.full((2, D), 0.1, np.float32)
  z = np.zeros((2, D), np.float32)
  g = np.array([[1e-3] * D, [1.0] * D], np.float32)
  x1, a1, z1, upd = R.group_ftrl_v2(x, a, z, g, 0.5, 0.05, 0.0, 0.0, -0.5)
  assert list(upd) == [False, True]
  np.testing.assert_array_equal(x1[0], 0)
  np.testing.assert_array_equal(a1[0], (np.float32(0.1) + np.float32(1e-6)) + np.float32(1e-6))
  norm = np.sqrt(np.float64(z1[1]) @ np.float64(z1[1]))
  exp = (0.05 - norm) / ((np.sqrt(1.1) / 0.5) * norm) * np.float64(z1[1])
  np.testing.assert_allclose(x1[1], exp, rtol=1e-6)
