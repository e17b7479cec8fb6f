"""Plain Adam's fused op at the drop-in boundary, without a GPU: include/kvhip.h declares the six kv_apply_adam entry
points, libkvhip.so exports them, the binding table carries them with the header's arity, and the Python layer names the
op and its optimizer code."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (var, m_v, grad, ids, n) + six scalars + stream; the batched forms carry the table count, _tok the token(s)
ARITY = {"kv_apply_adam": 12, "kv_apply_adam_tok": 13, "kv_apply_adam_unique": 12,
         "kv_multi_apply_adam": 13, "kv_multi_apply_adam_tok": 14, "kv_multi_apply_adam_unique": 13}
NAMES = sorted(ARITY)


def _header_args(name):
  text = open(os.path.join(ROOT, "include", "kvhip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
  assert m, "include/kvhip.h does not declare %s" % name
  return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares(name):
  args = _header_args(name)
  assert len(args) == ARITY[name]
  floats = [a.split()[-1] for a in args if a.startswith("float ")]
  assert floats == ["lr", "beta1_power", "beta2_power", "beta1", "beta2", "epsilon"]


@pytest.mark.parametrize("name", NAMES)
def test_library_exports(name):
  so = ctypes.CDLL(_lib.build())
  assert hasattr(so, name), "libkvhip.so does not export %s" % name


@pytest.mark.parametrize("name", NAMES)
def test_binding_table_has_the_headers_arity(name):
  assert name in _lib.SIGNATURES
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype is ctypes.c_int32 or restype is ctypes.c_int
  assert len(argtypes) == ARITY[name]
  assert argtypes.count(ctypes.c_float) == 6


def test_python_layer_names_the_op():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  from tfplus_amd.kv_variable.python import training
  assert _lib.OPT_FAMILIES["adam"] == (2, "gin" + "f" * 6)
  assert g.OPT_ADAM == 7 and g._COUNTED_CODE["adam"] == 7
  assert callable(g.kv_variable_sparse_apply_adam) and callable(g.kv_multi_sparse_apply_adam)
  assert training.AdamOptimizer()._fused is False and training.AdamOptimizer(fused=True)._fused is True
  assert "tools/soak.py" in training.adam.__doc__
