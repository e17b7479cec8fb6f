"""Group LAMB at the drop-in boundary, without a GPU: header, library, binding table, Python layer."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvhip.h")
# (var, opt, grad, ids, n) + nine floats + stream; the batched forms carry the table count, _tok the token(s)
ARITY = {"kv_%sapply_group_lamb%s" % (multi, form): 15 + bool(multi) + (form == "_tok")
         for multi in ("", "multi_") for form in ("", "_tok", "_unique")}
SCALARS = ["lr", "beta1_power", "beta2_power", "beta1", "beta2", "epsilon", "l1", "l2", "l21"]


@pytest.mark.parametrize("name", sorted(ARITY))
def test_header_library_and_binding_table_agree(name):
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
  assert m, "include/kvhip.h does not declare %s" % name
  args = [a.strip() for a in m.group(1).split(",") if a.strip()]
  assert len(args) == ARITY[name] and [a.split()[-1] for a in args if a.startswith("float ")] == SCALARS
  assert hasattr(ctypes.CDLL(_lib.build()), name), "libkvhip.so does not export %s" % name
  argtypes = _lib.SIGNATURES[name][1]
  assert len(argtypes) == ARITY[name] and argtypes.count(ctypes.c_float) == 9


def test_python_layer_names_the_op():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  from tfplus_amd.kv_variable.python import training
  assert len(ARITY) == 6 and g.OPT_GROUP_LAMB == 10 and g._HP_LEN[10] == 9
  assert _lib.OPT_FAMILIES["group_lamb"] == (2, "gin" + "f" * 9)
  assert g._code_and_hp("group_lamb", range(1, 10)) == (10, [float(v) for v in range(1, 10)])
  assert callable(g.kv_variable_group_sparse_apply_lamb) and callable(g.kv_multi_group_sparse_apply_lamb)
  assert training.GroupLambOptimizer(0.01)._stem == "group_lamb"
