"""kv_apply_rectified_adam at the drop-in boundary, without a GPU: header, library, binding table and Python layer agree."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvhip.h")
# (var, opt, grad, ids, n) + eight floats + three flags + stream; the batched forms carry the table count, _tok the token(s)
ARITY = {"kv_apply_rectified_adam": 17, "kv_apply_rectified_adam_tok": 18, "kv_apply_rectified_adam_unique": 17,
         "kv_multi_apply_rectified_adam": 18, "kv_multi_apply_rectified_adam_tok": 19, "kv_multi_apply_rectified_adam_unique": 18}
SCALARS = ["lr_t", "beta1_power", "beta2_power", "beta1", "beta2", "epsilon", "weight_decay", "r_t", "tractable", "amsgrad",
           "use_nesterov"]


@pytest.mark.parametrize("name", sorted(ARITY))
def test_header_library_and_binding_table_agree(name):
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
  assert m, "include/kvhip.h does not declare %s" % name
  args = [a.strip() for a in m.group(1).split(",") if a.strip()]
  assert len(args) == ARITY[name] and [a.split()[-1] for a in args if a.startswith(("float ", "int "))][-11:] == SCALARS
  assert hasattr(ctypes.CDLL(_lib.build()), name), "libkvhip.so does not export %s" % name
  argtypes = _lib.SIGNATURES[name][1]
  assert len(argtypes) == ARITY[name] and argtypes.count(ctypes.c_float) == 8


def test_python_layer_names_the_op():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  from tfplus_amd.kv_variable.python import training
  assert _lib.OPT_FAMILIES["rectified_adam"] == (2, "gin" + "f" * 8 + "bbb")
  assert g.OPT_RADAM == 8 and g._COUNTED_CODE["radam"] == 8 and g._COUNTED_CODE["rectified_adam"] == 8
  assert callable(g.kv_variable_sparse_apply_rectified_adam) and callable(g.kv_multi_sparse_apply_rectified_adam)
  assert training.RectifiedAdamOptimizer()._fused is False and training.RectifiedAdamOptimizer(fused=True)._fused is True
  assert "NOT interchangeable" in training.rectified_adam.__doc__
