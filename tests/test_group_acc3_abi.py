"""Group Momentum / group Adadelta at the drop-in boundary, without a GPU: header, library, binding table, Python layer."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvhip.h")
SCALARS = {"momentum": ["lr", "momentum", "l1", "l2", "l21"], "adadelta": ["lr", "rho", "epsilon", "l1", "l2", "l21"]}
# (var, opt, grad, ids, n) + the scalars (Momentum: five floats and int use_nesterov) + stream; the batched forms carry the
# table count, _tok the token(s)
ARITY = {"kv_%sapply_group_%s%s" % (multi, stem, form): 12 + bool(multi) + (form == "_tok")
         for multi in ("", "multi_") for stem in SCALARS for form in ("", "_tok", "_unique")}


@pytest.mark.parametrize("name", sorted(ARITY))
def test_header_library_and_binding_table_agree(name):
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
  assert m, "include/kvhip.h does not declare %s" % name
  args = [a.strip() for a in m.group(1).split(",") if a.strip()]
  floats = SCALARS["momentum" if "momentum" in name else "adadelta"]
  assert len(args) == ARITY[name] and [a.split()[-1] for a in args if a.startswith("float ")] == floats
  assert ("int use_nesterov" in args) == ("momentum" in name)
  assert hasattr(ctypes.CDLL(_lib.build()), name), "libkvhip.so does not export %s" % name
  argtypes = _lib.SIGNATURES[name][1]
  assert len(argtypes) == ARITY[name] and argtypes.count(ctypes.c_float) == len(floats)


def test_python_layer_names_the_ops():
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  from tfplus_amd.kv_variable.python import training
  assert len(ARITY) == 12 and g.OPT_GROUP_ACC3 == 11 and g._HP_LEN[11] == 7
  assert _lib.OPT_FAMILIES["group_momentum"] == (2, "gin" + "f" * 5 + "b")
  assert _lib.OPT_FAMILIES["group_adadelta"] == (2, "gin" + "f" * 6)
  # hp = lr, decay, epsilon, l1, l2, l21, variant: the variant appended, Momentum's from use_nesterov, its epsilon 0
  assert g._code_and_hp("group_momentum", (1, 2, 3, 4, 5, False)) == (11, [1.0, 2.0, 0.0, 3.0, 4.0, 5.0, 0.0])
  assert g._code_and_hp("group_momentum", (1, 2, 3, 4, 5, True)) == (11, [1.0, 2.0, 0.0, 3.0, 4.0, 5.0, 1.0])
  assert g._code_and_hp("group_adadelta", range(1, 7)) == (11, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 2.0])
  with pytest.raises(_lib.InvalidArgumentError, match="0 or 1"):
    g._code_and_hp("group_momentum", (1, 2, 3, 4, 5, 2))
  for stem in ("momentum", "adadelta"):
    assert callable(getattr(g, "kv_variable_group_sparse_apply_" + stem)) and callable(getattr(g, "kv_multi_group_sparse_apply_" + stem))
  assert training.GroupMomentumOptimizer(0.01)._stem == "group_momentum"
  assert training.GroupAdadeltaOptimizer()._stem == "group_adadelta"
