"""The max_norm sparse lookups at the drop-in boundary, without a GPU: declared in include/kvhip.h, exported, bound with its arity."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"kv_lookup_sparse_clip": 13, "kv_lookup_sparse_clip_grad": 12, "kv_lookup_sparse_zeros_clip": 11}


@pytest.mark.parametrize("name", sorted(ARITY))
def test_declared_exported_and_bound(name):
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kvhip.h")).read(), flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
  assert m, "include/kvhip.h does not declare %s" % name
  assert len([a for a in m.group(1).split(",") if a.strip()]) == ARITY[name]
  assert hasattr(ctypes.CDLL(_lib.build()), name), "libkvhip.so does not export %s" % name
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype is ctypes.c_int and len(argtypes) == ARITY[name] and ctypes.c_float in argtypes   # (max_norm travels as a float)
