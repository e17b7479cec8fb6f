"""The sparse lookup on sharded tables at the drop-in boundary, without a GPU: include/kvhip.h declares the combining finish
(kv_shard_lookup_finish_sparse) and the four whole ops, libkvhip.so exports them, and the binding table carries them with
the header's arity."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"kv_shard_lookup_finish_sparse": 8, "kv_shard_lookup_sparse": 12, "kv_shard_lookup_sparse_zeros": 12,
         "kv_multi_shard_lookup_sparse": 13, "kv_multi_shard_lookup_sparse_zeros": 13}
NAMES = tuple(ARITY)


def _header_arity(name):
  text = open(os.path.join(ROOT, "include", "kvhip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
  assert m, "include/kvhip.h does not declare %s" % name
  return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NAMES)
def test_header_declares(name):
  assert _header_arity(name) == ARITY[name]


@pytest.mark.parametrize("name", NAMES)
def test_library_exports(name):
  so = ctypes.CDLL(_lib.build())
  assert hasattr(so, name), "libkvhip.so does not export %s" % name


@pytest.mark.parametrize("name", NAMES)
def test_binding_table_has_the_headers_arity(name):
  assert name in _lib.SIGNATURES
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype is ctypes.c_int32 or restype is ctypes.c_int
  assert len(argtypes) == _header_arity(name)
