"""The fused backward of the sparse lookup on plain tables at the drop-in boundary, without a GPU: include/kvhip.h declares
kv_apply_sparse and kv_multi_apply_sparse, libkvhip.so exports them, the binding table carries them with the header's arity."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_shard_apply_sparse_abi import _header_arity  # noqa: E402
from tfplus_amd import _lib  # noqa: E402

ARITY = {"kv_apply_sparse": 14, "kv_multi_apply_sparse": 15}


@pytest.mark.parametrize("name", tuple(ARITY))
def test_declared_exported_and_bound_with_the_headers_arity(name):
  assert _header_arity(name) == ARITY[name]
  assert hasattr(ctypes.CDLL(_lib.build()), name), "libkvhip.so does not export %s" % name
  restype, argtypes = _lib.SIGNATURES[name]
  assert restype in (ctypes.c_int32, ctypes.c_int) and len(argtypes) == ARITY[name]
