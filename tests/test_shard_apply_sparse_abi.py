"""The fused backward of the sharded sparse lookup at the drop-in boundary, without a GPU: include/kvhip.h declares the sparse
gradient pre-sum (kv_shard_apply_route_sparse) and the two whole ops, libkvhip.so exports them, and the binding table carries
them with the header's arity."""
import ctypes
import os
import re

import pytest

from tfplus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"kv_shard_apply_route_sparse": 8, "kv_shard_apply_sparse": 14, "kv_multi_shard_apply_sparse": 15}
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


def test_the_new_unit_is_built_and_its_launchers_are_declared():
  csrc = os.path.join(ROOT, "tfplus_amd", "csrc")
  units = re.search(r"^UNITS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
  assert "kv_sums_seg" in units and os.path.exists(os.path.join(csrc, "kv_sums_seg.hip"))
  launch = open(os.path.join(csrc, "kv_launch.h")).read()
  assert "int launch_tsum_seg(" in launch and "int launch_papply_dedup_seg(" in launch
  body = open(os.path.join(csrc, "kv_sums_seg.hip")).read()
  assert re.findall(r"with_row_geom<([^>]*)>\(", body) == ["ENTRY_MAX_Q", "ENTRY_MAX_Q"]   # every rung of the entry ladder
