"""The de-duplicated path without a host round trip, at the ABI boundary (no GPU): include/kvhip.h declares
kv_dedup_segment_sum_dev (the count left on the device) and kv_apply_unique_counted (the unique apply that reads it there),
and the ctypes table binds both with the header's arity."""
import os
import re

from tfplus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("kv_dedup_segment_sum_dev", "kv_apply_unique_counted")


def _prototypes():
  """{name: [parameter text, ...]} of every function the header declares"""
  text = open(os.path.join(ROOT, "include", "kvhip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  out = {}
  for m in re.finditer(r"\bint\s+(kv_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
    params = [p.strip() for p in m.group(2).split(",")]
    out[m.group(1)] = [] if params in ([""], ["void"]) else params
  return out


def test_header_declares_the_two_functions():
  protos = _prototypes()
  for name in NEW:
    assert name in protos, "include/kvhip.h does not declare %s" % name
  d = protos["kv_dedup_segment_sum_dev"]
  assert len(d) == len(protos["kv_dedup_segment_sum"]) == 9
  assert re.search(r"int64_t\s*\*\s*num_unique_dev$", d[7]) and d[8].startswith("kv_stream_t")
  a = protos["kv_apply_unique_counted"]
  assert [re.sub(r".*\W", "", p) for p in a] == ["var", "optimizer", "slot0", "slot1", "hp", "grad", "ids", "ids_dtype", "n_max",
                                                 "n_dev", "stream"]
  assert a[9].startswith("const int64_t")


def test_signatures_carry_them_with_the_headers_arity():
  protos = _prototypes()
  for name in NEW:
    assert name in _lib.SIGNATURES, "%s is not bound" % name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._i32
    assert len(args) == len(protos[name])
  # the scalar arguments sit where the header has them
  args = _lib.SIGNATURES["kv_apply_unique_counted"][1]
  assert args[1] is _lib._i32 and args[7] is _lib._i32 and args[8] is _lib._i64
  assert _lib.SIGNATURES["kv_dedup_segment_sum_dev"][1][3] is _lib._i64


def test_every_bound_function_has_the_headers_arity():
  protos = _prototypes()
  for name, (_, args) in _lib.SIGNATURES.items():
    if name in protos:   # (kv_last_error returns a string: not an `int kv_...` prototype)
      assert len(args) == len(protos[name]), name
