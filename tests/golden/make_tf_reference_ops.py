"""Generates tests/golden/tf_reference_ops.json — the fingerprint of the reference's op interface that
tests/test_tf_shim_schema.py checks the TF shim against.

The reference (tfplus) is not part of this repository and none of its text is stored here: the record holds SHA-256
digests only (tests/test_tf_shim_schema.py _digest):
  op_names_sha256            one per op that the reference's tfplus/kv_variable/ops/*.cc register (REGISTER_OP)
  schemas_sha256             per op the shim registers: the digest of the reference's Input / Output / Attr /
                             SetIsStateful items of that op, in source order, as the test's _schemas() reads them
  python_layer_calls_sha256  one per gen_kv_variable_ops wrapper name that the reference's Python layer calls

Run:  python tests/golden/make_tf_reference_ops.py <reference source root>      (rewrites the .json in place)
"""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_tf_shim_schema as t  # noqa: E402

PY_FILES = ["ops/kv_variable_ops.py", "ops/embedding_ops.py", "ops/variable_scope.py", "training/group_adam.py",
            "training/adagrad.py", "training/sparse_group_ftrl.py", "training/adam.py", "training/gradient_descent.py"]


def main(ref_root):
  kv = os.path.join(ref_root, "tfplus", "kv_variable")
  ref = {}
  for f in sorted(glob.glob(os.path.join(kv, "ops", "*.cc"))):
    ref.update(t._schemas(open(f).read()))
  if not ref:
    sys.exit("no REGISTER_OP found under %s" % os.path.join(kv, "ops"))
  ours = t._schemas(open(t.SHIM).read())
  called = set()
  for f in PY_FILES:
    p = os.path.join(kv, "python", f)
    if os.path.exists(p):
      called |= set(re.findall(r"gen_kv_variable_ops\.([a-z_0-9]+)", open(p).read()))
  have = {t._snake(n) for n in t.REQUIRED} | t.EXCLUDED
  for n in sorted(called - have):
    print("called by the reference's Python layer, neither required nor excluded:", n)
  rec = {"op_names_sha256": sorted(t._digest(n) for n in ref),
         "schemas_sha256": {n: t._digest(ref[n]) for n in sorted(ours) if n in ref},
         "python_layer_calls_sha256": sorted(t._digest(n) for n in called)}
  with open(os.path.join(HERE, "tf_reference_ops.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")


if __name__ == "__main__":
  if len(sys.argv) != 2:
    sys.exit(__doc__)
  main(sys.argv[1])
