"""Generates tests/golden/tf_reference_radam_ops.json — the fingerprint of the reference's schemas of the op that
tfplus_amd/tf_shim/kv_radam_ops_hip.cc registers (KvVariableGroupSparseApplyRectifiedAdam), in the
digest form of make_tf_reference_ops.py: SHA-256 of the op name, and of the reference's Input / Output / Attr /
SetIsStateful items of that op in source order (tests/test_tf_shim_schema.py _schemas / _digest).  Digests only: none
of the reference's text is stored here.

Run:  python tests/golden/make_tf_reference_radam_ops.py <reference source root>      (rewrites the .json in place)
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_tf_shim_schema as t  # noqa: E402

SHIM = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tfplus_amd", "tf_shim", "kv_radam_ops_hip.cc")
OPS = ["KvVariableGroupSparseApplyRectifiedAdam"]


def main(ref_root):
  kv = os.path.join(ref_root, "tfplus", "kv_variable")
  ref = {}
  for f in sorted(glob.glob(os.path.join(kv, "ops", "*.cc"))):
    ref.update(t._schemas(open(f).read()))
  missing = [n for n in OPS if n not in ref]
  if missing:
    sys.exit("the reference registers no op named %s" % ", ".join(missing))
  rec = {"op_names_sha256": sorted(t._digest(n) for n in OPS),
         "schemas_sha256": {n: t._digest(ref[n]) for n in sorted(OPS)}}
  with open(os.path.join(HERE, "tf_reference_radam_ops.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")


if __name__ == "__main__":
  if len(sys.argv) != 2:
    sys.exit(__doc__)
  main(sys.argv[1])
