"""The shard's batch record (tfplus_amd/csrc/kv_shard_batch.h): its transitions and what route_holds(), route_holds_ids(),
may_apply() and the tokens say after each, walked by a stand-alone program (tests/c_abi/shard_batch_check.cc) that includes the
header and kv_batch_index.h alone.  Built with the host compiler under AddressSanitizer and UBSan and run directly: no GPU,
nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_batch_transitions(tmp_path):
  src = os.path.join(ROOT, "tests", "c_abi", "shard_batch_check.cc")
  inc = os.path.join(ROOT, "tfplus_amd", "csrc")
  exe = str(tmp_path / "shard_batch_check")
  if shutil.which("g++"):
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined"]
  else:   # the compiler the library itself needs
    cmd = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined"]
  subprocess.check_call(cmd + ["-Wall", "-Werror", "-I", inc, "-o", exe, src])
  r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.strip() == "ok", r.stdout + r.stderr
