"""The table's batch-index record (tfplus_amd/csrc/kv_batch_index.h): its transitions, holds() and the four outcomes of
plan(), walked by a stand-alone program (tests/c_abi/batch_index_check.cc) that includes the header alone.  Built with the
host compiler under AddressSanitizer and UBSan and run directly: no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_index_transitions(tmp_path):
  src = os.path.join(ROOT, "tests", "c_abi", "batch_index_check.cc")
  inc = os.path.join(ROOT, "tfplus_amd", "csrc")
  exe = str(tmp_path / "batch_index_check")
  if shutil.which("g++"):
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined"]
  else:   # the compiler the library itself needs
    cmd = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined"]
  subprocess.check_call(cmd + ["-Wall", "-Werror", "-I", inc, "-o", exe, src])
  r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.strip() == "ok", r.stdout + r.stderr
