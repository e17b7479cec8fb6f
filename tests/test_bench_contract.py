"""bench.py's pieces that need no GPU: the `exchange` object of a sharded line at N = 8 (the driver's largest run; no
8-GPU node is available to the tests), parsed dry."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
  spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


def test_exchange_block_of_the_eight_gpu_line():
  b = _bench()
  D, cap, distinct = 32, 18000, 109000
  x = b.exchange_block(8, cap, D, distinct, lossless=False, staged=False)
  assert x["exchanges_per_step"] == 3 and x["peer_capacity_records"] == cap and x["lossless"] is False
  # seven peers, one fixed segment each per exchange: (id, count) records out, rows back, gradient rows out
  assert x["wire_bytes_per_rank_per_step"] == 7 * (cap + 1) * (16 + 4 * D + 4 * D)
  assert x["payload_bytes_per_rank_per_step_estimate"] == int(7 / 8 * distinct * (16 + 8 * D))
  assert x["payload_bytes_per_rank_per_step_estimate"] <= x["wire_bytes_per_rank_per_step"]
  assert "RCCL" in x["transport"] and "stays in place" in x["transport"]
  # a world of one puts nothing on the wire; the rehearsal transport says what it is
  assert b.exchange_block(1, cap, D, distinct, True, False)["wire_bytes_per_rank_per_step"] == 0
  assert "staged" in b.exchange_block(2, cap, D, distinct, True, True)["transport"]


def test_dump_outputs_samples_a_fixed_bounded_set_of_rows(tmp_path):
  """--dump-outputs on the sharded path's form (lookup rows only), on host tensors: float32, within the byte budget, the
  same seeded positions from call to call, the whole output when it fits."""
  import numpy as np
  import torch
  b = _bench()
  D = 32
  out = torch.arange(300000 * D, dtype=torch.float32).reshape(300000, D)
  for d in ("a", "b"):
    b.dump_outputs(str(tmp_path / d), out, None, None, None, None)
  assert sorted(os.listdir(tmp_path / "a")) == ["lookup_rows.npy"]
  a, c = np.load(str(tmp_path / "a" / "lookup_rows.npy")), np.load(str(tmp_path / "b" / "lookup_rows.npy"))
  assert a.dtype == np.float32 and a.nbytes <= b.DUMP_ROWS_BYTES and a.shape == (b.DUMP_ROWS_BYTES // (4 * D), D)
  assert np.array_equal(a, c)
  pos = a[:, 0] // D                                   # row r of `out` starts with r * D
  assert np.array_equal(a, out.numpy()[pos.astype(np.int64)]) and (np.diff(pos) > 0).all()
  small = out[:1000]
  b.dump_outputs(str(tmp_path / "s"), small, None, None, None, None)
  assert np.array_equal(np.load(str(tmp_path / "s" / "lookup_rows.npy")), small.numpy())


def test_bench_options():
  """--full (everything besides the headline) and --dump-outputs are on the command line."""
  import subprocess
  import sys
  r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-2000:]
  assert "--full" in r.stdout and "--dump-outputs" in r.stdout
