"""The two forms of every route-side phase of a sharded table (kv_shard.hip route_impl / finish_impl / presum_impl): several
tables in one launch, and one table with its descriptor by value — which is also what the phase calls kv_shard_lookup_route /
kv_shard_lookup_finish / kv_shard_apply_route run.  World 1 without RCCL, dims 4 and 12 (12: a masked-lane row geometry),
batches of at most 300 ids with repeats, peer_capacity sized to the batch.

ONE kv_multi_shard_lookup + kv_multi_shard_apply over four tables, so that every grouped phase also has tables left over:
  0, 1  default mode, one dim       the grouped arm of route, finish and pre-sum
  2     deterministic mode, the     left over: the single arm, with the ordered owner scatter (and, being of another row
        other dim                   geometry, left over by the finish too)
  3     an empty batch              left over: the void route; no finish, no pre-sum
against twin tables driven one at a time through the phase calls with the in-process exchange.  Then, on the tables of the whole
ops: the empty table's apply_route with a null gradient, and a finish whose route index is not there — here because the route
in between was refused and published none (a shard's route table is its own: no other route reaches it); the arm in which
another publish made the token stale is walked on the host, by tests/c_abi/shard_batch_check.cc.

Tolerance: rows are copies (bit for bit); the state of the deterministic table and of every id that occurs once in its batch
is bit for bit; a repeated id's fp32 sums take another order in the default mode — rtol 2e-5, atol 1e-6, the bar of
tests/test_gpu_multi_shard.py::test_multi_shard_batched_phases_equal_the_per_table_ops."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DAY = 19000
HP = (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
RTOL, ATOL = 2e-5, 1e-6
NS = (300, 257, 300, 0)                    # ids per table
DET = (False, False, True, False)
CAP, MAX_IDS = 300, 8192                   # peer_capacity: the batch; max_ids: room for the batch the refused route names
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _table(ops, D, init, det):
  h = ops.kv_variable([D])
  ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, init)
  if det:
    ops.kv_set_deterministic(h, True)
  return h


def _tables(ops, dims):
  vs, ss, shs = [], [], []
  for k, (D, det) in enumerate(zip(dims, DET)):
    init = np.random.default_rng(700 + k).standard_normal((32, D)).astype(np.float32)
    v = _table(ops, D, init, det); s = _table(ops, 3 * D, np.zeros((4, 3 * D), np.float32), det)
    vs.append(v); ss.append(s)
    shs.append(ops.KvShard(v, 1, 0, ops.KV_OWNER_HASH, max_ids=MAX_IDS, peer_capacity=CAP))
  return vs, ss, shs


def _phase_lookup(ops, sh, ids):
  sh.lookup_route(ids)
  ops.kv_shard_exchange_local([sh], 0)
  sh.lookup_serve()
  ops.kv_shard_exchange_local([sh], 1)
  return sh.lookup_finish()


def _phase_apply(ops, sh, slot, grad):
  sh.apply_route(grad)                     # (table 3: an empty batch, a null gradient)
  ops.kv_shard_exchange_local([sh], 1)
  sh.apply_serve(ops.OPT_GROUP_ADAM_V4, [slot], HP)


def _export(ops, h):
  k, v = ops.read_kv_variable_op_v2(h)
  o = torch.argsort(k)
  return k[o].cpu().numpy(), v[o].cpu().numpy()


@pytest.mark.parametrize("D", [4, 12])
def test_grouped_and_single_forms_of_the_phases_agree(ops, D):
  from tfplus_amd import _lib as L
  rng = np.random.default_rng(40 + D)
  dims = (D, D, 16 - D, D)
  multi, twin = _tables(ops, dims), _tables(ops, dims)
  comm = ops.KvComm(1, 0, None)
  batches = [rng.integers(0, 200, n) for n in NS]
  for b in batches[:3]:
    cnt = np.unique(b, return_counts=True)[1]
    assert (cnt == 1).any() and (cnt > 1).any()                    # ids that occur once, and repeats
  ids = [torch.from_numpy(b).cuda() for b in batches]
  sign = rng.choice([-1.0, 1.0], (1, 12))                          # one sign per element: sums of repeated ids do not cancel
  grads = [torch.from_numpy((rng.uniform(0.5, 1.5, (n, d)) * 1e-2 * sign[:, :d]).astype(np.float32)).cuda() for n, d in zip(NS, dims)]
  # 1. the whole ops against the phase calls
  outs = ops.kv_multi_shard_lookup(multi[2], comm, ids)
  for k in range(4):
    want = _phase_lookup(ops, twin[2][k], ids[k])
    assert outs[k].shape == (NS[k], dims[k]) and torch.equal(outs[k], want), k
  ops.kv_multi_shard_apply(multi[2], comm, ops.OPT_GROUP_ADAM_V4, [[s] for s in multi[1]], grads, HP)
  for k in range(4):
    _phase_apply(ops, twin[2][k], twin[1][k], grads[k])
  torch.cuda.synchronize()
  for k in range(4):
    once = np.unique(batches[k])[np.unique(batches[k], return_counts=True)[1] == 1]
    for a, b in ((multi[0][k], twin[0][k]), (multi[1][k], twin[1][k])):
      ka, va = _export(ops, a)
      kb, vb = _export(ops, b)
      np.testing.assert_array_equal(ka, kb)
      if a is multi[0][k]:
        np.testing.assert_array_equal(ka, np.unique(batches[k]))
      exact = np.ones(ka.size, bool) if DET[k] else np.isin(ka, once)
      assert np.array_equal(va[exact].view(np.uint32), vb[exact].view(np.uint32)), k
      np.testing.assert_allclose(va[~exact], vb[~exact], rtol=RTOL, atol=ATOL, err_msg=str(k))
    assert ops.kv_variable_frequency(multi[0][k]) == ops.kv_variable_frequency(twin[0][k])
  # 2. the table whose batch was empty: there is no gradient to name, and nothing to sum
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  assert L.lib().kv_shard_apply_route(multi[2][3].ptr, None, st) == L.KV_OK
  # 3. a finish whose route index is not there.  A shard's route table is its own, so the only route that can come between
  # a route and its finish is the shard's own next one; one that is refused after it began — under a stream capture, because
  # the batch is longer than any before and the route table's workspace would have to grow — leaves no index behind.
  sh = multi[2][0]
  big = torch.arange(MAX_IDS, dtype=torch.int64, device="cuda") % 50
  torch.cuda.synchronize()
  s0 = torch.cuda.Stream()
  s0.wait_stream(torch.cuda.current_stream())
  g0 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g0, stream=s0):
    with pytest.raises(L.FailedPreconditionError, match="workspace has to grow"):
      sh.lookup_route(big)
  torch.cuda.synchronize()
  with pytest.raises(L.FailedPreconditionError, match="without kv_shard_lookup_route"):
    sh.lookup_finish()
  with pytest.raises(L.FailedPreconditionError, match="lookup must come first"):
    sh.apply_route(torch.zeros((MAX_IDS, D), device="cuda"))
  # ... and the shard's next route is a route like any other
  assert torch.equal(_phase_lookup(ops, sh, ids[0]), ops.kv_variable_gather_or_zeros_v2(multi[0][0], ids[0]))
  # 4. kv_shard_apply_route behind kv_shard_lookup_zeros is refused: asserted in
  # tests/test_gpu_shard_lookup_zeros.py::test_pending_batches_and_the_refused_apply (and, for a rank whose batch was empty,
  # in tests/test_gpu_fuzz_sharded.py)
  torch.cuda.synchronize()
  del comm
