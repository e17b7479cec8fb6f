"""The N > 1 path with the REAL GPU pieces (kv_unique, kv_bucket_by_owner, kv_dedup_segment_sum,
kv_take_rows, HBM table shards) at world_size 2 on one GPU: two processes share cuda:0, the
all_to_all is staged through gloo on the host (RCCL refuses two ranks on one device), everything
else is the product path.  Checked against ONE unsharded oracle table fed every rank's ids."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY = 20000


def _a2a_via_host(out, inp, output_split_sizes=None, input_split_sizes=None, group=None):
  o = torch.empty(out.shape, dtype=out.dtype)
  dist.all_to_all_single(o, inp.cpu(), output_split_sizes=output_split_sizes, input_split_sizes=input_split_sizes,
                         group=group)
  out.copy_(o)


def _worker(rank, world, port, q, D, rule):
  sys.path.insert(0, ROOT)
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from oracle import kv_oracle as ko
    from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops, sharded

    class _Dist(object):  # sharded.py's `dist`, with the exchange staged through the host
      get_world_size = staticmethod(dist.get_world_size)
      get_rank = staticmethod(dist.get_rank)
      all_to_all_single = staticmethod(_a2a_via_host)
    sharded.dist = _Dist

    rng = np.random.default_rng(5)
    table = rng.standard_normal((64, D)).astype(np.float32)
    var = ops.kv_variable([D]); slot = ops.kv_variable([3 * D])
    for h, t in ((var, table), (slot, np.zeros((4, 3 * D), np.float32))):
      ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)

    class Shard(object):
      def sparse_read_with_counts(self, ids, counts=None):
        return ops.kv_variable_gather_or_insert_with_counts(var, ids, counts) if counts is not None \
            else ops.kv_variable_gather_or_insert_v2(var, ids)

      def sparse_read_pairs(self, pairs):
        return ops.kv_variable_gather_or_insert_pairs(var, pairs)

      def apply(self, g, ids):
        ops.kv_variable_group_sparse_apply_adam_v4(var, slot, g, ids, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)

    rule_id = {"hash": ops.KV_OWNER_HASH, "mod": ops.KV_OWNER_MOD}[rule]
    sh = sharded.ShardedKvVariable(Shard(), owner_rule=rule,
                                   bucket_fn=lambda i, w, nd=None, c=None: ops.kv_bucket_by_owner(var, i, w, nd, c, with_payload=nd is not None, owner_rule=rule_id),
                                   unique_fn=lambda i, c: ops.kv_unique(var, i, c),
                                   segsum_fn=lambda i, g: ops.kv_dedup_segment_sum(var, i, g),
                                   take_fn=ops.kv_take_rows,
                                    index_sum_fn=lambda g, i, n: ops.kv_unsorted_segment_sum(var, g, i, n),
                                    unique_async_fn=lambda i, c: ops.kv_unique(var, i, c, sync=False))
    ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)          # the unsharded truth, same on every rank
    rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
    for step in range(4):
      batches = [rng.integers(-400, 400, 3000 + 517 * r) for r in range(world)]   # heavy repeats, negative ids
      # one-signed gradients: the summed gradient of a repeated id never cancels to ~epsilon, where
      # Adam's quotient would amplify the order-dependent fp32 rounding of the per-rank partial sums
      sign = rng.choice([-1.0, 1.0], (1, D))
      grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2 * sign).astype(np.float32) for b in batches]
      mine = torch.from_numpy(batches[rank]).cuda()
      out = sh.lookup(mine).cpu().numpy()
      want_all = ref.gather_or_insert(np.concatenate(batches))
      off = sum(b.size for b in batches[:rank])
      want = want_all[off:off + mine.numel()]
      if step == 0:
        np.testing.assert_array_equal(out, want)                        # rows are copies
      else:
        np.testing.assert_allclose(out, want, rtol=2e-5, atol=2e-6)     # per-rank partial sums: fp32 order
      sh.apply_gradients(lambda shard, g, i: shard.apply(g, i), torch.from_numpy(grads[rank]).cuda(), mine)
      u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
      ko.apply_group_adam(ref, rslot, s, u, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8)
      keys, vals = ops.read_kv_variable_op_v2(var)
      keys = keys.cpu().numpy()
      own = lambda k: sharded.owner_of(torch.from_numpy(np.asarray(k, np.int64)), world, rule).numpy()
      assert keys.size and np.all(own(keys) == rank)                    # ownership: the rule, negatives included
      if rule == "mod":
        assert np.all(np.mod(keys, world) == rank)                      # floor-mod: the reference's partition
      allk = np.array(sorted(ref.as_dict()), np.int64)
      mine_ref = {int(k): ref.as_dict()[int(k)] for k in allk[own(allk) == rank]}
      assert set(keys.tolist()) == set(mine_ref)
      got = dict(zip(keys.tolist(), vals.cpu().numpy()))
      for k in mine_ref:
        np.testing.assert_allclose(got[k], mine_ref[k], rtol=2e-5, atol=2e-6)
      tot = torch.tensor([ops.kv_variable_frequency(var)])
      dist.all_reduce(tot)
      assert int(tot) == ref.sum_freq()                                 # every occurrence counted exactly once
    q.put((rank, "ok"))
  except Exception:  # pragma: no cover
    import traceback
    q.put((rank, traceback.format_exc()))
  finally:
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,D,rule", [(2, 16, "hash"), (4, 64, "mod")])      # (4, 64): configs[3]'s shape — dim 64, more than two owners
def test_sharded_world2_on_one_gpu(world, D, rule):
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  port = s.getsockname()[1]
  s.close()
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  procs = [ctx.Process(target=_worker, args=(r, world, port, q, D, rule)) for r in range(world)]
  for p in procs:
    p.start()
  res = [q.get(timeout=300) for _ in procs]
  for p in procs:
    p.join(timeout=60)
  assert all(r[1] == "ok" for r in res), res


# ---- the native path: kv_shard_* phases, fixed-capacity segments, no host synchronisation -----------------
def _native_setup(world, D, rule, table, cap=0, max_ids=1 << 14, det=False):
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  rule_id = {"hash": ops.KV_OWNER_HASH, "mod": ops.KV_OWNER_MOD}[rule]
  vars_, slots, shards = [], [], []
  for r in range(world):
    var = ops.kv_variable([D]); slot = ops.kv_variable([3 * D])
    for h, t in ((var, table), (slot, np.zeros((4, 3 * D), np.float32))):
      ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)
    if det:   # the four-kernel stable routing instead of the fused one
      ops.kv_set_deterministic(var, True); ops.kv_set_deterministic(slot, True)
    vars_.append(var); slots.append(slot)
    shards.append(ops.KvShard(var, world, r, rule_id, max_ids=max_ids, peer_capacity=cap))
  return ops, vars_, slots, shards


@pytest.mark.gpu
@pytest.mark.parametrize("world,D,rule,det", [(2, 16, "hash", False), (4, 64, "hash", True), (4, 64, "mod", False),
                                              (8, 32, "hash", False)])
def test_native_shard_phases_match_one_unsharded_table(world, D, rule, det):
  """`world` shards of one table in one process on one device: route -> exchange -> serve -> exchange -> finish and
  the apply's route -> exchange -> serve, against ONE oracle table fed every rank's ids (kvhip.h kv_shard_*)."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  from oracle import kv_oracle as ko
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(11)
  table = rng.standard_normal((64, D)).astype(np.float32)
  ops, vars_, slots, shards = _native_setup(world, D, rule, table, det=det)
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
  b1p, b2p = np.float32(0.9), np.float32(0.999)
  for step in range(4):
    batches = [rng.integers(-400, 400, 3000 + 517 * r) for r in range(world)]
    if step == 3:
      batches[world - 1] = batches[world - 1][:0]                         # a rank with an empty batch
    sign = rng.choice([-1.0, 1.0], (1, D))
    grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2 * sign).astype(np.float32) for b in batches]
    for r in range(world):
      shards[r].lookup_route(torch.from_numpy(batches[r]).cuda())
    ops.kv_shard_exchange_local(shards, 0)
    for r in range(world):
      shards[r].lookup_serve()
    ops.kv_shard_exchange_local(shards, 1)
    outs = [shards[r].lookup_finish().cpu().numpy() for r in range(world)]
    want_all = ref.gather_or_insert(np.concatenate(batches))
    off = 0
    for r in range(world):
      want = want_all[off:off + batches[r].size]
      off += batches[r].size
      if step == 0:
        np.testing.assert_array_equal(outs[r], want)                      # rows are copies
      else:
        np.testing.assert_allclose(outs[r], want, rtol=2e-5, atol=2e-6)   # per-rank partial sums: fp32 order
    for r in range(world):
      shards[r].apply_route(torch.from_numpy(grads[r]).cuda())
    ops.kv_shard_exchange_local(shards, 1)
    hp = (0.1, b1p, b2p, 0.9, 0.999, 1e-8, 0, 0, 0)
    for r in range(world):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], hp)
    u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
    ko.apply_group_adam(ref, rslot, s, u, 0.1, float(b1p), float(b2p), 0.9, 0.999, 1e-8)
    allk = np.array(sorted(ref.as_dict()), np.int64)
    own = sharded.owner_of(torch.from_numpy(allk), world, rule).numpy()    # the torch statement of the rule
    total = 0
    for r in range(world):
      keys, vals = ops.read_kv_variable_op_v2(vars_[r])
      keys = keys.cpu().numpy()
      assert set(keys.tolist()) == set(allk[own == r].tolist())           # every key lives on its owner, only there
      got = dict(zip(keys.tolist(), vals.cpu().numpy()))
      for k in keys.tolist():
        np.testing.assert_allclose(got[k], ref.as_dict()[k], rtol=2e-5, atol=2e-6)
      total += ops.kv_variable_frequency(vars_[r])
    assert total == ref.sum_freq()                                        # every occurrence counted exactly once


@pytest.mark.gpu
def test_native_shard_segment_overflow_is_reported_late_and_once():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D, world = 16, 2
  table = np.ones((4, D), np.float32)
  ops, vars_, slots, shards = _native_setup(world, D, "mod", table, cap=16, max_ids=4096)
  ids = torch.arange(0, 400, 2, dtype=torch.int64).cuda()                  # 200 distinct ids, all owned by rank 0
  for r in range(world):
    shards[r].lookup_route(ids)
  ops.kv_shard_exchange_local(shards, 0)
  for r in range(world):
    shards[r].lookup_serve()
  ops.kv_shard_exchange_local(shards, 1)
  out = shards[0].lookup_finish().cpu().numpy()
  assert np.count_nonzero(out.any(axis=1)) == 16                           # the surplus read zeros
  torch.cuda.synchronize()
  # reported by the next call — after that call has queued all its work, so a reporting rank keeps step with its peers
  with pytest.raises(Exception, match="peer_capacity"):
    shards[0].lookup_route(ids[:8])
  with pytest.raises(Exception, match="peer_capacity"):
    shards[1].lookup_route(ids[:0])                                       # shard 1 routed the same ids: its own report
  ops.kv_shard_exchange_local(shards, 0)                                  # the reporting calls' records are there
  for r in range(world):
    shards[r].lookup_serve()
  ops.kv_shard_exchange_local(shards, 1)
  out = shards[0].lookup_finish().cpu().numpy()
  assert out.shape == (8, D) and np.count_nonzero(out.any(axis=1)) == 8
  shards[0].lookup_route(ids[:8])                                         # reported once


@pytest.mark.gpu
def test_native_shard_lossless_mode_grows_the_capacity_on_every_shard():
  """kv_shard_set_lossless: after the routes the shards agree on the largest segment any of them wanted; it exceeds
  peer_capacity (16) here, so every shard raises its capacity to the same value and routes again — no id reads zeros,
  no gradient is dropped, nothing is reported late, and the state equals ONE unsharded oracle table."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  from oracle import kv_oracle as ko
  D, world = 16, 2
  rng = np.random.default_rng(3)
  table = rng.standard_normal((32, D)).astype(np.float32)
  ops, vars_, slots, shards = _native_setup(world, D, "mod", table, cap=16, max_ids=4096)
  for sh in shards:
    sh.set_lossless(True)
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
  caps = []
  for step in range(3):
    # rank 0's batch: 200 .. 600 distinct even ids (all owned by rank 0); rank 1's: a few odd ones
    batches = [np.arange(0, 400 * (step + 1), 2, dtype=np.int64), rng.integers(0, 50, 40) * 2 + 1]
    grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2).astype(np.float32) for b in batches]
    for r in range(world):
      shards[r].lookup_route(torch.from_numpy(batches[r]).cuda())
    if ops.kv_shard_agree_local(shards):                                   # raised on every shard: route again
      for r in range(world):
        shards[r].lookup_route(torch.from_numpy(batches[r]).cuda())
      assert not ops.kv_shard_agree_local(shards)
    caps.append(shards[0].peer_capacity)
    assert shards[1].peer_capacity == caps[-1] >= batches[0].size
    ops.kv_shard_exchange_local(shards, 0)
    for r in range(world):
      shards[r].lookup_serve()
    ops.kv_shard_exchange_local(shards, 1)
    want = ref.gather_or_insert(np.concatenate(batches))
    off = 0
    for r in range(world):
      got = shards[r].lookup_finish().cpu().numpy()
      np.testing.assert_allclose(got, want[off:off + batches[r].size], rtol=2e-5, atol=2e-6)   # every row is there
      assert np.count_nonzero(got.any(axis=1)) == batches[r].size
      off += batches[r].size
    for r in range(world):
      shards[r].apply_route(torch.from_numpy(grads[r]).cuda())
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0))
    u, s_, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
    ko.apply_group_adam(ref, rslot, s_, u, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8)
  assert caps[0] > 16 and caps[2] > caps[0]                                # grew twice (200 ids, then 600)
  torch.cuda.synchronize()
  keys, vals = ops.read_kv_variable_op_v2(vars_[0])
  refd = ref.as_dict()
  even = sorted(k for k in refd if k % 2 == 0)
  assert sorted(keys.cpu().tolist()) == even
  o = torch.argsort(keys)
  np.testing.assert_allclose(vals[o].cpu().numpy(), np.stack([refd[k] for k in even]), rtol=2e-5, atol=2e-6)
  shards[0].lookup_route(torch.arange(4, dtype=torch.int64).cuda())        # no late report: nothing was dropped


@pytest.mark.gpu
def test_native_shard_lossless_whole_op_through_rccl():
  """The whole op on a world of one through RCCL (ncclAllReduce of the needed capacity, grouped send / recv): a batch
  of 5000 distinct ids against peer_capacity 16 comes back complete and equals the unsharded ops."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D = 16
  rng = np.random.default_rng(9)
  table = rng.standard_normal((32, D)).astype(np.float32)
  ops, vars_, slots, shards = _native_setup(1, D, "hash", table, cap=16, max_ids=1 << 14)
  var2 = ops.kv_variable([D]); slot2 = ops.kv_variable([3 * D])
  for h, t in ((var2, table), (slot2, np.zeros((4, 3 * D), np.float32))):
    ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)
  # (no set_lossless call: lossless is the library's DEFAULT — VERDICT r3 item 6 — a batch that overflows the capacity
  #  grows it on every rank and is routed again: no zero rows, no dropped gradients)
  comm = ops.KvComm(1, 0, ops.kv_comm_unique_id(), self_via_rccl=True)
  hp = (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
  for step, n in enumerate((5000, 12000, 300)):
    ids = torch.from_numpy(rng.choice(100000, n, replace=False)).cuda()
    g = torch.from_numpy((rng.uniform(0.5, 1.5, (n, D)) * 1e-2).astype(np.float32)).cuda()
    out = shards[0].lookup(comm, ids)
    assert torch.equal(out, ops.kv_variable_gather_or_insert_v2(var2, ids))     # distinct ids: rows are copies
    assert shards[0].peer_capacity >= min(n, 12000 if step else 5000)
    shards[0].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[0]], g, hp)
    ops.kv_variable_group_sparse_apply_adam_v4(var2, slot2, g, ids, *hp)
  torch.cuda.synchronize()
  k1, v1 = ops.read_kv_variable_op_v2(vars_[0]); k2, v2 = ops.read_kv_variable_op_v2(var2)
  o1, o2 = torch.argsort(k1), torch.argsort(k2)
  assert torch.equal(k1[o1], k2[o2])
  torch.testing.assert_close(v1[o1], v2[o2], rtol=1e-6, atol=1e-7)              # unique ids: the op boundary's tolerance
  del comm


@pytest.mark.gpu
def test_native_shard_lossy_mode_is_the_opt_in():
  """kv_shard_set_lossless(shard, 0): the synchronisation-free mode — a batch that sends one owner more than
  peer_capacity distinct ids reads zeros for the surplus and the NEXT sharded call reports it; the default mode (the
  test above) grows the capacity instead."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D = 16
  table = np.ones((4, D), np.float32)
  ops, vars_, slots, shards = _native_setup(1, D, "hash", table, cap=16, max_ids=4096)
  shards[0].set_lossless(False)
  comm = ops.KvComm(1, 0, ops.kv_comm_unique_id(), self_via_rccl=True)
  ids = torch.arange(0, 200, dtype=torch.int64).cuda()
  out = shards[0].lookup(comm, ids).cpu().numpy()
  assert np.count_nonzero(out.any(axis=1)) == 16 and shards[0].peer_capacity == 16
  torch.cuda.synchronize()
  with pytest.raises(Exception, match="peer_capacity"):
    shards[0].lookup(comm, ids[:8])
  out = shards[0].lookup(comm, ids[:8]).cpu().numpy()                       # reported once; this batch fits
  assert np.count_nonzero(out.any(axis=1)) == 8
  del comm


@pytest.mark.gpu
def test_native_shard_full_capacity_cannot_overflow():
  """peer_capacity = max_ids: the worst case — every distinct id of a full batch owned by ONE rank — fits; nothing is
  dropped, nothing is reported (the lossless setting; it costs world x the wire bytes)."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D, world = 16, 2
  table = np.ones((4, D), np.float32)
  ops, vars_, slots, shards = _native_setup(world, D, "mod", table, cap=4096, max_ids=4096)
  ids = torch.arange(0, 8192, 2, dtype=torch.int64).cuda()                 # 4096 distinct ids, all owned by rank 0
  for step in range(2):
    for r in range(world):
      shards[r].lookup_route(ids)
    ops.kv_shard_exchange_local(shards, 0)
    for r in range(world):
      shards[r].lookup_serve()
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      out = shards[r].lookup_finish()
      assert torch.equal(out, torch.ones(4096, D, device="cuda")) if step == 0 else bool(out.any(dim=1).all())
    for r in range(world):
      shards[r].apply_route(torch.full((4096, D), 0.25, device="cuda"))
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0))
    torch.cuda.synchronize()
  assert ops.kv_variable_size_v2(vars_[0]) == 4096 and ops.kv_variable_size_v2(vars_[1]) == 0
  # both ranks sent + 0.25 per id and element: all 4096 keys took the same two updates, none was dropped
  k, v = ops.read_kv_variable_op_v2(vars_[0])
  assert k.numel() == 4096 and bool((v == v[0, 0]).all()) and float(v[0, 0]) != 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("with_rccl", [False, True])
def test_native_shard_world_of_one_equals_the_unsharded_ops(with_rccl):
  """kv_shard_lookup / kv_shard_apply as whole ops (forked stream, RCCL grouped send / recv when asked for) on a world
  of one: same rows, same table as the plain ops on a second table."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D = 32
  rng = np.random.default_rng(4)
  table = rng.standard_normal((64, D)).astype(np.float32)
  ops, vars_, slots, shards = _native_setup(1, D, "hash", table, max_ids=1 << 15)
  var2 = ops.kv_variable([D]); slot2 = ops.kv_variable([3 * D])
  for h, t in ((var2, table), (slot2, np.zeros((4, 3 * D), np.float32))):
    ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)
    ops.kv_set_deterministic(h, True)
  for h in (vars_[0], slots[0]):
    ops.kv_set_deterministic(h, True)
  # with_rccl: the self segment through grouped ncclSend / ncclRecv as a peer's would go
  comm = ops.KvComm(1, 0, ops.kv_comm_unique_id() if with_rccl else None, self_via_rccl=with_rccl)
  for step in range(3):
    ids = torch.from_numpy(rng.integers(0, 5000, 20000)).cuda()
    g = torch.from_numpy((rng.standard_normal((20000, D)) * 1e-2).astype(np.float32)).cuda()
    if step == 1:     # deferred join: the caller's stream waits only when it needs the rows
      out = shards[0].lookup(comm, ids, join=False)
      shards[0].join()
    else:
      out = shards[0].lookup(comm, ids)
    want = ops.kv_variable_gather_or_insert_v2(var2, ids)
    if step == 0:
      assert torch.equal(out, want)
    else:   # two states that already differ by the order of their sums; the per-step bound below is the real check
      torch.testing.assert_close(out, want, rtol=1e-3, atol=1e-4)
    # the two paths sum a repeated id's gradients (two-signed here) in different fp32 orders — local pre-sum then the
    # owner's sum, against tile sums then the key's entries: each is held to the float64 update of ITS OWN state before
    # the step, within the per-element reorder bound (tests/_reorder.py), not to a blanket rtol
    from _reorder import adam_hp, adam_reorder_check
    u = torch.unique(ids)
    pre = []
    for hv, hs in ((vars_[0], slots[0]), (var2, slot2)):
      st = ops.kv_variable_gather_or_zeros_v2(hs, u).cpu().numpy()
      pre.append((ops.kv_variable_gather_or_zeros_v2(hv, u).cpu().numpy(), st[:, :D], st[:, D:2 * D], st[:, 2 * D:]))
    shards[0].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[0]], g, (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0))
    ops.kv_variable_group_sparse_apply_adam_v4(var2, slot2, g, ids, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
    hp = adam_hp(0.1, 0.9, 0.999)
    for (x0, m0, v0, z0), hv, name in zip(pre, (vars_[0], var2), ("sharded", "unsharded")):
      x1 = ops.kv_variable_gather_or_zeros_v2(hv, u).cpu().numpy()
      adam_reorder_check(x0, m0, v0, z0, ids.cpu().numpy(), g.cpu().numpy(), x1, hp, what="%s step %d" % (name, step))
    k1, v1 = ops.read_kv_variable_op_v2(vars_[0]); k2, v2 = ops.read_kv_variable_op_v2(var2)
    assert torch.equal(torch.sort(k1).values, torch.sort(k2).values)
  del comm


@pytest.mark.gpu
def test_native_shard_a_failing_rank_still_queues_its_exchanges():
  """A phase that fails on THIS rank (a batch longer than max_ids) returns its error only after the exchanges were
  queued — void headers, zero rows — so peers are not left waiting in a grouped recv; the table is untouched and the
  next batch runs as if nothing had happened."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  D = 16
  table = np.ones((4, D), np.float32)
  ops, vars_, slots, shards = _native_setup(1, D, "hash", table, max_ids=1024)
  comm = ops.KvComm(1, 0, ops.kv_comm_unique_id(), self_via_rccl=True)
  good = torch.arange(100, dtype=torch.int64).cuda()
  out = shards[0].lookup(comm, good)
  assert torch.equal(out, torch.ones(100, D, device="cuda"))
  with pytest.raises(Exception, match="queued all the same"):
    shards[0].lookup(comm, torch.arange(5000, dtype=torch.int64).cuda())
  # the failed batch left an empty route: its apply exchanges void records and changes nothing
  shards[0].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[0]], torch.ones(5000, D, device="cuda"), (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0))
  torch.cuda.synchronize()
  assert ops.kv_variable_size_v2(vars_[0]) == 100                    # nothing of the failed batch reached the table
  assert torch.equal(ops.kv_variable_gather_or_zeros_v2(vars_[0], good), torch.ones(100, D, device="cuda"))
  out = shards[0].lookup(comm, good)
  shards[0].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[0]], torch.full((100, D), 0.5, device="cuda"), (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0))
  torch.cuda.synchronize()
  assert torch.equal(out, torch.ones(100, D, device="cuda")) and ops.kv_variable_size_v2(vars_[0]) == 100
  del comm


@pytest.mark.gpu
def test_native_shard_refuses_a_dim_the_entry_list_kernels_do_not_serve():
  """kv_shard_create takes the dims its route, finish and owner kernels serve — multiples of 4 up to 256 — and refuses
  the rest with KV_UNIMPLEMENTED."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  import ctypes
  from tfplus_amd import _lib
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  for D, ok in ((256, True), (260, False), (512, False)):
    hv = ops.kv_variable([D])
    ops.init_kv_variable_v2(hv, np.zeros((4, D), np.float32))
    sh = ctypes.c_void_p()
    rc = _lib.lib().kv_shard_create(hv.ptr, 2, 0, 0, 1 << 16, 0, ctypes.byref(sh))
    if ok:
      assert rc == 0, _lib.lib().kv_last_error()
      assert _lib.lib().kv_shard_destroy(sh) == 0
    else:
      assert rc == _lib.KV_UNIMPLEMENTED and "up to 256" in _lib.lib().kv_last_error().decode(), (D, rc)


@pytest.mark.gpu
def test_comm_self_via_rccl_needs_an_rccl_communicator():
  """kv_comm_set_self_via_rccl is a setting of one communicator: KV_INVALID_ARGUMENT on one without RCCL."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  from tfplus_amd import _lib
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  comm = ops.KvComm(1, 0, None)
  assert _lib.lib().kv_comm_set_self_via_rccl(comm.ptr, 1) == _lib.KV_INVALID_ARGUMENT
  with pytest.raises(Exception):
    ops.KvComm(1, 0, None, self_via_rccl=True)
  del comm


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam_v3", "adagrad", "ftrl"])
def test_native_shard_every_optimizer_matches_the_unsharded_oracle(opt):
  """kv_shard_apply_serve's other optimizers (GroupAdam V3, Adagrad, SparseGroupFtrl with its two slot tables)
  through route -> exchange -> serve on 3 shards, against ONE unsharded oracle table."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  from oracle import kv_oracle as ko
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops, sharded
  world, D = 3, 16
  rng = np.random.default_rng(23)
  table = rng.standard_normal((64, D)).astype(np.float32)
  slot_dims = {"adam_v3": [3 * D], "adagrad": [D], "ftrl": [D, D]}[opt]
  slot_init = {"adam_v3": [0.0], "adagrad": [0.1], "ftrl": [0.1, 0.0]}[opt]
  vars_, slots, shards = [], [], []
  for r in range(world):
    var = ops.kv_variable([D])
    ops.kv_set_clock_days(var, DAY); ops.kv_set_seed(var, 3); ops.init_kv_variable_v2(var, table)
    ss = []
    for d, v in zip(slot_dims, slot_init):
      s = ops.kv_variable([d])
      ops.kv_set_clock_days(s, DAY); ops.kv_set_seed(s, 3); ops.init_kv_variable_v2(s, np.full((4, d), v, np.float32))
      ss.append(s)
    vars_.append(var); slots.append(ss)
    shards.append(ops.KvShard(var, world, r, ops.KV_OWNER_HASH, max_ids=1 << 14))
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  rslots = [ko.OracleKv(d, 0, np.full((4, d), v, np.float32), day=DAY) for d, v in zip(slot_dims, slot_init)]
  b1p, b2p = np.float32(0.9), np.float32(0.999)
  for step in range(3):
    batches = [rng.integers(-300, 300, 2000 + 311 * r) for r in range(world)]
    sign = rng.choice([-1.0, 1.0], (1, D))
    grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2 * sign).astype(np.float32) for b in batches]
    for r in range(world):
      shards[r].lookup_route(torch.from_numpy(batches[r]).cuda())
    ops.kv_shard_exchange_local(shards, 0)
    for r in range(world):
      shards[r].lookup_serve()
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      shards[r].lookup_finish()
    ref.gather_or_insert(np.concatenate(batches))
    for r in range(world):
      shards[r].apply_route(torch.from_numpy(grads[r]).cuda())
    ops.kv_shard_exchange_local(shards, 1)
    u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
    if opt == "adam_v3":
      hp, code = (0.1, b1p, b2p, 0.9, 0.999, 1e-8, 1e-4, 1e-3, 1e-3), ops.OPT_GROUP_ADAM_V3
      ko.apply_group_adam(ref, rslots[0], s, u, 0.1, float(b1p), float(b2p), 0.9, 0.999, 1e-8, 1e-4, 1e-3, 1e-3, version=3)
      b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.999))
    elif opt == "adagrad":
      hp, code = (0.05, 1.0), ops.OPT_ADAGRAD
      ko.apply_adagrad(ref, rslots[0], 0.05, s, u, True)
    else:
      hp, code = (0.1, 1e-3, 1e-3, 1e-3, 0.0, -0.5), ops.OPT_SPARSE_GROUP_FTRL
      ko.apply_sparse_group_ftrl(ref, rslots[0], rslots[1], s, u, 0.1, 1e-3, 1e-3, 1e-3, 0.0, -0.5)
    for r in range(world):
      shards[r].apply_serve(code, slots[r], hp)
    allk = np.array(sorted(ref.as_dict()), np.int64)
    own = sharded.owner_of(torch.from_numpy(allk), world, "hash").numpy()
    for r in range(world):
      keys, vals = ops.read_kv_variable_op_v2(vars_[r])
      keys = keys.cpu().numpy()
      assert set(keys.tolist()) <= set(allk[own == r].tolist())          # blacklisted rows are not exported
      got = dict(zip(keys.tolist(), vals.cpu().numpy()))
      want = ref.as_dict()
      for k in keys.tolist():
        np.testing.assert_allclose(got[k], want[k], rtol=3e-5, atol=3e-6)
      # the rows a lookup returns (zeros for blacklisted keys) agree for every key of the shard
      mine = allk[own == r]
      np.testing.assert_allclose(ops.kv_variable_gather_or_zeros_v2(vars_[r], mine).cpu().numpy(), ref.gather_or_zeros(mine),
                                 rtol=3e-5, atol=3e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("world,D,lossless,cap", [(2, 16, False, 0), (4, 32, True, 48), (3, 8, True, 0)])
def test_whole_ops_with_ranks_as_threads_match_one_unsharded_table(world, D, lossless, cap):
  """kv_shard_lookup / kv_shard_apply — the ops a real run calls — with `world` ranks as THREADS of this process, each
  with its own tables, shard and a staged communicator (kv_comm_create_staged) whose callbacks move the segments
  between the ranks' buffers on the device.  Unlike the phase tests this runs the whole-op code of every rank > 0: the
  first-exchange verification, the lossless agreement (the capacity grows on every rank at once), the rank's own segment
  read in place (the transport does NOT deliver it: it poisons that part of the receive buffer), the forked stream.
  Checked against ONE oracle table fed every rank's ids."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  import threading
  sys.path.insert(0, ROOT)
  from oracle import kv_oracle as ko
  from tfplus_amd.kv_variable.python.ops import sharded
  import _hash_keys as hk
  rng = np.random.default_rng(31 + world)
  table = rng.standard_normal((64, D)).astype(np.float32)
  ops, vars_, slots, shards = _native_setup(world, D, "hash", table, cap=cap, max_ids=1 << 14)
  for sh in shards:
    sh.set_lossless(lossless)
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
  dev = torch.device("cuda", 0)
  bar = threading.Barrier(world, timeout=120)
  sent = [None] * world
  vals = [0] * world

  def make_comm(r):
    def exchange(send, recv, per_peer):
      n = per_peer * world
      sent[r] = ops.KvCommStaged.raw(send, n, dev)
      torch.cuda.synchronize()
      bar.wait()
      dst = ops.KvCommStaged.raw(recv, n, dev)
      for p in range(world):
        if p == r and per_peer != 32:                            # (32 bytes: the first exchange's verification record)
          dst[p * per_peer:(p + 1) * per_peer].fill_(0xA5)      # never delivered: the ops read their own segment in place
        else:
          dst[p * per_peer:(p + 1) * per_peer].copy_(sent[p][r * per_peer:(r + 1) * per_peer])
      torch.cuda.synchronize()
      bar.wait()

    def max_u32(v):
      vals[r] = v
      bar.wait()
      m = max(vals)
      bar.wait()
      return m
    return ops.KvCommStaged(0, world=world, rank=r, exchange=exchange, max_u32=max_u32)

  comms = [make_comm(r) for r in range(world)]
  b1p, b2p = np.float32(0.9), np.float32(0.999)
  hp = (0.1, b1p, b2p, 0.9, 0.999, 1e-8, 0, 0, 0)
  for step in range(4):
    batches = [rng.integers(-300, 300, 2500 + 411 * r) for r in range(world)]
    if step == 2:
      batches[0] = batches[0][:0]                                           # a rank with an empty batch
    if step == 3:
      # keys crafted against the owner hash (tests/_hash_keys.py): rank 0's whole batch — 1500 keys, the edge keys INT64_MIN
      # (the index's sentinel: the route_seg .. EMPTY_KEY records of kv_papply.h), INT64_MAX, 0 and -1, with repeats —
      # belongs to ONE owner, the last rank (the edge keys to whoever owns them); rank 1 sends the sentinel key as well
      crafted = hk.case("D_w%d" % world)
      batches[0] = rng.permutation(np.concatenate([crafted, crafted[rng.integers(0, crafted.size, 700)],
                                                   np.repeat(np.array(hk.EDGE_KEYS, np.int64), 3)]))
      batches[1] = rng.permutation(np.concatenate([batches[1], np.full(3, hk.INT64_MIN, np.int64)]))
    sign = rng.choice([-1.0, 1.0], (1, D))
    grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2 * sign).astype(np.float32) for b in batches]
    outs, errs = [None] * world, []

    def rank_step(r):
      try:
        torch.cuda.set_device(0)
        o = shards[r].lookup(comms[r], torch.from_numpy(batches[r]).cuda())
        torch.cuda.synchronize()
        outs[r] = o.cpu().numpy()
        shards[r].apply(comms[r], ops.OPT_GROUP_ADAM_V4, [slots[r]], torch.from_numpy(grads[r]).cuda(), hp)
        torch.cuda.synchronize()
      except Exception as e:   # (a rank that fails breaks the barrier: the others fail too instead of waiting)
        errs.append((r, repr(e)))
        bar.abort()
    ts = [threading.Thread(target=rank_step, args=(r,)) for r in range(world)]
    for t in ts:
      t.start()
    for t in ts:
      t.join()
    assert not errs, errs
    bar.reset()
    want_all = ref.gather_or_insert(np.concatenate(batches))
    off = 0
    for r in range(world):
      want = want_all[off:off + batches[r].size]
      off += batches[r].size
      if step == 0:
        np.testing.assert_array_equal(outs[r], want)
      else:
        np.testing.assert_allclose(outs[r], want, rtol=2e-5, atol=2e-6)
    u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
    ko.apply_group_adam(ref, rslot, s, u, 0.1, float(b1p), float(b2p), 0.9, 0.999, 1e-8)
    allk = np.array(sorted(ref.as_dict()), np.int64)
    own = sharded.owner_of(torch.from_numpy(allk), world, "hash").numpy()
    total = 0
    for r in range(world):
      keys, vals_r = ops.read_kv_variable_op_v2(vars_[r])
      keys = keys.cpu().numpy()
      assert set(keys.tolist()) == set(allk[own == r].tolist())
      got = dict(zip(keys.tolist(), vals_r.cpu().numpy()))
      for k in keys.tolist():
        np.testing.assert_allclose(got[k], ref.as_dict()[k], rtol=2e-5, atol=2e-6)
      total += ops.kv_variable_frequency(vars_[r])
    assert total == ref.sum_freq()
  if lossless and cap:
    assert all(sh.peer_capacity > cap for sh in shards)                     # grown, on every rank alike
    assert len({sh.peer_capacity for sh in shards}) == 1
  assert all(c.exchanges >= 12 for c in comms)
  del comms


@pytest.mark.gpu
def test_shard_manifest_refuses_a_checkpoint_of_another_partitioning():
  """A sharded table's checkpoint is its ranks' exports plus the record of the partitioning they were written under:
  another world size, rank or owner rule (or the older arithmetic of the hash rule) is refused, not imported."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  sys.path.insert(0, ROOT)
  table = np.ones((4, 8), np.float32)
  ops, vars_, slots, shards = _native_setup(2, 8, "hash", table)
  m = shards[1].manifest()
  assert m == {"world": 2, "rank": 1, "owner_rule": "hash", "owner_rule_version": 2}
  shards[1].check_manifest(dict(m))
  for key, val in (("world", 4), ("rank", 0), ("owner_rule", "mod"), ("owner_rule_version", 1)):
    with pytest.raises(ValueError, match=key):
      shards[1].check_manifest(dict(m, **{key: val}))
