"""sharded.ShardedKvVariable.lookup_zeros on CPU: world_size 2, gloo, as tests/test_sharded_gloo.py — the exchange is the
product code, the rank-local shard is the CPU oracle, the truth is ONE unsharded oracle table.  The read-only lookup returns
that table's gather_or_zeros exactly, changes nothing on the shards, and leaves nothing a following apply_gradients could
take for the backward pass of a training lookup: that apply takes the long path and matches the unsharded oracle."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY, D = 20000, 8


class OracleShard(object):
  """KvVariable look-alike over the oracle: the training read, the read-only one, a GroupAdam apply"""

  def __init__(self, table):
    from oracle import kv_oracle as ko
    self.ko = ko
    self.var = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
    self.slot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
    self.applied = []

  def sparse_read_with_counts(self, ids, counts=None):
    c = None if counts is None else counts.numpy().astype(np.int32)
    return torch.from_numpy(self.var.gather_or_insert(ids.numpy(), c))

  def gather_or_zeros(self, ids):
    return torch.from_numpy(self.var.gather_or_zeros(ids.numpy()))

  def apply(self, grad, ids):
    self.applied.append(ids.clone())
    u, s, _ = self.ko.dedup_segment_sum(ids.numpy(), grad.numpy())
    self.ko.apply_group_adam(self.var, self.slot, s, u, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8)

  def counters(self):
    return self.var.size(), self.var.sum_freq(), self.var.map_size()


def _worker(rank, world, port, q, rule):
  sys.path.insert(0, ROOT)
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from tfplus_amd.kv_variable.python.ops import sharded
    rng = np.random.default_rng(19)
    table = rng.standard_normal((32, D)).astype(np.float32)
    sh = sharded.ShardedKvVariable(OracleShard(table), owner_rule=rule)
    ref = OracleShard(table)                                   # the unsharded truth, same on every rank
    own_of = lambda k: int(sharded.owner_of(torch.tensor([int(k)]), world, rule))
    # a training lookup fills the tables and leaves its backward state: what the read-only lookup must not leave standing
    batches = [torch.from_numpy(rng.integers(-50, 200, 90 + 17 * r)) for r in range(world)]
    sh.lookup(batches[rank])
    ref.sparse_read_with_counts(torch.cat(batches))
    assert sh._last is not None
    # the read-only lookup: held keys, absent ones (>= 1000 among them), repeats, a 2-D shape
    reads = [torch.from_numpy(np.concatenate([rng.integers(-60, 210, 120 + 8 * r), rng.integers(1000, 1050, 30)])).reshape(-1, 2)
             for r in range(world)]
    mine = reads[rank]
    before = sh.shard.counters()
    out = sh.lookup_zeros(mine)
    assert tuple(out.shape) == tuple(mine.shape) + (D,)
    want = torch.from_numpy(ref.var.gather_or_zeros(mine.numpy()))
    assert torch.equal(out, want)                              # ONE unsharded table's GatherOrZeros, exactly
    absent = mine.reshape(-1) >= 1000
    assert int(absent.sum()) == 30 and not out.reshape(-1, D)[absent].any() and bool(out.any())
    assert sh.shard.counters() == before                       # size, sum_freq, map_size: nothing inserted, nothing counted
    assert sh._last is None
    empty = sh.lookup_zeros(mine[:0] if rank == 0 else mine[:3])       # a rank with an empty batch
    assert tuple(empty.shape) == ((0, 2, D) if rank == 0 else (3, 2, D))
    assert sh.shard.counters() == before
    # apply_gradients with the very tensor of the read-only lookup: the long path (this batch's unique ids travel), never
    # the stale short one of the training lookup before it — and the state matches the unsharded oracle
    g = torch.from_numpy(rng.uniform(0.5, 1.5, (mine.numel(), D)).astype(np.float32) * 1e-2)
    both = [None] * world
    dist.all_gather_object(both, (mine.reshape(-1), g))
    sh.apply_gradients(lambda shard, gg, i: shard.apply(gg, i), g, mine)
    ref.apply(torch.cat([x[1] for x in both]), torch.cat([x[0] for x in both]))
    everyone = torch.unique(torch.cat([x[0] for x in both]))
    owned = everyone[sharded.owner_of(everyone, world, rule) == rank]
    assert sorted(torch.unique(sh.shard.applied[-1]).tolist()) == sorted(owned.tolist())   # the ids of THIS batch reached their owner
    keys, vals, *_ = sh.shard.var.export(2)
    assert all(own_of(k) == rank for k in keys)
    rk, rv, *_ = ref.var.export(2)
    want_own = {int(k): v for k, v in zip(rk, rv) if own_of(k) == rank}
    got = {int(k): v for k, v in zip(keys, vals)}
    assert set(want_own) == set(got)
    for k in want_own:                                         # tests/test_sharded_gloo.py's bar after an apply
      np.testing.assert_allclose(got[k], want_own[k], rtol=1e-5, atol=1e-6)
    cnt = torch.tensor([sh.shard.var.sum_freq()])
    dist.all_reduce(cnt)
    assert int(cnt) == ref.var.sum_freq()
    q.put((rank, "ok"))
  except Exception:  # pragma: no cover
    import traceback
    q.put((rank, traceback.format_exc()))
  finally:
    dist.destroy_process_group()


def _run(worker, rule):
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  port = s.getsockname()[1]
  s.close()
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  procs = [ctx.Process(target=worker, args=(r, 2, port, q, rule)) for r in range(2)]
  for p in procs:
    p.start()
  res = [q.get(timeout=240) for _ in procs]
  for p in procs:
    p.join(timeout=60)
  assert all(r[1] == "ok" for r in res), res


@pytest.mark.parametrize("rule", ["hash", "mod"])
def test_sharded_lookup_zeros_world2(rule):
  _run(_worker, rule)
