"""The read-only sharded lookup (kvhip.h kv_shard_lookup_serve_zeros / kv_shard_lookup_zeros / kv_multi_shard_lookup_zeros):
every id reads the bits kv_variable_gather_or_zeros_v2 returns on its OWNER's local table (rows are copies: array_equal),
agrees with ONE unsharded oracle table at test_gpu_sharded_two_ranks.py's bar (rtol 2e-5, atol 2e-6 after training steps — the
per-rank partial sums of the sharded apply take another fp32 order — exact after none; a row the oracle gives as zero is
exactly zero), and leaves the owners' tables bit-identical.  Shards are built as that file's _native_setup builds them:
`world` shards of one table in one process, kv_shard_exchange_local between the phases; the whole ops run with ranks as
threads over KvCommStaged."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ranks import Ranks as _Ranks  # noqa: E402  (ranks as threads, shared with tests/test_gpu_fuzz_sharded.py)

DAY, THR = 20000, 3
RTOL, ATOL = 2e-5, 2e-6
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _lib():
  from tfplus_amd import _lib as L
  return L


def _owner(ids, world, rule):
  from tfplus_amd.kv_variable.python.ops import sharded
  return sharded.owner_of(torch.from_numpy(np.asarray(ids, np.int64)), world, rule).numpy()


def _setup(ops, world, D, rule, table, thr=0, cap=0, max_ids=1 << 14, det=False, delta=False):
  """tests/test_gpu_sharded_two_ranks.py::_native_setup with an enter threshold and delta tracking"""
  rule_id = {"hash": ops.KV_OWNER_HASH, "mod": ops.KV_OWNER_MOD}[rule]
  vars_, slots, shards = [], [], []
  for r in range(world):
    var = ops.kv_variable([D], enter_threshold=thr); slot = ops.kv_variable([3 * D])
    for h, t in ((var, table), (slot, np.zeros((4, 3 * D), np.float32))):
      ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)
    if det:
      ops.kv_set_deterministic(var, True); ops.kv_set_deterministic(slot, True)
    if delta:
      ops.kv_set_delta_tracking(var, True)
    vars_.append(var); slots.append(slot)
    shards.append(ops.KvShard(var, world, r, rule_id, max_ids=max_ids, peer_capacity=cap))
  return vars_, slots, shards


def _read_phases(ops, shards, batches):
  """route -> exchange -> the read-only serve -> exchange -> finish, on every shard"""
  for sh, b in zip(shards, batches):
    sh.lookup_route(torch.from_numpy(np.asarray(b, np.int64)).cuda())
  ops.kv_shard_exchange_local(shards, 0)
  for sh in shards:
    sh.lookup_serve_zeros()
  ops.kv_shard_exchange_local(shards, 1)
  return [sh.lookup_finish().cpu().numpy() for sh in shards]


def _owner_reads(ops, vars_, ids, world, rule):
  """what kv_variable_gather_or_zeros_v2 on each id's owner's local table returns"""
  ids = np.asarray(ids, np.int64)
  out = np.empty((ids.size, vars_[0].dim), np.float32)
  own = _owner(ids, world, rule) if ids.size else np.zeros(0, np.int64)
  for o in range(world):
    if np.any(own == o):
      out[own == o] = ops.kv_variable_gather_or_zeros_v2(vars_[o], ids[own == o]).cpu().numpy()
  return out


def _check_rows(got, owner_rows, oracle_rows, trained):
  np.testing.assert_array_equal(got, owner_rows)                 # rows are copies of the owner's own read
  if trained:
    np.testing.assert_allclose(got, oracle_rows, rtol=RTOL, atol=ATOL)
  else:
    np.testing.assert_array_equal(got, oracle_rows)
  zero = ~oracle_rows.any(axis=1)
  assert not got[zero].any()                                     # exactly zero where the oracle reads zeros


# ---- cases 1 and 2: the phases against the owners' own reads; nothing changes -------------------------------------------
CASES = [(2, 16, "hash", False), (4, 64, "mod", True), (3, 12, "hash", False), (8, 32, "hash", False), (2, 4, "hash", False),
         (2, 256, "hash", False)]
HOT, COLD = np.arange(-150, 150), np.arange(1000, 1120)          # hot keys: many occurrences; cold: one, ever
ABSENT = np.arange(5000, 5100)                                    # never looked up in training


def _train_plan(world, D):
  """Two training steps.  Step 0 (plain GroupAdam) also meets every cold key once, on one rank: its frequency stays under
  the enter threshold of 3.  Step 1 is a GroupAdam step with l21 = 2e-2 (the regulariser case of tests/test_gpu_parity.py):
  the keys whose gradients are tiny (HOT[::2], scale 1e-5) fall under the group-lasso threshold and are blacklisted, those
  with scale 3e-2 stay far above it — no row near the threshold, where the oracle and the kernel may legitimately differ."""
  rng = np.random.default_rng(100 * world + D)
  scale = np.where((HOT - HOT[0]) % 2 == 0, 1e-5, 3e-2)
  steps = []
  for step in range(2):
    batches = [HOT[rng.integers(0, HOT.size, 1500 + 211 * r)] for r in range(world)]
    if step == 0:
      batches = [rng.permutation(np.concatenate([b, COLD[r::world]])) for r, b in enumerate(batches)]
    sign = rng.choice([-1.0, 1.0], (1, D))
    grads = []
    for b in batches:
      sc = np.where(b >= COLD[0], 1e-2, scale[np.clip(b - HOT[0], 0, HOT.size - 1)])
      grads.append((rng.uniform(0.5, 1.5, (b.size, D)) * sign * sc[:, None]).astype(np.float32))
    hp = (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0) if step == 0 else \
         (0.05, float(np.float32(0.9) ** 2), float(np.float32(0.999) ** 2), 0.9, 0.999, 1e-8, 1e-3, 1e-2, 2e-2)
    steps.append((batches, grads, hp))
  pool = np.concatenate([HOT, COLD, ABSENT])
  reads = [[pool[rng.integers(0, pool.size, 3000 + 13 + 22 * r)] for r in range(world)] for _ in range(2)]
  reads[1][world - 1] = reads[1][world - 1][:0]                   # one rank's batch is empty in one round
  return steps, reads


def _oracle_after(world, D, table):
  from oracle import kv_oracle as ko
  steps, reads = _train_plan(world, D)
  ref = ko.OracleKv(D, THR, table, day=DAY, picker=1, seed=3)
  rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
  for batches, grads, hp in steps:
    ref.gather_or_insert(np.concatenate(batches))
    u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
    ko.apply_group_adam(ref, rslot, s, u, *hp)
  return ref


def _states(ref, ids):
  """ids of the batch by state: held with a frequency over the enter threshold, held under it (LowFreq, kv_variable.h:910-912),
  blacklisted, absent"""
  st = {"over": 0, "under": 0, "black": 0, "absent": 0}
  for k in np.unique(ids):
    m = ref.meta(int(k))
    st["absent" if m is None else "black" if m["blacklist"] else "under" if m["freq"] < THR else "over"] += 1
  return st


def _export(ops, var):
  """the full export (first_n = 6), sorted by key"""
  k, v, bl, fk, fv = ops.kv_variable_export(var, first_n=6)
  o, fo = torch.argsort(k), torch.argsort(fk)
  return (k[o].cpu().numpy().tobytes(), v[o].cpu().numpy().tobytes(), np.sort(bl.cpu().numpy()).tobytes(),
          fk[fo].cpu().numpy().tobytes(), fv[fo].cpu().numpy().tobytes())


def _snapshot(ops, vars_, slots, ids):
  """everything of every rank's tables the read-only lookup must leave bit-identical"""
  L = _lib()
  ids_t = torch.from_numpy(np.unique(ids)).cuda()
  snap = []
  for var, slot in zip(vars_, slots):
    fw = torch.empty(ids_t.numel(), dtype=torch.int32, device="cuda")
    fl = torch.empty(ids_t.numel(), dtype=torch.uint8, device="cuda")
    L.check(L.lib().kv_get_meta(var.ptr, ids_t.data_ptr(), ids_t.numel(), fw.data_ptr(), fl.data_ptr(), None))
    torch.cuda.synchronize()
    dcnt = (ctypes.c_int64 * 4)()
    L.check(L.lib().kv_export_delta_count(var.ptr, 6, dcnt, None))
    snap.append({"meta_words": fw.cpu().numpy().tobytes(), "meta_flags": fl.cpu().numpy().tobytes(),
                 "size": ops.kv_variable_size_v2(var), "map_size": ops.kv_variable_shape_v2(var)[0],
                 "sum_freq": ops.kv_variable_frequency(var), "export": _export(ops, var),
                 "mirror_epochs": (ops.kv_get_stat(var, ops.KV_STAT_MIRROR_EPOCHS), ops.kv_get_stat(slot, ops.KV_STAT_MIRROR_EPOCHS)),
                 "delta_counts": tuple(dcnt)})
  return snap


@functools.lru_cache(maxsize=None)
def _case(world, D, rule, det):
  """One run per case, shared by the tests of cases 1 and 2: two sharded training steps, a snapshot, two rounds of the
  read-only lookup, a snapshot."""
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  table = np.random.default_rng(11).standard_normal((64, D)).astype(np.float32)
  vars_, slots, shards = _setup(ops, world, D, rule, table, thr=THR, det=det, delta=True)
  steps, reads = _train_plan(world, D)
  for batches, grads, hp in steps:
    for r in range(world):
      shards[r].lookup_route(torch.from_numpy(batches[r]).cuda())
    ops.kv_shard_exchange_local(shards, 0)
    for r in range(world):
      shards[r].lookup_serve()
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      shards[r].lookup_finish()
    for r in range(world):
      shards[r].apply_route(torch.from_numpy(grads[r]).cuda())
    ops.kv_shard_exchange_local(shards, 1)
    for r in range(world):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], hp)
  ref = _oracle_after(world, D, table)
  all_ids = np.concatenate([b for rd in reads for b in rd])
  L = _lib()
  marked = []
  for var in vars_:   # delta tracking is on and training left marks: the counts below are not trivially equal
    c = (ctypes.c_int64 * 4)()
    L.check(L.lib().kv_export_delta_count(var.ptr, 6, c, None))
    marked.append(c[2])
  # (a full export hands the delta lists on — it clears the train marks — so one is taken up front: from here on the delta
  #  counts move only if something marks a row)
  _snapshot(ops, vars_, slots, all_ids)
  before = _snapshot(ops, vars_, slots, all_ids)
  got = [_read_phases(ops, shards, rd) for rd in reads]
  torch.cuda.synchronize()
  after = _snapshot(ops, vars_, slots, all_ids)
  want_owner = [[_owner_reads(ops, vars_, b, world, rule) for b in rd] for rd in reads]
  return {"reads": reads, "got": got, "want_owner": want_owner, "ref": ref, "before": before, "after": after, "marked": marked,
          "vars": vars_, "all_ids": all_ids}


@pytest.mark.parametrize("world,D,rule,det", CASES)
def test_read_only_phases_return_the_owners_own_reads(ops, world, D, rule, det):
  c = _case(world, D, rule, det)
  st = _states(c["ref"], c["reads"][0][0])
  assert min(st.values()) >= 20, st                               # all four states are in the batch
  for rd, got, want in zip(c["reads"], c["got"], c["want_owner"]):
    for r in range(world):
      assert got[r].shape == (rd[r].size, D)
      _check_rows(got[r], want[r], c["ref"].gather_or_zeros(rd[r]), trained=True)


@pytest.mark.parametrize("world,D,rule,det", CASES)
def test_read_only_phases_change_nothing(ops, world, D, rule, det):
  c = _case(world, D, rule, det)
  assert sum(c["marked"]) > 0
  for r in range(world):
    for key in c["before"][r]:
      assert c["before"][r][key] == c["after"][r][key], (r, key)
  absent = c["all_ids"][c["all_ids"] >= ABSENT[0]]
  for r in range(world):                                          # the ids that were absent are still absent
    assert all(m is None for m in ops.kv_get_meta(c["vars"][r], np.unique(absent)))


# ---- case 3: segment geometry ------------------------------------------------------------------------------------------
def _filled(ops, world, D, rule, keys, cap, lossless=True):
  """shards over tables that hold `keys` (each on its owner; threshold 0, no training) + the oracle of the same state"""
  from oracle import kv_oracle as ko
  table = np.random.default_rng(7).standard_normal((32, D)).astype(np.float32)
  vars_, slots, shards = _setup(ops, world, D, rule, table, cap=cap, max_ids=4096)
  own = _owner(keys, world, rule)
  for o in range(world):
    if np.any(own == o):
      ops.kv_variable_gather_or_insert_v2(vars_[o], keys[own == o])
  for sh in shards:
    sh.set_lossless(lossless)
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  ref.gather_or_insert(keys)
  return vars_, slots, shards, ref


def _geometry(ops, world, D, rule, batches, keys, cap=48):
  vars_, slots, shards, ref = _filled(ops, world, D, rule, keys, cap)
  got = _read_phases(ops, shards, batches)
  assert all(sh.peer_capacity == cap for sh in shards)
  for r in range(world):
    _check_rows(got[r], _owner_reads(ops, vars_, batches[r], world, rule), ref.gather_or_zeros(batches[r]), trained=False)
  for o in range(world):
    assert ops.kv_variable_frequency(vars_[o]) == int(np.sum(_owner(keys, world, rule) == o))


def test_segment_geometry_mostly_empty_segments(ops):
  """world 8, 3 ids per rank, 49 records per segment: most segments are empty, a wave's 64 live records straddle segments"""
  rng = np.random.default_rng(2)
  keys = np.arange(0, 400, 2)                                     # odd ids are absent
  _geometry(ops, 8, 16, "hash", [rng.integers(0, 400, 3) for _ in range(8)], keys)


def test_segment_geometry_a_full_segment(ops):
  """one segment holds exactly C = 48 ids (the pattern of test_native_shard_full_capacity_cannot_overflow)"""
  keys = np.arange(0, 200, 3)
  full = np.arange(0, 96, 2)                                      # 48 distinct ids, all owned by rank 0 under "mod"
  assert full.size == 48 and np.all(_owner(full, 2, "mod") == 0)
  _geometry(ops, 2, 16, "mod", [np.concatenate([full, full[:7], [1, 3, 5]]), np.array([0, 2, 9, 11])], keys)


@pytest.mark.parametrize("live", [63, 64, 65])
def test_segment_geometry_live_totals_around_a_wave(ops, live):
  """owner 0 receives 40 + (live - 40) records in its two segments: one wave step less one lane, exactly, plus one lane"""
  keys = np.arange(0, 300, 3)
  b0 = np.concatenate([np.arange(0, 80, 2), [1, 7]])              # 40 even ids
  b1 = np.concatenate([np.arange(100, 100 + 2 * (live - 40), 2), [3]])
  assert np.sum(_owner(np.unique(b0), 2, "mod") == 0) + np.sum(_owner(np.unique(b1), 2, "mod") == 0) == live
  _geometry(ops, 2, 12, "mod", [b0, b1], keys)


# ---- case 4: lossy overflow --------------------------------------------------------------------------------------------
def test_lossy_overflow_reads_zeros_for_the_surplus_and_reports_once(ops):
  L = _lib()
  D, cap = 16, 8
  keys = np.arange(0, 100)                                        # every id of the batches is held (rows are never zero)
  vars_, slots, shards, ref = _filled(ops, 2, D, "mod", keys, cap, lossless=False)
  many = np.arange(0, 40, 2)                                      # 20 distinct ids for owner 0 against a capacity of 8
  batches = [np.concatenate([many, [1, 3, 5, 7, 9]]), np.array([50, 51, 52, 53])]
  got = _read_phases(ops, shards, batches)
  want = [_owner_reads(ops, vars_, b, 2, "mod") for b in batches]
  assert all(w.any(axis=1).all() for w in want)
  surplus = ~got[0][:20].any(axis=1)
  assert int(surplus.sum()) == 12                                 # the 12 surplus ids read exact zeros ...
  np.testing.assert_array_equal(got[0][:20][~surplus], want[0][:20][~surplus])   # ... the 8 that found room their rows
  np.testing.assert_array_equal(got[0][20:], want[0][20:])        # every other id reads its row
  np.testing.assert_array_equal(got[1], want[1])
  torch.cuda.synchronize()
  with pytest.raises(L.ResourceExhaustedError, match="peer_capacity"):
    shards[0].lookup_route(torch.from_numpy(many[:4]).cuda())
  shards[0].lookup_route(torch.from_numpy(many[:4]).cuda())       # reported once
  shards[1].lookup_route(torch.from_numpy(many[:0]).cuda())       # shard 1's own batch fitted: nothing to report


# ---- cases 5 and 6: the whole ops, ranks as threads over KvCommStaged (tests/_ranks.py) -----------------------------------
def test_whole_ops_single_and_multi_table(ops):
  """kv_shard_lookup_zeros, lossless with a capacity of 48 that must grow once, and kv_multi_shard_lookup_zeros over tables
  of dims 8, 8 and 32 (two row geometries: one grouped serve launch and one single); world 3"""
  world, rule = 3, "hash"
  rng = np.random.default_rng(41)
  keys = np.unique(rng.integers(-300, 300, 400))
  tabs = [_filled(ops, world, D, rule, keys, 48) for D in (8, 8, 32)]   # [(vars, slots, shards, ref)] per table
  ranks = _Ranks(ops, world)
  batches = [rng.integers(-320, 320, 2500 + 411 * r) for r in range(world)]
  vars0, _, shards0, ref0 = tabs[0]
  outs = ranks.run(lambda r, comm: shards0[r].lookup_zeros(comm, torch.from_numpy(batches[r]).cuda()).cpu().numpy())
  for r in range(world):
    _check_rows(outs[r], _owner_reads(ops, vars0, batches[r], world, rule), ref0.gather_or_zeros(batches[r]), trained=False)
  assert all(sh.peer_capacity > 48 for sh in shards0) and len({sh.peer_capacity for sh in shards0}) == 1   # grown once, alike
  grown = shards0[0].peer_capacity
  ids3 = [[rng.integers(-320, 320, 700 + 97 * r + 31 * t) for t in range(3)] for r in range(world)]
  ids3[1][2] = ids3[1][2][:0]                                     # an empty batch for one table on one rank
  outs = ranks.run(lambda r, comm: [o.cpu().numpy() for o in ops.kv_multi_shard_lookup_zeros(
      [tabs[t][2][r] for t in range(3)], comm, [torch.from_numpy(ids3[r][t]).cuda() for t in range(3)])])
  for r in range(world):
    for t in range(3):
      _check_rows(outs[r][t], _owner_reads(ops, tabs[t][0], ids3[r][t], world, rule), tabs[t][3].gather_or_zeros(ids3[r][t]),
                  trained=False)
  assert shards0[0].peer_capacity == grown
  for t in range(3):                                              # nothing was inserted or counted anywhere
    for o in range(world):
      assert ops.kv_variable_frequency(tabs[t][0][o]) == int(np.sum(_owner(keys, world, rule) == o))
      assert ops.kv_variable_size_v2(tabs[t][0][o]) == int(np.sum(_owner(keys, world, rule) == o))
  ranks.close()


def test_whole_op_at_world_one_equals_gather_or_zeros(ops):
  """world 1 without RCCL: the whole op equals kv_gather_or_zeros bit for bit, and the profile does not sample it"""
  rng = np.random.default_rng(5)
  keys = np.unique(rng.integers(0, 5000, 3000))
  vars_, slots, shards, ref = _filled(ops, 1, 32, "hash", keys, 0)
  comm = ops.KvComm(1, 0, None)
  shards[0].profile(1)
  ids = torch.from_numpy(rng.integers(0, 6000, 4000 + 33)).cuda()
  for join in (True, False):
    out = shards[0].lookup_zeros(comm, ids, join=join)
    if not join:
      shards[0].join()
    assert torch.equal(out, ops.kv_variable_gather_or_zeros_v2(vars_[0], ids))
  np.testing.assert_array_equal(out.cpu().numpy(), ref.gather_or_zeros(ids.cpu().numpy()))
  assert all(ms is None for ms in shards[0].profile_read()["phases_ms"].values())   # no phase was sampled
  assert ops.kv_variable_frequency(vars_[0]) == keys.size
  del comm


def test_pending_batches_and_the_refused_apply(ops):
  from oracle import kv_oracle as ko
  L = _lib()
  world, D, rule = 2, 16, "hash"
  table = np.random.default_rng(13).standard_normal((32, D)).astype(np.float32)
  vars_, slots, shards = _setup(ops, world, D, rule, table)
  ref = ko.OracleKv(D, 0, table, day=DAY, picker=1, seed=3)
  rslot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=DAY)
  ranks = _Ranks(ops, world, timeout=30)
  rng = np.random.default_rng(17)
  batches = [rng.integers(-200, 200, 1500 + 77 * r) for r in range(world)]
  grads = [(rng.uniform(0.5, 1.5, (b.size, D)) * 1e-2).astype(np.float32) for b in batches]
  ids = [torch.from_numpy(b).cuda() for b in batches]
  hp = (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
  # a training lookup of new keys leaves its partition pass pending; the read-only lookup behind it settles that pass first
  trained = ranks.run(lambda r, comm: shards[r].lookup(comm, ids[r]).cpu().numpy())
  read = ranks.run(lambda r, comm: shards[r].lookup_zeros(comm, ids[r]).cpu().numpy())
  want = ref.gather_or_insert(np.concatenate(batches))
  off = 0
  for r in range(world):
    np.testing.assert_array_equal(read[r], trained[r])
    np.testing.assert_array_equal(read[r], want[off:off + batches[r].size])
    off += batches[r].size
  # the route index of the training batch is gone: every form of its apply is refused, on every shard, with nothing queued
  torch.cuda.synchronize()
  state = [_export(ops, v) for v in vars_]
  exchanges = [c.exchanges for c in ranks.comms]
  g = [torch.from_numpy(x).cuda() for x in grads]
  for r in range(world):
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      shards[r].apply(ranks.comms[r], ops.OPT_GROUP_ADAM_V4, [slots[r]], g[r], hp)
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      shards[r].apply_route(g[r])
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      ops.kv_multi_shard_apply([shards[r]], ranks.comms[r], ops.OPT_GROUP_ADAM_V4, [[slots[r]]], [g[r]], hp)
    with pytest.raises(L.FailedPreconditionError):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], hp)          # (the serve token is void)
  torch.cuda.synchronize()
  assert [_export(ops, v) for v in vars_] == state
  assert [c.exchanges for c in ranks.comms] == exchanges
  # a fresh training lookup + apply works as ever
  before = ranks.run(lambda r, comm: shards[r].lookup(comm, ids[r]).cpu().numpy())

  def step(r, comm):
    shards[r].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[r]], g[r], hp)
  ranks.run(step)
  ref.gather_or_insert(np.concatenate(batches))
  u, s, _ = ko.dedup_segment_sum(np.concatenate(batches), np.concatenate(grads))
  ko.apply_group_adam(ref, rslot, s, u, *hp)
  allk = np.array(sorted(ref.as_dict()), np.int64)
  own = _owner(allk, world, rule)
  for r in range(world):
    keys, vals = ops.read_kv_variable_op_v2(vars_[r])
    assert set(keys.cpu().tolist()) == set(allk[own == r].tolist())
    got = dict(zip(keys.cpu().tolist(), vals.cpu().numpy()))
    for k in got:
      np.testing.assert_allclose(got[k], ref.as_dict()[k], rtol=RTOL, atol=ATOL)
  assert sum(ops.kv_variable_frequency(v) for v in vars_) == ref.sum_freq()
  # a read-only lookup behind that apply sees the rows it wrote
  after = ranks.run(lambda r, comm: shards[r].lookup_zeros(comm, ids[r]).cpu().numpy())
  for r in range(world):
    _check_rows(after[r], _owner_reads(ops, vars_, batches[r], world, rule), ref.gather_or_zeros(batches[r]), trained=True)
    assert np.all(np.any(after[r] != before[r], axis=1))            # every row moved (lr 0.1, gradients away from zero)
  ranks.close()


# ---- case 7: errors ----------------------------------------------------------------------------------------------------
def test_errors(ops):
  L = _lib()
  lib = L.lib()
  D = 8
  var = ops.kv_variable([D])                                      # never initialised
  sh = ops.KvShard(var, 1, 0, max_ids=1024)
  with pytest.raises(L.FailedPreconditionError, match="uninitialized"):
    sh.lookup_serve_zeros()
  assert lib.kv_shard_lookup_serve_zeros(None, None) == L.KV_INVALID_ARGUMENT
  comm = ops.KvComm(1, 0, None)
  buf = torch.zeros(4, D, device="cuda")
  ids = torch.arange(4, dtype=torch.int64, device="cuda")
  assert lib.kv_shard_lookup_zeros(None, comm.ptr, ids.data_ptr(), 4, buf.data_ptr(), 1, None) == L.KV_INVALID_ARGUMENT
  arr = (ctypes.c_void_p * 1)(None)
  ip, op_ = (ctypes.c_void_p * 1)(ids.data_ptr()), (ctypes.c_void_p * 1)(buf.data_ptr())
  nn = (ctypes.c_int64 * 1)(4)
  assert lib.kv_multi_shard_lookup_zeros(arr, 1, comm.ptr, ip, nn, op_, 1, None) == L.KV_INVALID_ARGUMENT
  del comm


def test_lossless_whole_op_is_refused_under_capture_before_anything_is_queued(ops):
  L = _lib()
  keys = np.arange(0, 64)
  vars_, slots, shards, ref = _filled(ops, 1, 16, "hash", keys, 0)      # lossless: the default
  comm = ops.KvComm(1, 0, None)
  ids = torch.arange(0, 64, dtype=torch.int64, device="cuda")
  want = shards[0].lookup_zeros(comm, ids).clone()                        # outside a capture it works (and verifies the communicator)
  torch.cuda.synchronize()
  s0 = torch.cuda.Stream()
  s0.wait_stream(torch.cuda.current_stream())
  g0 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g0, stream=s0):                                   # the capture survives the refusal: it ends valid
    with pytest.raises(L.FailedPreconditionError, match="kv_shard_lookup_zeros under stream capture"):
      shards[0].lookup_zeros(comm, ids)
  torch.cuda.synchronize()
  assert torch.equal(shards[0].lookup_zeros(comm, ids), want)             # and the shard works as before
  assert ops.kv_variable_frequency(vars_[0]) == 64
  del comm


def test_kv_variable_gather_or_zeros_reads_whatever_the_mode(ops):
  """KvVariable.gather_or_zeros (the owner's read of sharded.ShardedKvVariable.lookup_zeros): GatherOrZeros also while the
  module is in training mode, where sparse_read inserts"""
  from tfplus_amd.kv_variable.python.ops import kv_variable_ops
  was = kv_variable_ops.IS_TRAINING
  kv_variable_ops.set_training(True)
  try:
    w = kv_variable_ops.KvVariable(torch.ones(4, 8), name="shard_zeros/kv")
    with torch.no_grad():
      w.sparse_read(torch.tensor([1, 2, 3]))
    got = w.gather_or_zeros(torch.tensor([[1, 9], [2, 9]]))
    assert tuple(got.shape) == (2, 2, 8)
    assert torch.equal(got[:, 0].cpu(), torch.ones(2, 8)) and not got[:, 1].any()
    assert w.shape[0] == 3 and w.total_freq == 3                  # key 9 was not inserted, nothing was counted
  finally:
    kv_variable_ops.set_training(was)
