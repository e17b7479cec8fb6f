"""The sparse lookup on sharded tables (kvhip.h kv_shard_lookup_finish_sparse / kv_shard_lookup_sparse[_zeros] /
kv_multi_shard_lookup_sparse[_zeros]): the finish phase combines into segments.

The reference of the phase form is the PLAIN finish of the same routed batch: lookup_finish() gives the owners' rows,
tests/_sparse_zeros_ref.combine their float64 combine and the sequential-summation bound of the float32 kernel (the project's
derived bound: (2 L + 4) 2^-24 sum|w x| / |den| for a segment of L positions) — NaN positions equal, every other element
inside its own bound.  Where the combine is a copy (unweighted sum, one position per segment) and between the forms of the op
the bits are equal.  Rigs as tests/test_gpu_shard_lookup_zeros.py builds them: `world` shards of one table in one process,
kv_shard_exchange_local between the phases, ranks as threads over KvCommStaged for the whole ops."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import _row_geometry as G  # noqa: E402
import _sparse_zeros_ref as ref  # noqa: E402
import test_gpu_shard_lookup_zeros as Z  # noqa: E402  (the rigs: _setup, _train_plan, _filled, _Ranks, _snapshot, _export)

pytestmark = pytest.mark.gpu
TILE = G.TILE
N = 2 * TILE + 37
COMBINERS = ("sum", "mean", "sqrtn")
POOL = np.concatenate([Z.HOT, Z.COLD, Z.ABSENT])


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _lanes(D):
  """lanes per segment: row_lanes(dim)"""
  return G._pow2ceil(max(1, D // 4))


def _layout(D, rng, n=N):
  """(segment ids [n] ascending, num_segments, index of the zero-sum segment): lengths 0 (first, middle, last, trailing),
  1, L - 1, L, L + 1, 4 L + 3, one of 2 100 positions that crosses a tile boundary, the rest 1 .. 8; num_segments is no
  multiple of the 64 / L segments a wave takes per step."""
  L = _lanes(D)
  lens = [0, 1, L - 1, L, 0, L + 1, 4 * L + 3]
  while sum(lens) < 1000:
    lens.append(int(rng.integers(1, 9)))
  lens.append(2100)
  assert sum(lens[:-1]) < TILE < sum(lens) and sum(lens) < n
  while sum(lens) < n:
    lens.append(min(n - sum(lens), int(rng.integers(1, 9))))
  lens.append(0)
  nseg = len(lens) + 3
  if 64 // L > 1 and nseg % (64 // L) == 0:
    nseg += 1
  seg = np.repeat(np.arange(len(lens)), lens)
  assert seg.size == n
  return seg, nseg, 6


def _batch(D, rank, rng):
  """ids over held, under-threshold, blacklisted and absent keys, the segment list, weights with one zero-sum segment"""
  ids = POOL[rng.integers(0, POOL.size, N)]
  seg, nseg, zs = _layout(D, rng)
  w = rng.uniform(0.1, 2.0, N).astype(np.float32)               # (one sign, as test_gpu_lookup_sparse_zeros.py draws them: the
                                                                #  bound's denominator term assumes sums without cancellation)
  at = np.flatnonzero(seg == zs)
  w[at] = 0.0                                                   # the same id with weights 1.5 and -1.5, the rest 0:
  w[at[0]], w[at[1]] = 1.5, -1.5                                # the weights sum to 0 and so do the products -> mean is 0/0
  ids[at[1]] = ids[at[0]]
  return ids, seg, nseg, w


@functools.lru_cache(maxsize=None)
def _trained(world, D):
  """shards over tables after the two training steps of test_gpu_shard_lookup_zeros._train_plan (enter threshold 3: cold keys
  stay under it, HOT[::2] are blacklisted), one read batch per rank routed and served READ-ONLY, the plain finish's rows"""
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  table = np.random.default_rng(11).standard_normal((64, D)).astype(np.float32)
  vars_, slots, shards = Z._setup(ops, world, D, "hash", table, thr=Z.THR)
  steps, _ = Z._train_plan(world, D)
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
  rng = np.random.default_rng(1000 * world + D)
  reads = [_batch(D, r, rng) for r in range(world)]
  rows = _route_and_serve(ops, shards, [b[0] for b in reads])
  return {"vars": vars_, "slots": slots, "shards": shards, "reads": reads, "rows": rows}


def _route_and_serve(ops, shards, batches):
  """route -> exchange -> the read-only serve -> exchange -> the plain finish's rows; the route index stays"""
  for sh, b in zip(shards, batches):
    sh.lookup_route(torch.from_numpy(np.asarray(b, np.int64)).cuda())
  ops.kv_shard_exchange_local(shards, 0)
  for sh in shards:
    sh.lookup_serve_zeros()
  ops.kv_shard_exchange_local(shards, 1)
  return [sh.lookup_finish().cpu().numpy() for sh in shards]


def _bits(t):
  return t.contiguous().view(torch.int32)


# ---- the phase form against the plain finish of the same routed batch -----------------------------------------------------
PHASE_CASES = [(2, 4), (3, 8), (3, 12), (2, 100), (3, 64), (2, 256)]


@pytest.mark.parametrize("segdt", [np.int32, np.int64])
@pytest.mark.parametrize("world,D", PHASE_CASES)
def test_phase_form_matches_the_combine_of_the_plain_finish(ops, world, D, segdt):
  c = _trained(world, D)
  for r in range(world):
    ids, seg, nseg, w = c["reads"][r]
    rows = c["rows"][r]
    zero = ~rows.any(axis=1)
    assert int(zero.sum()) > 500 and int((~zero).sum()) > 500     # rows that read zeros, and rows that do not
    assert nseg % max(1, 64 // _lanes(D)) != 0 or _lanes(D) == 64
    for combiner in COMBINERS:
      for weights in (None, w):
        got = c["shards"][r].lookup_finish_sparse(seg.astype(segdt), weights, nseg, combiner)
        assert tuple(got.shape) == (nseg, D)
        want, tol = ref.combine(rows, seg, weights, nseg, combiner)
        what = "world %d dim %d rank %d %s %s" % (world, D, r, combiner, "weighted" if weights is not None else "unweighted")
        ref.check(got.cpu().numpy(), want, tol, what)
        if weights is not None and combiner == "mean":
          assert np.isnan(want[6]).all()                          # the zero-sum segment: 0/0 as IEEE gives it
    # segment ids below 0 count towards segment 0, ids >= num_segments towards none
    clamped = seg.copy()
    clamped[:2] = (-5, -1)
    clamped[-3:] = (nseg, nseg + 1, nseg + 70000)
    got = c["shards"][r].lookup_finish_sparse(clamped.astype(segdt), w, nseg, "mean")
    want, tol = ref.combine(rows, clamped, w, nseg, "mean")
    ref.check(got.cpu().numpy(), want, tol, "clamped, world %d dim %d rank %d" % (world, D, r))


# ---- exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,D", PHASE_CASES)
def test_unweighted_sum_over_single_positions_is_the_plain_finish(ops, world, D):
  c = _trained(world, D)
  for r in range(world):
    got = c["shards"][r].lookup_finish_sparse(np.arange(N), None, N, "sum")
    np.testing.assert_array_equal(got.cpu().numpy(), c["rows"][r])


@pytest.mark.parametrize("D", [12, 64])
def test_every_form_gives_the_same_bits(ops, D):
  """the phase form (every segment moved into the receive buffer), the whole op and the multi form (this rank's own segment
  read in place), and a repeated call"""
  world = 2
  c = _trained(world, D)
  shards = c["shards"]
  ranks = Z._Ranks(ops, world)
  for combiner, weighted in (("mean", True), ("sqrtn", False), ("sum", True)):
    args = [(torch.from_numpy(i).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda() if weighted else None, n)
            for i, s, n, w in c["reads"]]
    _route_and_serve(ops, shards, [b[0] for b in c["reads"]])
    phase = [shards[r].lookup_finish_sparse(args[r][1], args[r][2], args[r][3], combiner) for r in range(world)]
    again = [shards[r].lookup_finish_sparse(args[r][1], args[r][2], args[r][3], combiner) for r in range(world)]
    whole = ranks.run(lambda r, comm: shards[r].lookup_sparse_zeros(comm, args[r][0], args[r][1], args[r][2], args[r][3], combiner))
    multi = ranks.run(lambda r, comm: ops.kv_multi_shard_lookup_sparse_zeros(
        [shards[r]], comm, [args[r][0]], [args[r][1]], [args[r][2]], [args[r][3]], combiner)[0])
    for r in range(world):
      assert torch.equal(_bits(phase[r]), _bits(again[r]))
      assert torch.equal(_bits(phase[r]), _bits(whole[r]))
      assert torch.equal(_bits(phase[r]), _bits(multi[r]))
  del ranks


# ---- edge cases --------------------------------------------------------------------------------------------------------------
def test_an_empty_batch_still_writes_its_segments_and_no_segments_is_a_no_op(ops):
  L = Z._lib()
  world, D = 2, 16
  keys = np.arange(0, 200)
  vars_, slots, shards, _ = Z._filled(ops, world, D, "hash", keys, 0)
  ids1 = np.arange(0, 77)
  rows = _route_and_serve(ops, shards, [ids1[:0], ids1])        # rank 0's batch is empty
  out = torch.full((5, D), 7.0, device="cuda")
  L.check(L.lib().kv_shard_lookup_finish_sparse(shards[0].ptr, None, L.KV_DT_INT64, None, 5, 1, out.data_ptr(), None))
  torch.cuda.synchronize()
  assert not out.any()                                            # n == 0: every segment by the empty-segment rule
  seg1 = np.sort(np.random.default_rng(3).integers(0, 9, 77))
  got = shards[1].lookup_finish_sparse(seg1, None, 9, "mean")
  want, tol = ref.combine(rows[1], seg1, None, 9, "mean")
  ref.check(got.cpu().numpy(), want, tol, "the rank with ids")
  assert tuple(shards[1].lookup_finish_sparse(seg1, None, 0, "mean").shape) == (0, D)      # num_segments == 0: a no-op
  assert tuple(shards[0].lookup_finish_sparse(seg1[:0], None, 0, "sum").shape) == (0, D)
  # the whole op: the same on one rank of two
  ranks = Z._Ranks(ops, world)
  whole = ranks.run(lambda r, comm: shards[r].lookup_sparse_zeros(
      comm, torch.from_numpy(ids1[:0] if r == 0 else ids1).cuda(), seg1[:0] if r == 0 else seg1, None, 9, "mean"))
  assert tuple(whole[0].shape) == (9, D) and not whole[0].any()
  assert torch.equal(_bits(whole[1]), _bits(got))
  assert all(ops.kv_variable_frequency(v) == int(np.sum(Z._owner(keys, world, "hash") == o)) for o, v in enumerate(vars_))
  del ranks


# ---- the training form -------------------------------------------------------------------------------------------------------
def test_training_form_equals_lookup_and_apply_of_the_expanded_gradient(ops):
  """two identical rigs in deterministic mode: lookup + apply(kv_variable_lookup_sparse_grad's values) against
  lookup_sparse + apply_sparse — exports, slot tables and frequencies bit for bit after two steps"""
  world, D, nseg = 2, 16, 301
  table = np.random.default_rng(29).standard_normal((32, D)).astype(np.float32)
  rigs = [Z._setup(ops, world, D, "hash", table, det=True) for _ in range(2)]
  ranks = Z._Ranks(ops, world)
  rng = np.random.default_rng(31)
  hp = (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
  for step in range(2):
    ids = [torch.from_numpy(rng.integers(-150, 250, 1800 + 133 * r)).cuda() for r in range(world)]
    segs = [torch.from_numpy(np.sort(rng.integers(0, nseg, i.numel()))).cuda() for i in ids]
    wts = [torch.from_numpy(rng.uniform(0.5, 1.5, i.numel()).astype(np.float32)).cuda() for i in ids]
    sgrad = [torch.from_numpy((rng.uniform(0.5, 1.5, (nseg, D)) * 1e-2).astype(np.float32)).cuda() for _ in ids]
    combiner = ("mean", "sqrtn")[step]
    (va, sa, sha), (vb, sb, shb) = rigs
    rows = ranks.run(lambda r, comm: sha[r].lookup(comm, ids[r]))

    def apply_a(r, comm):
      values = ops.kv_variable_lookup_sparse_grad(va[r], sgrad[r], segs[r], wts[r], nseg, combiner)
      sha[r].apply(comm, ops.OPT_GROUP_ADAM_V4, [sa[r]], values, hp)
    ranks.run(apply_a)
    outs = ranks.run(lambda r, comm: shb[r].lookup_sparse(comm, ids[r], segs[r], wts[r], nseg, combiner))
    ranks.run(lambda r, comm: shb[r].apply_sparse(comm, ops.OPT_GROUP_ADAM_V4, [sb[r]], sgrad[r], segs[r], wts[r], nseg, combiner, hp))
    for r in range(world):                                        # the forward: the combine of the rows rig A's lookup returned
      want, tol = ref.combine(rows[r].cpu().numpy(), segs[r].cpu().numpy(), wts[r].cpu().numpy(), nseg, combiner)
      ref.check(outs[r].cpu().numpy(), want, tol, "training form, step %d rank %d" % (step, r))
  torch.cuda.synchronize()
  (va, sa, _), (vb, sb, _) = rigs
  for r in range(world):
    assert Z._export(ops, va[r]) == Z._export(ops, vb[r])
    assert Z._export(ops, sa[r]) == Z._export(ops, sb[r])
    assert ops.kv_variable_frequency(va[r]) == ops.kv_variable_frequency(vb[r]) > 0
  assert sum(ops.kv_variable_frequency(v) for v in vb) == 2 * sum(1800 + 133 * r for r in range(world))   # every occurrence counted
  del ranks


# ---- the read-only form ------------------------------------------------------------------------------------------------------
def test_read_only_form_changes_nothing_and_voids_a_pending_batch(ops):
  L = Z._lib()
  world, D = 2, 16
  table = np.random.default_rng(13).standard_normal((32, D)).astype(np.float32)
  vars_, slots, shards = Z._setup(ops, world, D, "hash", table, delta=True)
  ranks = Z._Ranks(ops, world, timeout=30)
  rng = np.random.default_rng(17)
  batches = [rng.integers(-200, 200, 1500 + 77 * r) for r in range(world)]
  ids = [torch.from_numpy(b).cuda() for b in batches]
  segs = [np.sort(rng.integers(0, 100, b.size)) for b in batches]
  trained = ranks.run(lambda r, comm: shards[r].lookup(comm, ids[r]).cpu().numpy())     # a pending training batch
  probe = np.concatenate(batches + [np.arange(5000, 5050)])
  Z._snapshot(ops, vars_, slots, probe)                           # (a full export hands the delta lists on: taken up front)
  before = Z._snapshot(ops, vars_, slots, probe)
  read = ranks.run(lambda r, comm: shards[r].lookup_sparse_zeros(comm, ids[r], segs[r], None, 100, "mean"))
  torch.cuda.synchronize()
  assert Z._snapshot(ops, vars_, slots, probe) == before          # tables, kv_get_meta records, counters
  for r in range(world):
    want, tol = ref.combine(trained[r], segs[r], None, 100, "mean")
    ref.check(read[r].cpu().numpy(), want, tol, "read-only whole op, rank %d" % r)
  g = [torch.zeros(b.size, D, device="cuda") for b in batches]
  hp = (0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
  for r in range(world):                                          # the training batch can no longer be applied
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      shards[r].apply(ranks.comms[r], ops.OPT_GROUP_ADAM_V4, [slots[r]], g[r], hp)
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      shards[r].apply_sparse(ranks.comms[r], ops.OPT_GROUP_ADAM_V4, [slots[r]], torch.zeros(100, D, device="cuda"), segs[r], None,
                             100, "mean", hp)
  # the training form leaves the shard trainable again
  ranks.run(lambda r, comm: shards[r].lookup_sparse(comm, ids[r], segs[r], None, 100, "mean"))
  ranks.run(lambda r, comm: shards[r].apply(comm, ops.OPT_GROUP_ADAM_V4, [slots[r]], g[r], hp))
  del ranks


# ---- the multi form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_only", [True, False])
def test_multi_form_equals_the_single_table_calls(ops, read_only):
  """three tables: dims 12 and 16 share row_lanes (4; dim 12 with a masked lane) and are combined in one launch, dim 8 has
  segment_ids None and is finished plainly"""
  world, rule = 2, "hash"
  rng = np.random.default_rng(43)
  keys = np.unique(rng.integers(-300, 300, 400))
  tabs = [Z._filled(ops, world, D, rule, keys, 0) for D in (12, 8, 16)]
  ranks = Z._Ranks(ops, world)
  ids = [[torch.from_numpy(rng.integers(-320, 320, 900 + 97 * r + 31 * t)).cuda() for t in range(3)] for r in range(world)]
  nsegs = [150, 0, 77]
  segs = [[None if t == 1 else np.sort(rng.integers(0, nsegs[t], ids[r][t].numel())) for t in range(3)] for r in range(world)]
  wts = [[None, None, rng.uniform(-1, 2, ids[r][2].numel()).astype(np.float32)] for r in range(world)]
  multi = ops.kv_multi_shard_lookup_sparse_zeros if read_only else ops.kv_multi_shard_lookup_sparse
  outs = ranks.run(lambda r, comm: multi([tabs[t][2][r] for t in range(3)], comm, ids[r], segs[r], wts[r], nsegs, "sqrtn"))

  def single(r, comm):
    sh = [tabs[t][2][r] for t in range(3)]
    if read_only:
      return [sh[0].lookup_sparse_zeros(comm, ids[r][0], segs[r][0], None, nsegs[0], "sqrtn"), sh[1].lookup_zeros(comm, ids[r][1]),
              sh[2].lookup_sparse_zeros(comm, ids[r][2], segs[r][2], wts[r][2], nsegs[2], "sqrtn")]
    return [sh[0].lookup_sparse(comm, ids[r][0], segs[r][0], None, nsegs[0], "sqrtn"), sh[1].lookup(comm, ids[r][1]),
            sh[2].lookup_sparse(comm, ids[r][2], segs[r][2], wts[r][2], nsegs[2], "sqrtn")]
  ones = ranks.run(single)          # (the training form: the keys the first call inserted are held at the second, same rows)
  for r in range(world):
    assert [tuple(o.shape) for o in outs[r]] == [(150, 12), (ids[r][1].numel(), 8), (77, 16)]
    for t in range(3):
      assert torch.equal(_bits(outs[r][t]), _bits(ones[r][t])), (r, t)
    assert bool(outs[r][0].any()) and bool(outs[r][1].any())
  del ranks


# ---- lossy overflow ----------------------------------------------------------------------------------------------------------
def test_lossy_overflow_surplus_ids_are_zero_rows_that_count_in_the_mean(ops):
  L = Z._lib()
  D, cap = 16, 8
  keys = np.arange(0, 100)                                        # every id of the batches is held (rows are never zero)
  vars_, slots, shards, _ = Z._filled(ops, 2, D, "mod", keys, cap, lossless=False)
  many = np.arange(0, 40, 2)                                      # 20 distinct ids for owner 0 against a capacity of 8
  batches = [np.concatenate([many, [1, 3, 5, 7, 9]]), np.array([50, 51, 52, 53])]
  rows = _route_and_serve(ops, shards, batches)
  surplus = ~rows[0][:20].any(axis=1)
  assert int(surplus.sum()) == 12
  seg = np.concatenate([np.zeros(20, np.int64), [1, 1, 2, 2, 2]])
  got = shards[0].lookup_finish_sparse(seg, None, 3, "mean").cpu().numpy()
  want, tol = ref.combine(rows[0], seg, None, 3, "mean")
  ref.check(got, want, tol, "lossy overflow")
  held = Z._owner_reads(ops, vars_, many, 2, "mod")[~surplus]     # the 8 ids that found room: their rows, over a denominator of 20
  np.testing.assert_allclose(got[0], held.astype(np.float64).sum(0) / 20.0, rtol=1e-5, atol=1e-7)
  torch.cuda.synchronize()
  with pytest.raises(L.ResourceExhaustedError, match="peer_capacity"):   # one call late ...
    shards[0].lookup_route(torch.from_numpy(many[:4]).cuda())
  shards[0].lookup_route(torch.from_numpy(many[:4]).cuda())               # ... once


# ---- errors (world 1: no peer can be left waiting) ------------------------------------------------------------------------------
def _raw_args(bad):
  """the argument errors of the header, as (segment pointer, dtype, num_segments, combiner, out pointer) edits"""
  return [("null segment_ids", dict(seg=None)), ("null out", dict(out=None)), ("float segment ids", dict(dt=bad.KV_DT_FLOAT)),
          ("combiner 3", dict(comb=3)), ("combiner -1", dict(comb=-1)), ("num_segments -1", dict(nseg=-1)),
          ("num_segments 2^31 - 1", dict(nseg=(1 << 31) - 1))]


def test_argument_errors(ops):
  L = Z._lib()
  lib = L.lib()
  D, n = 8, 64
  keys = np.arange(0, 64)
  vars_, slots, shards, _ = Z._filled(ops, 1, D, "hash", keys, 0)
  sh = shards[0]
  comm = ops.KvComm(1, 0, None)
  ids = torch.arange(0, n, dtype=torch.int64, device="cuda")
  seg = torch.arange(0, n, dtype=torch.int64, device="cuda") // 4
  nseg = 16
  fresh = ops.KvShard(vars_[0], 1, 0, max_ids=1024)             # never routed
  out = torch.full((nseg, D), 7.0, device="cuda")
  assert lib.kv_shard_lookup_finish_sparse(fresh.ptr, seg.data_ptr(), L.KV_DT_INT64, None, nseg, 1, out.data_ptr(), None) \
      == L.KV_FAILED_PRECONDITION
  assert lib.kv_shard_lookup_finish_sparse(None, seg.data_ptr(), L.KV_DT_INT64, None, nseg, 1, out.data_ptr(), None) == L.KV_INVALID_ARGUMENT
  want = sh.lookup_sparse_zeros(comm, ids, seg, None, nseg, "mean").clone()
  sh.lookup_route(ids)
  sh.lookup_serve_zeros()
  ops.kv_shard_exchange_local([sh], 1)
  for what, edit in _raw_args(L):
    a = dict(seg=seg.data_ptr(), dt=L.KV_DT_INT64, nseg=nseg, comb=1, out=out.data_ptr())
    a.update(edit)
    assert lib.kv_shard_lookup_finish_sparse(sh.ptr, a["seg"], a["dt"], None, a["nseg"], a["comb"], a["out"], None) == L.KV_INVALID_ARGUMENT, what
    assert lib.kv_shard_lookup_sparse_zeros(sh.ptr, comm.ptr, ids.data_ptr(), a["seg"], a["dt"], None, n, a["nseg"], a["comb"], a["out"], 1,
                                            None) == L.KV_INVALID_ARGUMENT, what
    assert lib.kv_shard_lookup_sparse(sh.ptr, comm.ptr, ids.data_ptr(), a["seg"], a["dt"], None, n, a["nseg"], a["comb"], a["out"], 1,
                                      None) == L.KV_INVALID_ARGUMENT, what
    arr, ip = (ctypes.c_void_p * 1)(sh.ptr), (ctypes.c_void_p * 1)(ids.data_ptr())
    sp, op_ = (ctypes.c_void_p * 1)(a["seg"]), (ctypes.c_void_p * 1)(a["out"])
    nn, ns = (ctypes.c_int64 * 1)(n), (ctypes.c_int64 * 1)(a["nseg"])
    if a["seg"] is not None:                                      # (a null entry of the multi form asks for the plain finish)
      assert lib.kv_multi_shard_lookup_sparse_zeros(arr, 1, comm.ptr, ip, sp, a["dt"], None, nn, ns, a["comb"], op_, 1, None) \
          == L.KV_INVALID_ARGUMENT, what
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())                                 # out was never written
  assert lib.kv_shard_lookup_sparse_zeros(None, comm.ptr, ids.data_ptr(), seg.data_ptr(), L.KV_DT_INT64, None, n, nseg, 1, out.data_ptr(), 1,
                                          None) == L.KV_INVALID_ARGUMENT
  assert lib.kv_multi_shard_lookup_sparse(None, 1, comm.ptr, None, None, L.KV_DT_INT64, None, None, None, 1, None, 1, None) == L.KV_INVALID_ARGUMENT
  with pytest.raises(ValueError):
    sh.lookup_sparse_zeros(comm, ids, seg, None, nseg, "max")
  with pytest.raises(L.InvalidArgumentError):
    sh.lookup_sparse_zeros(comm, ids, seg[:-1], None, nseg, "sum")
  assert torch.equal(_bits(sh.lookup_sparse_zeros(comm, ids, seg, None, nseg, "mean")), _bits(want))     # the shard works as before
  assert ops.kv_variable_frequency(vars_[0]) == 64                # (the refused training forms inserted and counted nothing)
  del comm


def test_lossless_whole_op_is_refused_under_capture_before_anything_is_queued(ops):
  L = Z._lib()
  keys = np.arange(0, 64)
  vars_, slots, shards, _ = Z._filled(ops, 1, 16, "hash", keys, 0)        # lossless: the default
  comm = ops.KvComm(1, 0, None)
  ids = torch.arange(0, 64, dtype=torch.int64, device="cuda")
  seg = torch.arange(0, 64, dtype=torch.int64, device="cuda") // 3
  want = shards[0].lookup_sparse_zeros(comm, ids, seg, None, 22, "mean").clone()
  torch.cuda.synchronize()
  s0 = torch.cuda.Stream()
  s0.wait_stream(torch.cuda.current_stream())
  g0 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g0, stream=s0):                                   # the capture survives the refusal: it ends valid
    with pytest.raises(L.FailedPreconditionError, match="kv_shard_lookup_sparse_zeros under stream capture"):
      shards[0].lookup_sparse_zeros(comm, ids, seg, None, 22, "mean")
    with pytest.raises(L.FailedPreconditionError, match="kv_shard_lookup_sparse under stream capture"):
      shards[0].lookup_sparse(comm, ids, seg, None, 22, "mean")
  torch.cuda.synchronize()
  assert torch.equal(_bits(shards[0].lookup_sparse_zeros(comm, ids, seg, None, 22, "mean")), _bits(want))
  assert ops.kv_variable_frequency(vars_[0]) == 64
  del comm
