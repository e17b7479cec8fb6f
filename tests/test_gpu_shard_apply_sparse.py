"""The fused backward of the sharded sparse lookup (kvhip.h kv_shard_apply_route_sparse / kv_shard_apply_sparse /
kv_multi_shard_apply_sparse): the gradient pre-sum reads the SEGMENT gradients; the [n, dim] values are never written.

The reference of the phase form is the composition on the same routed shard: kv_variable_lookup_sparse_grad's values through
apply_route.  In deterministic mode send_rows must hold the same bits (the same additions in the same order); in the default
mode the same bits for inputs whose sums are exact in every order, and for general inputs every element within
m 2^-24 sum|term| of the float64 sum of the id's m terms (tests/_shard_apply_sparse_ref.py, which also draws the batches:
tests/test_shard_apply_sparse_ref.py holds its conditions on the CPU).  The whole ops are held against lookup + apply of the
expanded gradient on a twin rig, bit for bit.  Rigs as tests/test_gpu_shard_lookup_zeros.py builds them: `world` shards of one
table in one process, ranks as threads over KvCommStaged for the whole ops.  The pre-sum reads the route index alone, so the
phase-form cases route and sum; no exchange is needed."""
import ctypes
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
import _shard_apply_sparse_ref as A  # noqa: E402
import _sparse_grad_ref as R  # noqa: E402
import test_gpu_shard_lookup_zeros as Z  # noqa: E402  (the rigs: _setup, _filled, _Ranks, _export)

pytestmark = pytest.mark.gpu
N = A.N
SENT = -7777.25                                                   # no sum comes near it; not a NaN: a NaN would match a NaN
CASES = [(2, 4), (3, 8), (3, 12), (2, 32), (3, 64), (2, 100), (2, 256)]     # the seven classes of the entry ladder, two masked
COMB = {"sum": 0, "mean": 1, "sqrtn": 2}


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _cu(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(sh, D):
  """send_rows as [world, C + 1, D] float32 over the library's memory"""
  return sh.buffers()["send_rows"].view(torch.float32).view(sh.world, -1, D)


def _records(sh):
  """[(segment, record, id)] of the live records of send_pairs"""
  p = sh.buffers()["send_pairs"].view(torch.int64).view(sh.world, -1, 2).cpu().numpy()
  return [(o, i, int(p[o, i, 0])) for o in range(sh.world) for i in range(1, int(p[o, 0, 0]) + 1)]


def _routed(ops, world, D, det, inputs):
  """shards of a fresh table, rank r's batch routed"""
  table = np.random.default_rng(5).standard_normal((32, D)).astype(np.float32)
  vars_, slots, shards = Z._setup(ops, world, D, "hash", table, det=det, max_ids=4608)   # (small exchange buffers: they are copied out)
  for r in range(world):
    shards[r].lookup_route(_cu(inputs[r][0]))
  return vars_, shards


def _both(ops, var, sh, D, sg, seg, w, nseg, combiner):
  """(send_rows after the composition, send_rows after the fused pre-sum), each over a buffer of sentinels"""
  rows = _rows(sh, D)
  rows.fill_(SENT)
  sh.apply_route(ops.kv_variable_lookup_sparse_grad(var, sg, seg, w, nseg, combiner))
  torch.cuda.synchronize()
  want = rows.cpu().numpy().copy()
  rows.fill_(SENT)
  sh.apply_route_sparse(sg, seg, w, nseg, combiner)
  torch.cuda.synchronize()
  return want, rows.cpu().numpy().copy()


# ---- the phase form, deterministic mode: the composition's bits -----------------------------------------------------------
@pytest.mark.parametrize("world,D", CASES)
def test_phase_form_deterministic_is_the_composition_bit_for_bit(ops, world, D):
  inputs = [A.general_inputs(A.SEEDS[r], D) for r in range(world)]
  vars_, shards = _routed(ops, world, D, True, inputs)
  for r in range(world):
    ids, seg, nseg, w, sg = inputs[r]
    for combiner in R.COMBINERS:
      for weights in (None, w):
        for segdt in (np.int32, np.int64):
          want, got = _both(ops, vars_[r], shards[r], D, _cu(sg), _cu(seg.astype(segdt)), _cu(weights), nseg, combiner)
          what = (world, D, r, combiner, weights is not None, segdt.__name__)
          assert (want != SENT).any(), what
          assert R.same_bits(got, want, nan_ok=True), what
          if combiner == "mean" and weights is not None:
            assert np.isnan(want).any(), what                     # the zero-sum segment: 0 / 0 as IEEE gives it
    # segment ids outside [0, num_segments) are clamped as the expansion clamps them
    clamped = seg.copy()
    clamped[:2] = (-5, -1)
    clamped[-3:] = (nseg, nseg + 1, nseg + 70000)
    want, got = _both(ops, vars_[r], shards[r], D, _cu(sg), _cu(clamped), _cu(w), nseg, "sqrtn")
    assert R.same_bits(got, want, nan_ok=True), (world, D, r, "clamped")


# ---- the phase form, default mode (the 512-thread block shape) ---------------------------------------------------------------
@pytest.mark.parametrize("world,D", CASES)
def test_phase_form_default_mode_exact_inputs(ops, world, D):
  inputs = [A.exact_inputs(A.SEEDS[r], D) for r in range(world)]
  vars_, shards = _routed(ops, world, D, False, inputs)
  for r in range(world):
    ids, seg, nseg, w, sg = inputs[r]
    recs = _records(shards[r])
    assert sorted(k for _, _, k in recs) == sorted(set(ids.tolist()))     # every distinct id has one record
    for weights in (None, w):
      want, got = _both(ops, vars_[r], shards[r], D, _cu(sg), _cu(seg), _cu(weights), nseg, "sum")
      assert R.same_bits(got, want), (world, D, r)
      s64 = A.sums64(A.per_id_terms(ids, sg, seg, weights, nseg, "sum"))
      live = np.zeros(got.shape[:2], bool)
      for o, i, k in recs:
        live[o, i] = True
        assert np.array_equal(got[o, i].astype(np.float64), s64[k]), (world, D, r, k)
      assert (got[~live] == SENT).all()                           # nothing else was written


@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
@pytest.mark.parametrize("world,D", CASES)
def test_phase_form_default_mode_general_inputs_within_the_derived_bound(ops, world, D, combiner):
  inputs = [A.general_inputs(A.SEEDS[r], D) for r in range(world)]
  vars_, shards = _routed(ops, world, D, False, inputs)
  for r in range(world):
    ids, seg, nseg, w, sg = inputs[r]
    recs = _records(shards[r])
    rows = _rows(shards[r], D)
    for weights in (None, w):
      rows.fill_(SENT)
      shards[r].apply_route_sparse(_cu(sg), _cu(seg), _cu(weights), nseg, combiner)
      torch.cuda.synchronize()
      got = rows.cpu().numpy().astype(np.float64)
      terms = A.per_id_terms(ids, sg, seg, weights, nseg, combiner)
      s64, bound = A.sums64(terms), A.bounds(terms)
      live = np.zeros(got.shape[:2], bool)
      checked = 0
      for o, i, k in recs:
        live[o, i] = True
        x, y = got[o, i], s64[k]
        fin = np.isfinite(y)                                      # (every term finite: the float32 sum cannot overflow at 1e-2)
        err = np.abs(x[fin] - y[fin])
        assert np.all(err <= bound[k][fin]), "id %d (%d terms): error %.3g over the bound %.3g" % (
            k, len(terms[k]), float(err.max()), float(bound[k][fin][int(err.argmax())]))
        # a sum with a non-finite term (the zero-sum segment under mean): the same NaN / infinity in any order
        assert np.array_equal(np.isnan(x[~fin]), np.isnan(y[~fin])) and np.array_equal(x[~fin][~np.isnan(x[~fin])], y[~fin][~np.isnan(y[~fin])])
        checked += x.size
      assert checked == len(set(ids.tolist())) * D                # no element skipped
      assert (got[~live] == SENT).all()


# ---- the whole op -------------------------------------------------------------------------------------------------------------
def _rig(ops, world, D, table, slot_mult, det):
  vars_, slots, shards = [], [], []
  for r in range(world):
    var = ops.kv_variable([D]); slot = ops.kv_variable([slot_mult * D])
    for h, t in ((var, table), (slot, np.full((4, slot_mult * D), 0.1, np.float32))):
      ops.kv_set_clock_days(h, Z.DAY); ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t)
      if det:
        ops.kv_set_deterministic(h, True)
    vars_.append(var); slots.append(slot)
    shards.append(ops.KvShard(var, world, r, ops.KV_OWNER_HASH, max_ids=1 << 13))
  return vars_, slots, shards


def _native_apply_sparse(ops, sh, comm, opt, slot, sg, seg, w, nseg, combiner, hp):
  """kv_shard_apply_sparse through the ctypes entry itself (not through what KvShard.apply_sparse chooses to call)"""
  L = Z._lib()
  L.check(L.lib().kv_shard_apply_sparse(sh.ptr, comm.ptr, int(opt), slot.ptr, None, sg.data_ptr(), seg.data_ptr(), L.KV_DT_INT64,
                                        None if w is None else w.data_ptr(), int(nseg), COMB[combiner], ops._hp_array(hp), 1,
                                        ops._stream(sh.table)))
  torch.cuda.synchronize()                                        # (the tensors are the caller's: alive until here)


@pytest.mark.parametrize("family", ["group_adam_v4", "adagrad"])
def test_whole_op_equals_lookup_and_apply_of_the_expanded_gradient(ops, family):
  world, D = 2, 16
  opt, mult, hp = {"group_adam_v4": (ops.OPT_GROUP_ADAM_V4, 3, (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)),
                   "adagrad": (ops.OPT_ADAGRAD, 1, (0.05, 1))}[family]
  table = np.random.default_rng(29).standard_normal((32, D)).astype(np.float32)
  (va, sa, sha), (vb, sb, shb) = [_rig(ops, world, D, table, mult, True) for _ in range(2)]
  ranks = Z._Ranks(ops, world)
  for step in range(2):
    combiner = ("mean", "sqrtn")[step]
    inp = [A.general_inputs(A.SEEDS[r + step], D) for r in range(world)]
    # (weights of one sign here: a 0 / 0 scale would leave NaN rows in the tables, and every later step would compare NaNs)
    inp = [(i, sgm, ns, np.abs(w_) + np.float32(0.25), g) for i, sgm, ns, w_, g in inp]
    ids, seg, w, sg = ([_cu(x[i]) for x in inp] for i in (0, 1, 3, 4))
    nseg = [x[2] for x in inp]
    ranks.run(lambda r, comm: sha[r].lookup(comm, ids[r]))
    ranks.run(lambda r, comm: sha[r].apply(
        comm, opt, [sa[r]], ops.kv_variable_lookup_sparse_grad(va[r], sg[r], seg[r], w[r], nseg[r], combiner), hp))
    ranks.run(lambda r, comm: shb[r].lookup_sparse(comm, ids[r], seg[r], w[r], nseg[r], combiner))
    ranks.run(lambda r, comm: _native_apply_sparse(ops, shb[r], comm, opt, sb[r], sg[r], seg[r], w[r], nseg[r], combiner, hp))
  torch.cuda.synchronize()
  for r in range(world):
    assert Z._export(ops, va[r]) == Z._export(ops, vb[r])
    assert Z._export(ops, sa[r]) == Z._export(ops, sb[r])
    assert ops.kv_variable_frequency(va[r]) == ops.kv_variable_frequency(vb[r]) > 0
  ranks.close()


# ---- the multi form -----------------------------------------------------------------------------------------------------------
def test_multi_form_equals_the_single_table_calls(ops):
  """four tables in the default mode, exact inputs (so the sums are the same bits in any order): dims 12 and 12 are sparse and
  share one batched pre-sum, dim 64 is sparse and alone in its group, dim 8 passes plain values; two steps of the same shapes
  (the descriptor staging is reused) against the single-table calls on a twin rig"""
  world, dims, sparse = 2, (12, 8, 64, 12), (True, False, True, True)
  T = len(dims)
  hp = (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
  rigs = []
  for _ in range(2):
    tabs = [_rig(ops, world, D, np.random.default_rng(40 + D).standard_normal((32, D)).astype(np.float32), 3, False) for D in dims]
    rigs.append(tabs)
  ranks = Z._Ranks(ops, world)
  for step in range(2):
    inp = [[A.exact_inputs(A.SEEDS[r] + 100 * t + step, dims[t]) for t in range(T)] for r in range(world)]
    ids = [[_cu(inp[r][t][0]) for t in range(T)] for r in range(world)]
    seg = [[_cu(inp[r][t][1]) if sparse[t] else None for t in range(T)] for r in range(world)]
    nseg = [[inp[r][t][2] if sparse[t] else 0 for t in range(T)] for r in range(world)]
    w = [[_cu(inp[r][t][3]) if sparse[t] and t != 0 else None for t in range(T)] for r in range(world)]       # table 0: unweighted
    rng = np.random.default_rng(step)
    grads = [[_cu(inp[r][t][4]) if sparse[t] else _cu((rng.integers(-8, 9, (N, dims[t])) * G.GQ).astype(np.float32))
              for t in range(T)] for r in range(world)]

    def multi(r, comm):
      shs = [rigs[0][t][2][r] for t in range(T)]
      ops.kv_multi_shard_lookup_sparse(shs, comm, ids[r], seg[r], w[r], nseg[r], "sum")
      ops.kv_multi_shard_apply_sparse(shs, comm, ops.OPT_GROUP_ADAM_V4, [[rigs[0][t][1][r]] for t in range(T)], grads[r], seg[r], w[r],
                                      nseg[r], "sum", hp)

    def single(r, comm):
      for t in range(T):
        sh, slot = rigs[1][t][2][r], rigs[1][t][1][r]
        if sparse[t]:
          sh.lookup_sparse(comm, ids[r][t], seg[r][t], w[r][t], nseg[r][t], "sum")
          _native_apply_sparse(ops, sh, comm, ops.OPT_GROUP_ADAM_V4, slot, grads[r][t], seg[r][t], w[r][t], nseg[r][t], "sum", hp)
        else:
          sh.lookup(comm, ids[r][t])
          sh.apply(comm, ops.OPT_GROUP_ADAM_V4, [slot], grads[r][t], hp)
    ranks.run(multi)
    ranks.run(single)
  torch.cuda.synchronize()
  for t in range(T):
    for r in range(world):
      assert Z._export(ops, rigs[0][t][0][r]) == Z._export(ops, rigs[1][t][0][r]), (t, r)
      assert Z._export(ops, rigs[0][t][1][r]) == Z._export(ops, rigs[1][t][1][r]), (t, r)
      assert ops.kv_variable_frequency(rigs[0][t][0][r]) == ops.kv_variable_frequency(rigs[1][t][0][r]) > 0
  ranks.close()


# ---- edges (world 1: no peer can be left waiting) ---------------------------------------------------------------------------------
def test_empty_batch_argument_errors_and_refusals(ops):
  L = Z._lib()
  lib = L.lib()
  D, n, nseg = 8, 64, 16
  vars_, slots, shards, _ = Z._filled(ops, 1, D, "hash", np.arange(0, 64), 0)
  sh, comm = shards[0], ops.KvComm(1, 0, None)
  ids = torch.arange(0, n, dtype=torch.int64, device="cuda") % 40
  seg = torch.arange(0, n, dtype=torch.int64, device="cuda") // 4
  sg = torch.randn(nseg, D, device="cuda")
  hp = ops._hp_array((0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0))
  rows = _rows(sh, D)

  def phase(**edit):
    a = dict(sh=sh.ptr, sg=sg.data_ptr(), seg=seg.data_ptr(), dt=L.KV_DT_INT64, nseg=nseg, comb=1)
    a.update(edit)
    return lib.kv_shard_apply_route_sparse(a["sh"], a["sg"], a["seg"], a["dt"], None, a["nseg"], a["comb"], None)

  def whole(comb=1):
    return lib.kv_shard_apply_sparse(sh.ptr, comm.ptr, ops.OPT_GROUP_ADAM_V4, slots[0].ptr, None, sg.data_ptr(), seg.data_ptr(),
                                     L.KV_DT_INT64, None, nseg, comb, hp, 1, None)

  def multi(comb=1):
    arr, s0 = (ctypes.c_void_p * 1)(sh.ptr), (ctypes.c_void_p * 1)(slots[0].ptr)
    gp, sp, ns = (ctypes.c_void_p * 1)(sg.data_ptr()), (ctypes.c_void_p * 1)(seg.data_ptr()), (ctypes.c_int64 * 1)(nseg)
    return lib.kv_multi_shard_apply_sparse(arr, 1, comm.ptr, ops.OPT_GROUP_ADAM_V4, s0, None, gp, sp, L.KV_DT_INT64, None, ns, comb, hp,
                                           1, None)
  # an empty batch: a no-op, whatever else is passed
  sh.lookup_route(ids[:0])
  rows.fill_(SENT)
  assert phase(sg=None, seg=None, nseg=0) == L.KV_OK
  torch.cuda.synchronize()
  assert bool((rows == SENT).all())
  # the argument errors of the header, before anything is queued
  sh.lookup_route(ids)
  rows.fill_(SENT)
  assert phase(sh=None) == L.KV_INVALID_ARGUMENT
  for what, edit in [("null seg_grad", dict(sg=None)), ("null segment_ids", dict(seg=None)), ("float segment ids", dict(dt=L.KV_DT_FLOAT)),
                     ("combiner 3", dict(comb=3)), ("combiner -1", dict(comb=-1)), ("num_segments 0", dict(nseg=0)),
                     ("num_segments -1", dict(nseg=-1)), ("num_segments 2^31 - 1", dict(nseg=(1 << 31) - 1))]:
    assert phase(**edit) == L.KV_INVALID_ARGUMENT, what
  torch.cuda.synchronize()
  assert bool((rows == SENT).all())
  assert phase() == L.KV_OK                                       # the shard works as before
  torch.cuda.synchronize()
  assert not bool((rows == SENT).all())
  with pytest.raises(ValueError):
    sh.apply_route_sparse(sg, seg, None, nseg, "max")
  with pytest.raises(L.InvalidArgumentError):
    sh.apply_route_sparse(sg, seg[:-1], None, nseg, "sum")
  with pytest.raises(L.InvalidArgumentError):
    sh.apply_route_sparse(sg[:-1], seg, None, nseg, "sum")
  # the whole ops: a failed sparse pre-sum is reported at the end (the rank took part in the exchange)
  sh.lookup(comm, ids)
  assert whole(comb=3) == L.KV_INVALID_ARGUMENT
  sh.lookup(comm, ids)
  assert multi(comb=3) == L.KV_INVALID_ARGUMENT
  assert lib.kv_shard_apply_sparse(None, comm.ptr, 0, slots[0].ptr, None, sg.data_ptr(), seg.data_ptr(), L.KV_DT_INT64, None, nseg, 1, hp, 1,
                                   None) == L.KV_INVALID_ARGUMENT
  assert lib.kv_multi_shard_apply_sparse(None, 1, comm.ptr, 0, None, None, None, None, L.KV_DT_INT64, None, None, 1, hp, 1, None) \
      == L.KV_INVALID_ARGUMENT
  # after a read-only lookup the batch before it cannot be applied: refused before anything is queued
  sh.lookup(comm, ids)
  sh.lookup_zeros(comm, ids)
  torch.cuda.synchronize()
  rows.fill_(SENT)
  assert phase() == L.KV_FAILED_PRECONDITION
  assert whole() == L.KV_FAILED_PRECONDITION
  assert multi() == L.KV_FAILED_PRECONDITION
  with pytest.raises(L.FailedPreconditionError, match="read-only"):
    sh.apply_route_sparse(sg, seg, None, nseg, "mean")
  torch.cuda.synchronize()
  assert bool((rows == SENT).all())
  sh.lookup(comm, ids)                                            # a training lookup makes the shard trainable again
  assert whole() == L.KV_OK
  torch.cuda.synchronize()
  del comm


def test_a_call_that_would_grow_the_workspace_is_refused_under_capture(ops):
  """the routed shard has never run a sparse pre-sum, and then meets more segments than it has offsets for: under a stream
  capture both calls would have to grow a workspace buffer — refused before anything is queued, and the capture stays valid"""
  L = Z._lib()
  D, n = 16, 300
  vars_, slots, shards, _ = Z._filled(ops, 1, D, "hash", np.arange(0, 64), 0)
  sh = shards[0]
  ids = torch.arange(0, n, dtype=torch.int64, device="cuda") % 50
  seg = torch.arange(0, n, dtype=torch.int64, device="cuda") // 3
  sg, big = torch.randn(100, D, device="cuda"), torch.randn(5000, D, device="cuda")
  sh.lookup_route(ids)
  rows = _rows(sh, D)
  rows.fill_(SENT)
  torch.cuda.synchronize()
  s0 = torch.cuda.Stream()
  s0.wait_stream(torch.cuda.current_stream())
  g0 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g0, stream=s0):
    with pytest.raises(L.FailedPreconditionError, match="workspace has to grow"):
      sh.apply_route_sparse(sg, seg, None, 100, "mean")
  torch.cuda.synchronize()
  assert bool((rows == SENT).all())
  want, got = _both(ops, vars_[0], sh, D, sg, seg, None, 100, "mean")     # outside the capture: the buffers grow
  assert R.same_bits(got, want)
  rows.fill_(SENT)
  torch.cuda.synchronize()
  g1 = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g1, stream=s0):
    with pytest.raises(L.FailedPreconditionError, match="workspace has to grow"):
      sh.apply_route_sparse(big, seg, None, 5000, "mean")                 # more segments than the offsets hold
  torch.cuda.synchronize()
  assert bool((rows == SENT).all())


# ---- lossy overflow -----------------------------------------------------------------------------------------------------------
def test_lossy_overflow_equals_the_composition_and_reports_once(ops):
  L = Z._lib()
  D, cap = 16, 8
  vars_, slots, shards, _ = Z._filled(ops, 2, D, "mod", np.arange(0, 100), cap, lossless=False)
  for v in vars_:
    ops.kv_set_deterministic(v, True)
  many = np.arange(0, 40, 2)                                      # 20 distinct ids for owner 0 against a capacity of 8
  batches = [np.concatenate([many, many[:7], [1, 3, 5, 7, 9]]), np.array([50, 51, 52, 53, 50])]
  for sh, b in zip(shards, batches):
    sh.lookup_route(_cu(b.astype(np.int64)))
  rng = np.random.default_rng(3)
  for r, b in enumerate(batches):
    seg = np.sort(rng.integers(0, 6, b.size))
    w = rng.uniform(0.5, 1.5, b.size).astype(np.float32)
    sg = rng.standard_normal((6, D)).astype(np.float32)
    want, got = _both(ops, vars_[r], shards[r], D, _cu(sg), _cu(seg), _cu(w), 6, "mean")
    # record 0 of segment 0 is where the surplus ids' sums are dropped — several ids write it, the last one wins: not compared
    want[0, 0], got[0, 0] = 0, 0
    assert R.same_bits(got, want), r
    assert len(_records(shards[r])) == (8 + 5 if r == 0 else 4)   # owner 0's segment is full: 12 ids found no room
  torch.cuda.synchronize()
  with pytest.raises(L.ResourceExhaustedError, match="peer_capacity"):   # one call late ...
    shards[0].lookup_route(_cu(many[:4].astype(np.int64)))
  shards[0].lookup_route(_cu(many[:4].astype(np.int64)))                  # ... once
