"""kv_lookup_sparse_zeros / kv_batch_lookup_sparse_zeros (include/kvhip.h): embedding_lookup_sparse outside training in one
read-only launch.  The reference value is a float64 combine over the rows kv_variable_gather_or_zeros_v2 returns for the
same ids (tests/_sparse_zeros_ref.py); the per-element tolerance is the sequential-summation bound
(2 L + 4) 2^-24 sum_j |w_j x_j| / |den| of a segment of L positions, NaN positions must match.

The tables hold a few thousand keys inserted by training lookups (no capacity hint: they grew), some blacklisted by a
GroupAdam step with a group-lasso term, some under an enter threshold of 3; the id lists also hold keys never inserted, the
smallest and largest key of the dtype, and negative keys.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tfplus_amd import _lib  # noqa: E402
import _sparse_zeros_ref as ref  # noqa: E402

DIMS = [4, 8, 32, 64, 128, 256, 12, 260, 5, 100]
COMBINERS = ["sum", "mean", "sqrtn"]
THR = 3


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _build(ops, D, key_dtype=torch.int64, seed=0):
  """(var, slot, candidate ids): keys -1000 .. 2999 inserted; k % 4 == 1 looked up once (under the threshold), the rest three
  times; one GroupAdam step with l1 / l2 / l21 over all of them blacklists some of the rows it may update."""
  rng = np.random.default_rng(1000 + D + seed)
  npdt = np.int64 if key_dtype == torch.int64 else np.int32
  hv = ops.kv_variable([D], key_dtype=key_dtype, enter_threshold=THR)
  hs = ops.kv_variable([3 * D], key_dtype=key_dtype)
  ops.kv_set_clock_days(hv, 20000)
  ops.kv_set_seed(hv, 7)
  ops.init_kv_variable_v2(hv, rng.standard_normal((64, D)).astype(np.float32))
  ops.init_kv_variable_v2(hs, np.zeros((4, 3 * D), np.float32))
  lowest = np.iinfo(npdt).min
  keys = np.concatenate([np.arange(-1000, 3000), [lowest]]).astype(npdt)
  often = keys[keys % 4 != 1]
  ops.kv_variable_gather_or_insert_v2(hv, keys)
  for _ in range(2):
    ops.kv_variable_gather_or_insert_v2(hv, often)
  grad = (rng.normal(0, 1, (keys.size, D)) * rng.uniform(1e-4, 3e-2, (keys.size, 1))).astype(np.float32)
  ops.kv_variable_group_sparse_apply_adam_v4(hv, hs, grad, keys, 0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 1e-3, 1e-2, 2e-2)
  cand = np.concatenate([keys, np.arange(5000, 5200), [np.iinfo(npdt).max]]).astype(npdt)
  return hv, hs, cand


_TABLES = {}


def _table(ops, D, key_dtype=torch.int64):
  k = (D, key_dtype)
  if k not in _TABLES:
    _TABLES[k] = _build(ops, D, key_dtype)
  return _TABLES[k]


def _case(rng, cand, lens, trailing=5):
  """ids, ascending segment ids, weights and num_segments for segments of the given lengths"""
  lens = np.asarray(lens)
  seg = np.repeat(np.arange(lens.size), lens)
  ids = rng.choice(cand, seg.size)
  ids[: min(4, ids.size)] = [cand[-1], cand[-202], 5001, -7][: min(4, ids.size)]   # largest key (absent), smallest, absent, negative
  w = rng.uniform(0.1, 2.0, seg.size).astype(np.float32)
  return ids, seg, w, int(lens.size + trailing)


def _main_lens(rng):
  lens = rng.integers(0, 10, 200)
  lens[:3] = 0                       # empty segments lead
  lens[100] = 0                      # one in the middle
  lens[3] = 9
  return np.concatenate([lens, [300, 5000]])


def _check(ops, hv, ids, seg, w, nseg, combiner, got, what):
  rows = _np(ops.kv_variable_gather_or_zeros_v2(hv, ids))
  want, tol = ref.combine(rows, seg, w, nseg, combiner)
  ref.check(_np(got), want, tol, what)


def test_table_holds_what_the_tests_need(ops):
  hv, _, cand = _table(ops, 32)
  metas = ops.kv_get_meta(hv, cand[:4000])
  assert 0 < sum(1 for m in metas if m and m["blacklist"]) < 4000
  assert any(m and m["freq"] < THR for m in metas)
  rows = ops.kv_variable_gather_or_zeros_v2(hv, cand)
  zero = (rows == 0).all(1)
  assert bool(zero[4001:].all()) and 1000 < int((~zero).sum()) < 4001      # absent keys read zeros, and so do some present ones


@pytest.mark.parametrize("segdt", [np.int32, np.int64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("D", DIMS)
def test_parity(ops, D, combiner, weighted, segdt):
  hv, _, cand = _table(ops, D)
  rng = np.random.default_rng(D * 11 + len(combiner) + weighted)
  ids, seg, w, nseg = _case(rng, cand, _main_lens(rng))
  seg = seg.astype(segdt)
  got = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w if weighted else None, nseg, combiner)
  assert got.shape == (nseg, D)
  _check(ops, hv, ids, seg, w if weighted else None, nseg, combiner, got, "D %d %s" % (D, combiner))
  empty = np.setdiff1d(np.arange(nseg), seg)
  if weighted and combiner != "sum":
    assert bool(torch.isnan(got[empty]).all())
  else:
    assert float(got[empty].abs().sum()) == 0.0


@pytest.mark.parametrize("segdt", [np.int32, np.int64])
@pytest.mark.parametrize("D", [4, 32, 64, 256, 12, 5])
def test_parity_one_segment_and_65(ops, D, segdt):
  hv, _, cand = _table(ops, D)
  rng = np.random.default_rng(D + 5)
  for lens, trailing in (([7], 0), (rng.integers(0, 6, 65), 0)):
    ids, seg, w, nseg = _case(rng, cand, lens, trailing)
    assert nseg == len(lens)
    for combiner in COMBINERS:
      got = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg.astype(segdt), w, nseg, combiner)
      _check(ops, hv, ids, seg, w, nseg, combiner, got, "D %d nseg %d %s" % (D, nseg, combiner))


@pytest.mark.parametrize("D", [8, 64, 100])
def test_parity_int32_keys(ops, D):
  hv, _, cand = _table(ops, D, torch.int32)
  rng = np.random.default_rng(D + 9)
  ids, seg, w, nseg = _case(rng, cand, _main_lens(rng))
  for combiner in COMBINERS:
    got = ops.kv_variable_lookup_sparse_zeros(hv, ids.astype(np.int32), seg, w, nseg, combiner)
    _check(ops, hv, ids, seg, w, nseg, combiner, got, "int32 keys D %d %s" % (D, combiner))


def test_empty_inputs(ops):
  hv, _, _ = _table(ops, 8)
  none = np.zeros(0, np.int64)
  out = ops.kv_variable_lookup_sparse_zeros(hv, none, none, None, 5, "mean")
  assert out.shape == (5, 8) and float(out.abs().sum()) == 0.0
  assert ops.kv_variable_lookup_sparse_zeros(hv, none, none, None, 0, "sum").shape == (0, 8)


def _bits(t):
  return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("D", DIMS)
def test_one_id_per_segment_is_the_gather(ops, D):
  hv, _, cand = _table(ops, D)
  ids = torch.from_numpy(np.random.default_rng(D).choice(cand, 777))
  seg = torch.arange(777)
  rows = ops.kv_variable_gather_or_zeros_v2(hv, ids)
  ones = torch.ones(777)
  for combiner in ("sum", "mean"):
    got = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, None, 777, combiner)
    assert torch.equal(_bits(got), _bits(rows)), combiner
    assert torch.equal(_bits(ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, ones, 777, combiner)), _bits(got))


def test_all_ones_weights_give_the_unweighted_bits(ops):
  hv, _, cand = _table(ops, 32)
  rng = np.random.default_rng(3)
  ids, seg, _, nseg = _case(rng, cand, _main_lens(rng))
  for combiner in COMBINERS:
    a = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, None, nseg, combiner)
    b = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, np.ones(ids.size, np.float32), nseg, combiner)
    used = torch.from_numpy(np.unique(seg)).cuda()         # (an empty segment follows its own rule: zeros without weights,
    assert torch.equal(_bits(a[used]), _bits(b[used]))     #  0/0 with them)
    empty = torch.from_numpy(np.setdiff1d(np.arange(nseg), seg)).cuda()
    assert float(a[empty].abs().sum()) == 0.0
    assert bool(torch.isnan(b[empty]).all()) if combiner != "sum" else float(b[empty].abs().sum()) == 0.0


@pytest.mark.parametrize("combiner", COMBINERS)
def test_batched_equals_single_bit_for_bit(ops, combiner):
  """every dim of the parity test in ONE call; the dim-32 table listed twice with different id lists, one table without
  ids and one without segments"""
  rng = np.random.default_rng(17)
  tabs, ids, segs, ws, nsegs = [], [], [], [], []
  for k, D in enumerate(DIMS + [32, 8, 64]):
    hv, _, cand = _table(ops, D)
    i, s, w, n = _case(rng, cand, _main_lens(rng) if k % 3 == 0 else rng.integers(0, 6, 65 + k))
    if k == len(DIMS) + 1:
      i, s, w = i[:0], s[:0], w[:0]             # ns[i] == 0, segments stay
    if k == len(DIMS) + 2:
      i, s, w, n = i[:0], s[:0], w[:0], 0       # num_segments[i] == 0
    tabs.append(hv); ids.append(i); segs.append(s); ws.append(w if k % 2 else None); nsegs.append(n)
  outs = ops.batch_kv_variable_lookup_sparse_zeros(tabs, ids, segs, ws, nsegs, combiner)
  assert len(outs) == len(tabs)
  for hv, i, s, w, n, got in zip(tabs, ids, segs, ws, nsegs, outs):
    one = ops.kv_variable_lookup_sparse_zeros(hv, i, s, w, n, combiner)
    assert got.shape == one.shape == (n, hv.dim)
    assert torch.equal(_bits(got), _bits(one)), hv.dim
  ops.batch_kv_variable_lookup_sparse_zeros(tabs, ids, segs, None, nsegs, combiner)     # weights: no array at all


def _sorted_export(ops, h):
  keys, vals, black, fk, fv = [_np(x) for x in ops.kv_variable_export(h, first_n=6)]
  o, of = np.argsort(keys, kind="stable"), np.argsort(fk, kind="stable")
  return keys[o].tobytes(), vals[o].tobytes(), np.sort(black).tobytes(), fk[of].tobytes(), fv[of].tobytes()


def _state(ops, hv, probe):
  L = _lib.lib()
  figures = []
  for fn in (L.kv_size, L.kv_map_size, L.kv_sum_freq):
    v = ctypes.c_int64(-1)
    assert fn(ctypes.c_void_p(hv.ptr), ctypes.byref(v), None) == 0
    figures.append(v.value)
  return figures, ops.kv_get_meta(hv, probe), _sorted_export(ops, hv), ops.kv_get_stat(hv, ops.KV_STAT_MIRROR_APPLIES)


def test_no_side_effects(ops):
  D = 32
  A, B = _build(ops, D, seed=1), _build(ops, D, seed=1)          # twins: B never sees the op
  hv, hs, cand = A
  rng = np.random.default_rng(23)
  ids, seg, w, nseg = _case(rng, cand, _main_lens(rng))
  # a training lookup leaves its batch token on each table; the lookups under test run between it and the apply
  batch = torch.from_numpy(np.arange(-200, 1800, dtype=np.int64)).cuda()
  grad = torch.from_numpy(rng.normal(0, 1e-2, (batch.numel(), D)).astype(np.float32)).cuda()
  for t in (A, B):
    ops.kv_variable_gather_or_insert_v2(t[0], batch)
    assert t[0].batch is not None and t[0].batch[0] != 0
  tok = hv.batch[0]
  probe = np.unique(ids.astype(np.int64))
  before = _state(ops, hv, probe)
  assert any(m is None or not m for m in before[1])              # absent keys among the probed ones
  for combiner in COMBINERS:
    ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w, nseg, combiner)
    ops.batch_kv_variable_lookup_sparse_zeros([hv, hv], [ids, ids[::-1].copy()], [seg, seg], [None, w], [nseg, nseg], combiner)
  after = _state(ops, hv, probe)
  assert after == before
  assert hv.batch is not None and hv.batch[0] == tok
  for t in (A, B):                                               # the token taken before the calls is still honoured
    ops.kv_variable_group_sparse_apply_adam_v4(t[0], t[1], grad, batch, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
  assert hv.batch[0] == tok
  for a, b in zip(A[:2], B[:2]):
    assert torch.equal(_bits(ops.kv_variable_gather_or_zeros_v2(a, cand)), _bits(ops.kv_variable_gather_or_zeros_v2(b, cand)))
    assert ops.kv_get_meta(a, cand) == ops.kv_get_meta(b, cand)
  assert _state(ops, hv, probe)[3] == _state(ops, B[0], probe)[3]


def _vp(t):
  return ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("D", [64, 100])
@pytest.mark.parametrize("segdt", [torch.int32, torch.int64])
def test_segment_ids_are_clamped(ops, D, segdt):
  """out sits inside one larger allocation between guard rows; segment ids below 0 and at or above num_segments"""
  hv, _, cand = _table(ops, D)
  dev = torch.device("cuda", 0)
  rng = np.random.default_rng(D)
  nseg, guard = 40, 4
  seg_np = np.sort(rng.integers(-6, nseg + 6, 600))
  seg_np[:2], seg_np[-2:] = -(1 << 31) + 1, (1 << 31) - 1
  ids_np = rng.choice(cand, seg_np.size)
  w_np = rng.uniform(0.1, 2.0, seg_np.size).astype(np.float32)
  ids, seg, w = torch.from_numpy(ids_np).to(dev), torch.from_numpy(seg_np).to(dev).to(segdt), torch.from_numpy(w_np).to(dev)
  L = _lib.lib()
  for combiner, weights in ((0, None), (1, w), (2, w), (1, None)):
    big = torch.full((nseg + 2 * guard, D), 12345.0, device=dev)
    out = big[guard:guard + nseg]
    rc = L.kv_lookup_sparse_zeros(ctypes.c_void_p(hv.ptr), _vp(ids), _vp(seg), _lib.KV_DT_INT32 if segdt == torch.int32 else _lib.KV_DT_INT64,
                                  None if weights is None else _vp(weights), ids.numel(), nseg, combiner, _vp(out), _stream())
    assert rc == 0, L.kv_last_error()
    torch.cuda.synchronize()
    assert bool((big[:guard] == 12345.0).all()) and bool((big[guard + nseg:] == 12345.0).all())
    name = ("sum", "mean", "sqrtn")[combiner]
    rows = _np(ops.kv_variable_gather_or_zeros_v2(hv, ids))
    want, tol = ref.combine(rows, seg_np, None if weights is None else w_np, nseg, name)
    ref.check(_np(out), want, tol, "clamped %s" % name)
    assert bool((torch.isfinite(out) | torch.isnan(out)).all())
    if weights is None:
      assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("D", [32, 100])
def test_replays_in_a_graph(ops, D):
  """as test_gpu_graph_capture.py::test_gather_or_zeros_replays_in_a_graph: captured with no kv_prepare_capture"""
  hv, hs, cand = _build(ops, D, seed=2)
  dev = torch.device("cuda", 0)
  rng = np.random.default_rng(5)
  N, nseg = 3000, 500
  ids = torch.zeros(N, dtype=torch.int64, device=dev)
  seg = torch.zeros(N, dtype=torch.int64, device=dev)
  w = torch.ones(N, device=dev)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):                                            # warm-up outside the capture
    ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w, nseg, "mean")
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w, nseg, "mean")

  def fresh():
    ids.copy_(torch.from_numpy(rng.choice(cand, N)).to(dev))
    seg.copy_(torch.from_numpy(np.sort(rng.integers(0, nseg, N))).to(dev))
    w.copy_(torch.from_numpy(rng.uniform(0.1, 2.0, N).astype(np.float32)).to(dev))

  for rep in range(3):
    fresh()
    g.replay()
    torch.cuda.synchronize()
    eager = ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w, nseg, "mean")
    assert torch.equal(_bits(out), _bits(eager))
    _check(ops, hv, _np(ids), _np(seg), _np(w), nseg, "mean", out, "replay %d" % rep)
  # rows an optimizer step changed between replays are seen by the next replay (the graph holds no copy of the table)
  before = out.clone()
  keys = np.arange(-1000, 3000, dtype=np.int64)
  grad = rng.normal(0, 1e-1, (keys.size, D)).astype(np.float32)
  ops.kv_variable_group_sparse_apply_adam_v4(hv, hs, grad, keys, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
  g.replay()
  torch.cuda.synchronize()
  assert not torch.equal(_bits(out), _bits(before))
  assert torch.equal(_bits(out), _bits(ops.kv_variable_lookup_sparse_zeros(hv, ids, seg, w, nseg, "mean")))


def test_errors(ops):
  """refused before anything is queued, sizes unchanged"""
  hv, _, _ = _table(ops, 8)
  L = _lib.lib()
  dev = torch.device("cuda", 0)
  buf = torch.zeros(64, dtype=torch.int64, device=dev)
  P, H, st = _vp(buf), ctypes.c_void_p(hv.ptr), _stream()
  I32, I64 = _lib.KV_DT_INT32, _lib.KV_DT_INT64
  INVALID, PRECOND = _lib.KV_INVALID_ARGUMENT, _lib.KV_FAILED_PRECONDITION
  size = (ops.kv_variable_size_v2(hv), ops.kv_variable_frequency(hv))
  fresh = ops.kv_variable([8])                                           # never initialised
  F = ctypes.c_void_p(fresh.ptr)
  single = L.kv_lookup_sparse_zeros
  assert single(None, P, P, I64, None, 4, 2, 0, P, st) == INVALID
  assert single(F, P, P, I64, None, 4, 2, 0, P, st) == PRECOND
  assert b"uninitialized" in L.kv_last_error()
  for args in ((H, None, P, I64, None, 4, 2, 0, P, st), (H, P, None, I64, None, 4, 2, 0, P, st),
               (H, P, P, I64, None, 4, 2, 0, None, st), (H, P, P, I64, None, -1, 2, 0, P, st),
               (H, P, P, I64, None, 4, -1, 0, P, st), (H, P, P, _lib.KV_DT_FLOAT, None, 4, 2, 0, P, st),
               (H, P, P, I32, None, 4, 2, 3, P, st), (H, P, P, I32, None, 4, 2, -1, P, st)):
    assert single(*args) == INVALID, args
  assert single(H, None, None, I64, None, 0, 0, 0, None, st) == 0          # num_segments == 0: a no-op
  i64 = ctypes.c_int64

  def arr(*p):
    return (ctypes.c_void_p * len(p))(*p)

  batch = L.kv_batch_lookup_sparse_zeros
  pp, ns, nsegs = arr(P.value), (i64 * 1)(4), (i64 * 1)(2)
  hh = arr(H.value)
  assert batch(0, hh, pp, pp, I64, None, ns, nsegs, 0, pp, st) == INVALID
  assert batch(-1, hh, pp, pp, I64, None, ns, nsegs, 0, pp, st) == INVALID
  for args in ((1, None, pp, pp, I64, None, ns, nsegs, 0, pp, st), (1, hh, None, pp, I64, None, ns, nsegs, 0, pp, st),
               (1, hh, pp, None, I64, None, ns, nsegs, 0, pp, st), (1, hh, pp, pp, I64, None, None, nsegs, 0, pp, st),
               (1, hh, pp, pp, I64, None, ns, None, 0, pp, st), (1, hh, pp, pp, I64, None, ns, nsegs, 0, None, st),
               (1, arr(None), pp, pp, I64, None, ns, nsegs, 0, pp, st), (1, hh, arr(None), pp, I64, None, ns, nsegs, 0, pp, st),
               (1, hh, pp, pp, I64, None, (i64 * 1)(-4), nsegs, 0, pp, st), (1, hh, pp, pp, I64, None, ns, (i64 * 1)(-2), 0, pp, st),
               (1, hh, pp, pp, _lib.KV_DT_FLOAT, None, ns, nsegs, 0, pp, st), (1, hh, pp, pp, I64, None, ns, nsegs, 7, pp, st)):
    assert batch(*args) == INVALID, args
  assert batch(1, arr(F.value), pp, pp, I64, None, ns, nsegs, 0, pp, st) == PRECOND
  assert batch(2, arr(H.value, F.value), arr(P.value, P.value), arr(P.value, P.value), I64, None, (i64 * 2)(4, 4), (i64 * 2)(2, 2), 0,
               arr(P.value, P.value), st) == PRECOND
  if torch.cuda.device_count() > 1:                                      # tables on different devices
    other = ops.kv_variable([8], device=1)
    ops.init_kv_variable_v2(other, np.zeros((4, 8), np.float32))
    assert batch(2, arr(H.value, other.ptr), arr(P.value, P.value), arr(P.value, P.value), I64, None, (i64 * 2)(4, 4),
                 (i64 * 2)(2, 2), 0, arr(P.value, P.value), st) == INVALID
  torch.cuda.synchronize()
  assert (ops.kv_variable_size_v2(hv), ops.kv_variable_frequency(hv)) == size
  assert not bool(buf.any())
  with pytest.raises(ValueError):
    ops.kv_variable_lookup_sparse_zeros(hv, [1], [0], None, 1, "max")
  with pytest.raises(_lib.InvalidArgumentError):
    ops.kv_variable_lookup_sparse_zeros(hv, [1, 2], [0], None, 1, "sum")
  with pytest.raises(_lib.InvalidArgumentError):
    ops.batch_kv_variable_lookup_sparse_zeros([hv], [[1], [2]], [[0]], None, [1], "sum")


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def _sparse(emb_ops, seg, vals, width=16):
  ind = np.stack([seg, np.zeros_like(seg)], 1)
  return emb_ops.SparseTensor(ind, vals, [int(seg.max()) + 1, width])


def _filled_var(vs, name, D, keys, key_dtype=torch.int64):
  var = vs.get_kv_variable(name, embedding_dim=D, key_dtype=key_dtype, initializer=vs.random_normal_initializer(seed=D))
  var.sparse_read(torch.as_tensor(keys))          # training lookup: inserts
  return var


def test_embedding_lookup_sparse_in_inference_mode(ops, monkeypatch):
  from tfplus_amd.kv_variable.python.ops import embedding_ops, gen_kv_variable_ops, kv_variable_ops, variable_scope
  rng = np.random.default_rng(31)
  keys = np.arange(-300, 900, dtype=np.int64)
  calls = {"single": 0, "batch": 0, "goz": 0}

  def counted(name, key):
    real = getattr(gen_kv_variable_ops, name)

    def f(*a, **k):
      calls[key] += 1
      return real(*a, **k)
    monkeypatch.setattr(gen_kv_variable_ops, name, f)

  try:
    kv_variable_ops.set_training(True)
    variable_scope.reset_default_store()
    vars_ = [_filled_var(variable_scope, "serve_%d" % k, 16 if k % 2 else 32, keys) for k in range(6)]
    part = variable_scope.get_kv_variable("serve_part", embedding_dim=16, initializer=variable_scope.ones_initializer(),
                                          partitioner=variable_scope.fixed_size_partitioner(2))
    assert len(list(part)) == 2
    embedding_ops.embedding_lookup(part, torch.as_tensor(keys))
    kv_variable_ops.set_training(False)
    lens = rng.integers(0, 7, 120)
    lens[-1] = 3
    seg = np.repeat(np.arange(120), lens)
    feats = []
    for k in range(6):
      ids = rng.integers(-400, 1100, seg.size)      # some never inserted
      w = rng.uniform(0.1, 2.0, seg.size).astype(np.float32)
      feats.append((ids, w))
    # one variable: the reference helper's tolerance, nothing inserted, no autograd node, no pending gradient
    var = vars_[0]
    size, freq = var.total_count, var.total_freq
    ids, w = feats[0]
    rows_of = gen_kv_variable_ops.kv_variable_gather_or_zeros_v2        # (the reference's own gather is not counted)
    counted("kv_variable_lookup_sparse_zeros", "single")
    counted("batch_kv_variable_lookup_sparse_zeros", "batch")
    counted("kv_variable_gather_or_zeros_v2", "goz")
    for combiner in COMBINERS:
      for weights in (None, w):
        got = embedding_ops.embedding_lookup_sparse(var, _sparse(embedding_ops, seg, ids),
                                                    None if weights is None else _sparse(embedding_ops, seg, weights), combiner=combiner)
        assert got.grad_fn is None and not got.requires_grad
        rows = _np(rows_of(var.handle, ids))
        want, tol = ref.combine(rows, seg, weights, 120, combiner)
        ref.check(_np(got), want, tol, "embedding_lookup_sparse %s" % combiner)
    assert calls["single"] == 6 and calls["goz"] == 0 and calls["batch"] == 0
    assert (var.total_count, var.total_freq) == (size, freq) and not var._pending_grads
    # six variables of dims 16 / 32: one batched call for the device, no gather
    outs = embedding_ops.embedding_lookup_sparse_multi(vars_, [_sparse(embedding_ops, seg, i) for i, _ in feats],
                                                      [_sparse(embedding_ops, seg, x) for _, x in feats], combiner="sqrtn")
    assert calls == {"single": 6, "batch": 1, "goz": 0}
    for v, (i, x), got in zip(vars_, feats, outs):
      one = gen_kv_variable_ops.kv_variable_lookup_sparse_zeros(v.handle, i, seg, x, 120, "sqrtn")
      assert torch.equal(_bits(got), _bits(one))
    # max_norm and partitioned variables keep the chain
    calls.update(single=0, batch=0, goz=0)
    embedding_ops.embedding_lookup_sparse(var, _sparse(embedding_ops, seg, ids), None, combiner="sum", max_norm=1.0)
    assert calls["goz"] == 1 and calls["single"] == 0
    embedding_ops.embedding_lookup_sparse_multi([var], [_sparse(embedding_ops, seg, ids)], None, combiner="sum", max_norm=1.0)
    assert calls["goz"] == 2 and calls["single"] == 0 and calls["batch"] == 0
    embedding_ops.embedding_lookup_sparse(part, _sparse(embedding_ops, seg, ids), None, combiner="sum")
    assert calls["goz"] == 4 and calls["single"] == 0 and calls["batch"] == 0
  finally:
    kv_variable_ops.set_training(True)
