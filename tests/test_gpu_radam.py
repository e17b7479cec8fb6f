"""The fused plain-RectifiedAdam op (kvhip.h kv_apply_rectified_adam and its forms) against radam_ref (tests/_radam_ref.py), one restatement
of the step's arithmetic, run on the table model of tests/_kv_model.py through the chain the reference composes
(rectified_adam.py:68-96): gather_or_insert(opt) -> scatter_update(opt) [-> gather_or_insert(var)] -> scatter_sub(var)."""
import itertools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kv_model as M  # noqa: E402
import _ranks  # noqa: E402
from _radam_ref import HP, chain, radam_ref  # noqa: E402  (the scalars' order: _radam_ref.HP)

F = np.float32
DAY, SEED = 20000, 5
FLAGS = list(itertools.product((0.0, 0.01), (0, 1), (0, 1), (0, 1)))        # weight_decay x tractable x amsgrad x use_nesterov
DIMS_NS = [(D, n) for D in (4, 32, 256, 5, 260) for n in (1, 63, 2049)]     # entry-list classes, 5: the fallback; 2049: two tiles
# The largest elementwise distance of radam_ref in float32 from radam_ref in float64 over every step of every case of
# test_unique_ids, var and slot rows (on the CPU: max of |w32 - w64| over _unique_steps(D, n) for D, n in DIMS_NS):
# 3.0833053e-08.  The GPU's sqrt and division are correctly rounded outside fast math and should add nothing: twice that.
F64_BOUND = 2 * 3.0833053e-08


def _unique_steps(D, n):
  """-> the var's init table, [(ids, grad, hp, float32 [var, slot] rows, float64 ..., [var, slot] metas)]: half the keys new"""
  rng = np.random.default_rng(1000 * D + n)
  init = rng.uniform(-0.5, 0.5, (64, D)).astype(F)
  var, slot = _models(D, init)
  out, seen = [], np.zeros(0, np.int64)
  for t, (wd, tract, ams, nest) in enumerate(FLAGS):
    old = rng.choice(seen, min(n // 2, seen.size), replace=False)
    ids = np.concatenate([old, 10 ** 6 * (t + 1) + rng.choice(10 * n, n - old.size, replace=False) - n]).astype(np.int64)
    g = (rng.normal(0, 1, (n, D)) * rng.choice([1e-1, 1e-3], (n, 1))).astype(F)
    hp = (0.05, F(0.9) ** (t + 1), F(0.999) ** (t + 1), 0.9, 0.999, 1e-7, wd, 0.4, tract, ams, nest)
    w64 = chain(var, slot, ids, g, hp)[2:]
    out.append((ids, g, hp, [var.read(ids), slot.read(ids)], w64, [var.metas(ids), slot.metas(ids)]))
    seen = np.union1d(seen, ids)
  return init, out


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _models(D, init, thr=0):
  return M.Table(D, init, SEED, DAY, thr), M.Table(3 * D, np.full((16, 3 * D), 1e-4, F), SEED, DAY)


def _pair(ops, D, init, thr=0, cap=0):
  hs = [ops.kv_variable([D], enter_threshold=thr, capacity_hint=cap), ops.kv_variable([3 * D], capacity_hint=cap)]
  for h, t in zip(hs, (init, np.full((16, 3 * D), 1e-4, F))):
    ops.kv_set_clock_days(h, DAY)
    ops.kv_set_seed(h, SEED)
    ops.init_kv_variable_v2(h, np.asarray(t, F))
  return hs


def _apply(ops, hs, g, ids, hp=HP, **kw):
  ops.kv_variable_sparse_apply_rectified_adam(hs[0], hs[1], g, ids, *hp, **kw)


def _rows(ops, h, keys):
  return ops.kv_variable_gather_or_zeros_v2(h, np.asarray(keys, np.int64)).cpu().numpy()


def _same(ops, hs, want, keys):
  for h, w in zip(hs, want):
    model = isinstance(w, M.Table)
    assert np.array_equal(_rows(ops, h, keys).view(np.uint32), (w.read(keys) if model else _rows(ops, w, keys)).view(np.uint32))
    assert ops.kv_get_meta(h, keys) == (w.metas(keys) if model else ops.kv_get_meta(w, keys))
    assert int(ops.kv_variable_shape_v2(h)[0]) == (len(w.rows) if model else int(ops.kv_variable_shape_v2(w)[0]))


@pytest.mark.parametrize("D,n", DIMS_NS)
def test_unique_ids(ops, D, n):
  """rows bit for bit the float32 restatement's (amsgrad = 0: an existing row's vhat block as it was), F64_BOUND, the records"""
  init, steps = _unique_steps(D, n)
  hs = _pair(ops, D, init)
  for ids, g, hp, w32, w64, metas in steps:
    _apply(ops, hs, g, ids, hp)
    for h, a, b, mt in zip(hs, w32, w64, metas):
      got = _rows(ops, h, ids)
      print(D, n, hp[6:], "max |gpu - f64| %.3g" % np.abs(got - b).max())
      assert np.array_equal(got.view(np.uint32), a.view(np.uint32)), (hp, np.argwhere(got != a)[:5])
      assert (np.abs(got - b) <= F64_BOUND).all() and ops.kv_get_meta(h, ids) == mt


@pytest.mark.parametrize("order", ["occurrence", "default"])
def test_repeated_ids(ops, order):
  """Keys with 2, 17 and 300 occurrences among single ones, two tiles.  Occurrence order: the chain fed the in-order float32
  sums, bit for bit.  Default order: the sum the kernel formed lies within dg = (cnt - 1) 2^-24 sum|g| of the exact one
  (tests/_reorder.py's interval), so a var element may differ from the float64 step at the exact sum by the step's change
  over [gsum - dg, gsum + dg] (both ends, doubled as _reorder does) plus the float32 evaluation's own error, taken from the
  restatement: twice |float32 - float64| at the in-order sum, plus an ulp of the row."""
  rng = np.random.default_rng(33)
  D = 32
  init = rng.uniform(-0.5, 0.5, (64, D)).astype(F)
  hs, models = _pair(ops, D, init), _models(D, init)
  if order == "occurrence":
    ops.kv_set_deterministic(hs[0], ops.KV_ORDER_OCCURRENCE)
  ids = np.concatenate([np.repeat([7, 8, 9], [2, 17, 300]), np.arange(100, 2100)]).astype(np.int64)
  rng.shuffle(ids)
  for t in range(2):
    g = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    u, s = M.dedup_sum(ids, g)
    x0, s0, x64, _ = chain(models[0], models[1], u, s, HP)
    _apply(ops, hs, g, ids)
    if order == "occurrence":
      _same(ops, hs, models, u)
      continue
    inv = np.searchsorted(np.sort(u), ids)
    inv = np.argsort(u)[inv]                                      # every id's place in u
    gsum, gabs = np.zeros((u.size, D)), np.zeros((u.size, D))
    np.add.at(gsum, inv, g.astype(np.float64))
    np.add.at(gabs, inv, np.abs(g.astype(np.float64)))
    dg = (np.bincount(inv)[:, None] - 1) * 2.0 ** -24 * gabs
    f = lambda gs: x0 - radam_ref(x0, s0, gs, HP, np.float64)[0]
    mid = f(gsum)
    bound = 2 * np.maximum(np.abs(f(gsum - dg) - mid), np.abs(f(gsum + dg) - mid)) + 2 * np.abs(models[0].read(u) - x64) + \
        2.0 ** -23 * np.abs(mid)
    got = _rows(ops, hs[0], u)
    assert (np.abs(got - mid) <= bound).all(), np.abs(got - mid).max()
    for h, m in zip(hs, models):                                  # the next step starts from the device's own rows
      m.scatter_update(u, _rows(ops, h, u), 0)


@pytest.mark.parametrize("D", [8, 32])
def test_forms_agree(ops, D):
  """plain, _tok, _unique, counted, batched: the same bits; kv_apply_sparse = kv_lookup_sparse_grad + plain (deterministic mode)"""
  rng = np.random.default_rng(50 + D)
  init = rng.uniform(-0.5, 0.5, (64, D)).astype(F)
  twins = [_pair(ops, D, init) for _ in range(9)]
  for tw in twins[7:]:
    ops.kv_set_deterministic(tw[0], 1)
  for t in range(2):
    ids = torch.from_numpy(rng.choice(4000, 1500, replace=False).astype(np.int64)).cuda()
    g = torch.from_numpy(rng.normal(0, 0.05, (1500, D)).astype(F)).cuda()
    for tw in twins:
      ops.kv_variable_gather_or_insert_v2(tw[0], ids if tw is twins[1] else ids.clone())
    assert ops._token_for(twins[1][0], ids) != 0
    _apply(ops, twins[0], g, ids.clone())
    _apply(ops, twins[1], g, ids)
    _apply(ops, twins[2], g, ids.clone(), unique_indices=True)
    _apply(ops, twins[3], g, ids.clone(), unique_count=torch.tensor([1500], dtype=torch.int64, device="cuda"))
    ops.kv_multi_sparse_apply_rectified_adam([tw[0] for tw in twins[4:7]], [tw[1] for tw in twins[4:7]], [g] * 3,
                                             [ids.clone() for _ in range(3)], *HP)
    for tw in twins[1:7]:
      _same(ops, tw, twins[0], ids.cpu().numpy())
    rep = torch.cat([ids, ids[:700]])                             # repeated ids, segments of 1 .. 3 positions, weighted mean
    seg, w = torch.arange(rep.numel(), device="cuda") // 3, torch.rand(rep.numel(), device="cuda") + 0.5
    nseg = int(seg[-1]) + 1
    sg = torch.randn(nseg, D, device="cuda") * 3e-2
    ops.kv_variable_apply_sparse("rectified_adam", twins[7], HP, sg, rep, seg, w, nseg, "mean")
    _apply(ops, twins[8], ops.kv_variable_lookup_sparse_grad(twins[8][0], sg, seg, w, nseg, "mean"), rep.clone())
    _same(ops, twins[7], twins[8], ids.cpu().numpy())


def test_sharded_apply_takes_code_8(ops):
  """world 2 through tests/_ranks.py against one table, at tests/test_gpu_adam.py's tolerance for the same check"""
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76)
  D, world = 16, 2
  init = rng.uniform(-0.5, 0.5, (64, D)).astype(F)
  ref, parts = _pair(ops, D, init), [_pair(ops, D, init) for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
  grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]

  def step(r, comm):
    shs[r].lookup(comm, torch.from_numpy(ids[r]).cuda())
    torch.cuda.synchronize()
    shs[r].apply(comm, ops.OPT_RADAM, [parts[r][1]], torch.from_numpy(grads[r]).cuda(), [float(v) for v in HP])
  ranks = _ranks.Ranks(ops, world)
  ranks.run(step)
  ranks.close()
  ops.kv_variable_gather_or_insert_v2(ref[0], np.concatenate(ids))
  _apply(ops, ref, np.concatenate(grads), np.concatenate(ids))
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r, j in itertools.product(range(world), range(2)):
    np.testing.assert_allclose(_rows(ops, parts[r][j], u[own == r]), _rows(ops, ref[j], u[own == r]), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("cap", [0, 4096])                        # the general path; a pre-sized pair: later steps on the slot mirrors
def test_bookkeeping(ops, wd, cap):
  """keys under the enter threshold are updated; blacklisted rows stay unwritten; the var's hits come with weight decay only"""
  rng = np.random.default_rng(80)
  D, hp = 8, HP[:6] + (wd,) + HP[7:]
  init = rng.uniform(-0.5, 0.5, (64, D)).astype(F)
  hs, models = _pair(ops, D, init, thr=3, cap=cap), _models(D, init, thr=3)
  ids = rng.choice(2000, 300, replace=False).astype(np.int64)
  ops.kv_variable_gather_or_insert_v2(hs[0], ids)
  models[0].gather_or_insert(ids)                                 # frequency 1: below the threshold
  before = _rows(ops, hs[0], ids)
  for t in range(4):
    if t == 1:                                                    # var keys 0 .. 4, slot keys 3 .. 8 go on the blacklists
      for h, m, black in zip(hs, models, (ids[:5], ids[3:9])):
        fw = np.array([m.rows[int(k)].freq for k in ids], np.uint32)
        ops.kv_variable_import(h, ids, m.read(ids), blacklist=[int(k) for k in black], freq_keys=ids, freq_values=fw)
        for k in black:
          m.blacklist(k)
    g = rng.normal(0, 0.1, (ids.size, D)).astype(F)
    chain(models[0], models[1], ids, g, hp)
    _apply(ops, hs, g, ids, hp, unique_indices=t == 2)
  _same(ops, hs, models, ids)
  assert not _rows(ops, hs[0], ids[:5]).any() and not _rows(ops, hs[1], ids[3:9]).any()
  assert (_rows(ops, hs[0], ids[5:]) != before[5:]).all()
  assert [m["freq"] for m in ops.kv_get_meta(hs[0], ids)] == [5 if wd else 1] * ids.size
  assert [m["freq"] for m in ops.kv_get_meta(hs[1], ids)] == [4] * ids.size


def test_argument_errors_queue_nothing(ops):
  from tfplus_amd import _lib
  D = 8
  hs = _pair(ops, D, np.ones((4, D), F))
  ids, g = np.arange(3, dtype=np.int64), np.full((3, D), 0.1, F)
  inv, pre = _lib.InvalidArgumentError, _lib.FailedPreconditionError
  bad = lambda i, v: HP[:i] + (v,) + HP[i + 1:]
  wide = lambda k: ops.kv_variable([k * D])                       # (not initialised)
  t1, t2 = wide(1), wide(2)
  for k, h in ((1, t1), (2, t2)):
    ops.init_kv_variable_v2(h, np.zeros((4, k * D), F))
  cases = [(hs, bad(0, 0.0), inv, "lr_t"), (hs, bad(1, 1.0), inv, "beta1_power"), (hs, bad(2, 1.5), inv, "beta2_power"),
           (hs, bad(6, -0.1), inv, "weight_decay"), (hs, bad(8, 2), inv, "0 or 1"), (hs, bad(10, -1), inv, "0 or 1"),
           ([hs[0], hs[0]], HP, inv, "same table"), ([hs[0], t1], HP, inv, "opt must be 3x"), ([hs[0], t2], HP, inv, "opt must be 3x"),
           ([hs[0], wide(3)], HP, pre, "opt"), ([wide(1), hs[1]], HP, pre, "var")]
  for (tabs, hp, exc, word), kw in itertools.product(cases, ({}, {"unique_indices": True})):
    with pytest.raises(exc, match=word):
      _apply(ops, tabs, g, ids, hp, **kw)
  with pytest.raises(inv, match="0 or 1"):                        # a flag in the generic entries' float vector
    ops.kv_variable_apply_sparse("rectified_adam", hs, bad(9, 0.5), g, ids, np.arange(3), None, 3, "sum")
  with pytest.raises(inv, match="optimizer 8 reads 11"):            # another family's vector is not read past its end
    ops.kv_variable_apply_sparse("rectified_adam", hs, HP[:6], g, ids, np.arange(3), None, 3, "sum")
  with pytest.raises(inv, match="opt must be 3x"):
    ops.kv_multi_sparse_apply_rectified_adam([hs[0]], [t2], [g], [ids], *HP)
  if torch.cuda.device_count() > 1:
    other = ops.kv_variable([3 * D], device=1)
    ops.init_kv_variable_v2(other, np.zeros((4, 3 * D), F))
    with pytest.raises(inv, match="different devices"):
      _apply(ops, [hs[0], other], g, ids)
  torch.cuda.synchronize()
  assert all(int(ops.kv_variable_shape_v2(h)[0]) == 0 and ops.kv_variable_frequency(h) == 0 for h in hs)


def test_optimizer_fused_equals_the_composition(ops):
  """twin variables, distinct ids per step: records equal, rows at the Adam twin test's tolerance (rtol 1e-6, atol 1e-9)"""
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import kv_variable_ops, variable_scope as vs
  vs.reset_default_store()
  kv_variable_ops.set_training(True)
  D, rng = 16, np.random.default_rng(3)
  kw = dict(weight_decay=0.01, amsgrad=True, use_nesterov=True)
  kvs = [vs.get_kv_variable("radam_%d" % f, embedding_dim=D, initializer=vs.ones_initializer) for f in (0, 1)]
  opts = [training.RectifiedAdamOptimizer(0.01, fused=bool(f), **kw) for f in (0, 1)]
  for o in opts:                                                  # steps 4, 5, 6: sma_t passes the threshold of 5 on the way
    o._step, o._beta1_power, o._beta2_power = F(4), F(0.9) ** 4, F(0.999) ** 4
  for t in range(3):
    ids = rng.choice(60, 40, replace=False).astype(np.int64)
    g = rng.normal(0, 0.1, (40, D)).astype(F)
    for opt, kv in zip(opts, kvs):
      opt.apply_gradients([(kv_variable_ops.IndexedSlices(torch.from_numpy(g), torch.from_numpy(ids), None), kv)])
  assert opts[1].get_slot_names() == ["m_v_vhat"] and opts[1]._native_step(kvs[1])[0] == "rectified_adam"
  slot, keys = opts[1].get_slot(kvs[1], "m_v_vhat").handle, np.arange(60)      # (a key a table does not hold: no record)
  fused = _rows(ops, slot, keys)
  assert not np.isnan(fused).any() and [o._step_scalars()[3] for o in opts] == [True, True]
  for j, comp in enumerate([kvs[0].handle] + [opts[0].get_slot(kvs[0], name).handle for name in ("m", "v", "vhat")]):
    h, got = (kvs[1].handle, _rows(ops, kvs[1].handle, keys)) if j == 0 else (slot, fused[:, (j - 1) * D:j * D])
    np.testing.assert_allclose(got, _rows(ops, comp, keys), rtol=1e-6, atol=1e-9)
    assert ops.kv_get_meta(comp, keys) == ops.kv_get_meta(h, keys)   # (every slot block is non-zero: one flag says the same)


def test_captured_tok_step_replays_on_fresh_ids(ops):
  dev = torch.device("cuda", 0)
  D, n = 32, 4000
  gen = torch.Generator(device=dev).manual_seed(3)
  ids, grad = torch.randperm(8000, device=dev, generator=gen)[:n], torch.randn(n, D, device=dev, generator=gen) * 1e-2
  cap, eag = [_pair(ops, D, np.full((16, D), 0.01, F), cap=8 * n) for _ in range(2)]
  for hs in (cap, eag):
    ops.kv_variable_gather_or_insert_v2(hs[0], ids)
    _apply(ops, hs, grad, ids)                                    # warm-up outside the capture: rows, hints, workspace
  torch.cuda.synchronize()
  for h in cap:
    ops.kv_prepare_capture(h, 4 * n)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    ops.kv_variable_gather_or_insert_v2(cap[0], ids)
    _apply(ops, cap, grad, ids)
  seen = [ids.cpu().numpy()]
  for rep in range(3):
    ids.copy_(torch.randperm(8000, device=dev, generator=gen)[:n] + 2000 * rep)     # fresh ids, new keys among them
    seen.append(ids.cpu().numpy())
    graph.replay()
    ops.kv_variable_gather_or_insert_v2(eag[0], ids)
    _apply(ops, eag, grad, ids)
  torch.cuda.synchronize()
  _same(ops, cap, eag, np.unique(np.concatenate(seen)))
