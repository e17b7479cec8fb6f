"""GPU checks of the group RectifiedAdam op (kvhip.h kv_apply_group_rectified_adam and its forms): parity with the NumPy
restatement tests/_radam_ref.py (rows bit for bit where the group-lasso scale is exactly 1; frequency words, flags and
sizes against the oracle's GroupAdam V3 run on the same ids), blacklisting and its lifting, the frequency filter, the
_unique / _tok / batched / sharded forms against the plain op, repeated ids, slot mirrors, the Python optimizer against
the restatement and against the composite RectifiedAdamOptimizer, and a captured step."""
import os
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _radam_ref as R  # noqa: E402
from oracle import kv_oracle as ko  # noqa: E402  (checker only: TF-core's de-duplication, GroupAdam V3's bookkeeping)

DAY = 20000
F = np.float32
RTOL = 1e-6          # tests/test_gpu_parity.py's bar for GroupAdam state


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _table(ops, D, init, thr=0, seed=5, cap=0):
  h = ops.kv_variable([D], enter_threshold=thr, capacity_hint=cap)
  ops.kv_set_clock_days(h, DAY)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, np.asarray(init, F))
  return h


def _var_init(rng, D):
  """Rows of two magnitudes, all positive: a new key's row (the mean of two of them) is either ~0.04 or ~4e-5, so the
  rows' lasso norms fall into separate groups whatever D is."""
  t = rng.uniform(0.5, 1.0, (64, D)) * 0.05
  t[::2] *= 1e-3
  return t.astype(F)


def _pair(ops, D, rng, thr=0, cap=0, init=None):
  return (_table(ops, D, _var_init(rng, D) if init is None else init, thr, cap=cap),
          _table(ops, 5 * D, np.zeros((16, 5 * D), F), cap=cap))


def _beta_pows(t):
  p1, p2 = F(0.9), F(0.999)
  for _ in range(t):
    p1, p2 = F(p1 * F(0.9)), F(p2 * F(0.999))
  return float(p1), float(p2)


def _hp(t, lr=0.1, l1=0.0, l2=0.0, l21=0.0, r_t=0.4, tractable=False, amsgrad=False, nesterov=False):
  """The op's thirteen scalars in its order."""
  b1p, b2p = _beta_pows(t)
  return (lr, b1p, b2p, 0.9, 0.999, 1e-7, l1, l2, l21, r_t, tractable, amsgrad, nesterov)


def _apply(ops, hs, grad, ids, hp, **kw):
  ops.kv_variable_group_sparse_apply_rectified_adam(hs[0], hs[1], grad, ids, *hp, **kw)


def _state(ops, hs, u):
  """(x, slot, live, new): the rows the step starts from (a slot row that does not exist yet starts from the slot
  table's init value, zeros), which keys pass the frequency filter, which slot rows the step creates."""
  x = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], u))
  sl = _np(ops.kv_variable_gather_or_zeros_v2(hs[1], u))
  mv, ms = ops.kv_get_meta(hs[0], u), ops.kv_get_meta(hs[1], u)
  thr = hs[0].enter_threshold
  live = np.array([m is not None and m["freq"] >= thr for m in mv])
  return x, sl, live, np.array([m is None for m in ms]), mv, ms


def _expect(ops, hs, u, s, hp):
  """What one step on unique ids u with summed rows s leaves, from the tables' state now: (rows, metas, updated)."""
  x, sl, live, news, mv, ms = _state(ops, hs, u)
  x1, s1, upd = R.group_radam(x, sl, s, *hp)
  ex = [np.where(live[:, None], x1, x), np.where(live[:, None], s1, sl)]
  ux, us = R.under_threshold(x1), R.under_threshold(s1)
  metas = [[], []]
  for i in range(u.size):
    if not live[i]:
      metas[0].append(mv[i]); metas[1].append(ms[i])
      continue
    metas[0].append({"freq": mv[i]["freq"], "day": mv[i]["day"], "blacklist": not upd[i],
                     "under_threshold": bool(ux[i]) if upd[i] else True})
    if news[i]:
      metas[1].append({"freq": 1, "day": 0, "blacklist": False, "under_threshold": bool(us[i])})
    else:
      metas[1].append({"freq": min(ms[i]["freq"] + 1, 65535), "day": DAY, "blacklist": ms[i]["blacklist"],
                       "under_threshold": bool(us[i])})
  return ex, metas, upd


def _bits(a, b):
  return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _check(ops, hs, u, ex, metas, var_tol=None):
  """var_tol None: the var bit for bit; else its per-element tolerance.  The slot row never depends on the norm: always
  bit for bit.  Frequency words and flags: exact."""
  got = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], u))
  if var_tol is None:
    assert _bits(got, ex[0]), np.argwhere(got != ex[0])[:5]
  else:
    bad = np.abs(got.astype(np.float64) - ex[0]) > var_tol
    assert not bad.any(), (np.argwhere(bad)[:5], np.abs(got - ex[0]).max())
  gs = _np(ops.kv_variable_gather_or_zeros_v2(hs[1], u))
  assert _bits(gs, ex[1]), np.argwhere(gs != ex[1])[:5]
  assert ops.kv_get_meta(hs[0], u) == metas[0]
  assert ops.kv_get_meta(hs[1], u) == metas[1]


def _lasso_tol(x, sl, s, hp, ex_var):
  """tests/test_gpu_parity.py's bar for a GroupAdam var under l21 > 0: the norm is summed in another order, which moves it
  by an ulp that 1 - thr / norm amplifies by 1 / scale -> 1e-6 / scale of the value + 1e-9.  Asserts that no key is
  within 1e-3 of the threshold (so that no decision can flip and scale >= ~1e-3)."""
  ratio = R.norm_over_threshold(x, sl, s, *hp)
  assert not (np.abs(ratio - 1.0) < 1e-3).any(), ratio[np.abs(ratio - 1.0) < 1e-3]
  with np.errstate(divide="ignore"):
    scale = np.where(ratio > 1.0, 1.0 - 1.0 / ratio, 1.0)
  return RTOL / scale[:, None] * np.abs(ex_var) + 1e-9


def _pick_regularizers(x, sl, s, hp0):
  """l1 = the median |linear'| (about half the elements clamped) and, with it, l21 in the widest gap of the rows' norms
  between the 10th and the 90th percentile — inputs, chosen so that both lasso branches occur and no key sits at the
  threshold.  -> (l1, l21)."""
  D = x.shape[1]
  z1 = R.group_radam(x, sl, s, *hp0)[1][:, 2 * D:3 * D]
  l1 = float(np.median(np.abs(z1)))
  hp1 = hp0[:6] + (l1,) + hp0[7:]
  n = R.row_norms(x, sl, s, *hp1)
  n = np.sort(n[n > 0])                                   # (a row whose elements are all clamped has norm 0)
  lo, hi = n.size // 10, n.size - n.size // 10
  gap = n[lo + 1:hi] / n[lo:hi - 1]
  k = int(np.argmax(gap))
  assert gap[k] > 1.01, gap[k]
  return l1, float(np.sqrt(n[lo + k] * n[lo + k + 1]) / np.sqrt(D))


# ---- 1. parity with the restatement at the op boundary (unique ids) ---------------------------------------------------
BRANCHES = {"plain": dict(tractable=False), "tractable": dict(tractable=True), "amsgrad": dict(tractable=True, amsgrad=True)}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
@pytest.mark.parametrize("D", [4, 8, 32, 64, 256, 1, 7, 12])          # entry-list kernels; 1, 7, 12: the fallback pipeline
def test_parity_unique_ids(ops, D, branch):
  for nesterov in (False, True):
    rng = np.random.default_rng(1000 + D + (50 if nesterov else 0))
    kw = dict(BRANCHES[branch], nesterov=nesterov)
    # (a) l1 = l2 = l21 = 0: scale is exactly 1 -> var and all five slot blocks bit for bit; the math cannot blacklist, so the
    #     frequency words, flags and sizes are those of the oracle's GroupAdam V3 run on the same ids
    # (b) l1 > 0 (about half the elements clamped), l2 > 0, l21 = 0: still bit for bit
    # (c) l1, l2, l21 > 0: the norm decides and scales -> the parity file's tolerance on the var
    for cfg in "abc":
      init = _var_init(rng, D)
      hs = _pair(ops, D, rng, init=init)
      ov = ko.OracleKv(D, 0, init, day=DAY, picker=1, seed=5)
      o3 = ko.OracleKv(3 * D, 0, np.zeros((16, 3 * D), F), day=DAY, picker=1, seed=5)
      for t in range(2):                                                # two steps: vhat and vamsgrad non-zero going in
        ids = rng.choice(1500 + 500 * t, 600, replace=False).astype(np.int64)     # new keys arrive in step 2
        grad = (rng.normal(0, 1, (ids.size, D)) * rng.choice([1e-1, 1e-3], (ids.size, 1))).astype(F)
        got = _np(ops.kv_variable_gather_or_insert_v2(hs[0], ids))
        want = ov.gather_or_insert(ids)          # (the oracle's rows follow GroupAdam's math: only its bookkeeping is used)
        if t == 0:
          np.testing.assert_array_equal(got, want)
        hp = _hp(t, **kw)
        var_tol = None
        if cfg != "a":
          x, sl = _state(ops, hs, ids)[:2]
          l1, l21 = _pick_regularizers(x, sl, grad, hp)
          hp = _hp(t, l1=l1, l2=1e-2, l21=l21 if cfg == "c" else 0.0, **kw)
          z1 = R.group_radam(x, sl, grad, *hp)[1][:, 2 * D:3 * D]
          assert 0.2 < (np.abs(z1) <= F(l1)).mean() < 0.8                     # some elements clamped, some not
        ex, metas, upd = _expect(ops, hs, ids, grad, hp)
        if cfg == "c":
          var_tol = _lasso_tol(*_state(ops, hs, ids)[:2], grad, hp, ex[0])
          assert 0 < upd.sum() < upd.size, upd.sum()                         # both lasso branches
        elif cfg == "a":
          assert upd.all()                         # ((b): a row whose elements are all clamped has norm 0 and is blacklisted)
        _apply(ops, hs, grad, ids, hp)
        _check(ops, hs, ids, ex, metas, var_tol)
        if cfg == "a":
          ko.apply_group_adam(ov, o3, grad, ids, hp[0], hp[1], hp[2], 0.9, 0.999, 1e-8, version=3)
          assert ops.kv_get_meta(hs[0], ids) == [ov.meta(int(k)) for k in ids]
          assert ops.kv_get_meta(hs[1], ids) == [o3.meta(int(k)) for k in ids]
          for h, o in ((hs[0], ov), (hs[1], o3)):
            assert ops.kv_variable_size_v2(h) == o.size() and ops.kv_variable_frequency(h) == o.sum_freq()
            assert ops.kv_variable_shape_v2(h)[0] == o.map_size()


# ---- 2. blacklist and its lifting ----------------------------------------------------------------------------------------
def test_blacklist_then_unblacklist(ops):
  D = 8
  hs = [_table(ops, D, np.zeros((16, D), F)), _table(ops, 5 * D, np.zeros((16, 5 * D), F))]
  ids = np.arange(4, dtype=np.int64)
  for t, scale in enumerate((1e-3, 1e-3, 50.0)):       # var 0: linear follows m / (1 - b1p); small -> norm <= l21 sqrt(D)
    ops.kv_variable_gather_or_insert_v2(hs[0], ids)
    grad = np.full((4, D), scale, F) * np.linspace(1, 2, D, dtype=F)
    hp = _hp(0, l21=0.5)
    x, sl = _state(ops, hs, ids)[:2]
    ex, metas, upd = _expect(ops, hs, ids, grad, hp)
    assert upd.all() == (t == 2) and (not upd.any()) == (t < 2)
    tol = _lasso_tol(x, sl, grad, hp, ex[0])
    _apply(ops, hs, grad, ids, hp)
    _check(ops, hs, ids, ex, metas, tol)               # slot rows and frequency words: exact throughout
    assert [m["blacklist"] for m in ops.kv_get_meta(hs[0], ids)] == [t < 2] * 4
    rows = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], ids))
    assert (rows == 0).all() == (t < 2) and (t < 2 or (rows != 0).all())
    np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_v2(hs[0], ids)), rows)      # training lookup too
    ops.kv_variable_gather_or_zeros_v2(hs[0], ids)


def test_enter_threshold(ops):
  rng = np.random.default_rng(77)
  D = 16
  hs = _pair(ops, D, rng, thr=2)
  seen = rng.choice(2000, 800, replace=False).astype(np.int64)
  ops.kv_variable_gather_or_insert_v2(hs[0], seen)
  ops.kv_variable_gather_or_insert_v2(hs[0], seen[:400])                          # half reach the threshold
  grad = rng.normal(0, 0.05, (seen.size, D)).astype(F)
  hp = _hp(0, l2=1e-2, tractable=True)
  before = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], seen))
  ex, metas, _ = _expect(ops, hs, seen, grad, hp)
  _apply(ops, hs, grad, seen, hp)
  _check(ops, hs, seen, ex, metas)
  assert _bits(_np(ops.kv_variable_gather_or_zeros_v2(hs[0], seen[400:])), before[400:])       # filtered: left alone
  assert ops.kv_get_meta(hs[1], seen[400:]) == [None] * 400 and ops.kv_variable_size_v2(hs[1]) == 400


# ---- 3. the three forms agree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 12, 32])
def test_plain_unique_tok_forms_agree(ops, D):
  rng = np.random.default_rng(50 + D)
  init = _var_init(rng, D)
  twins = [_pair(ops, D, rng, init=init) for _ in range(3)]
  for t in range(3):
    hp = _hp(t, l1=1e-3, l2=1e-2, l21=1e-3, tractable=t > 0, amsgrad=True)
    ids = torch.from_numpy(rng.choice(4000, 1500, replace=False).astype(np.int64)).cuda()
    grad = torch.from_numpy(rng.normal(0, 0.05, (ids.numel(), D)).astype(F)).cuda()
    ops.kv_variable_gather_or_insert_v2(twins[0][0], ids.clone())
    ops.kv_variable_gather_or_insert_v2(twins[1][0], ids.clone())
    ops.kv_variable_gather_or_insert_v2(twins[2][0], ids)                    # the lookup's token goes with these ids
    _apply(ops, twins[0], grad, ids.clone(), hp)
    _apply(ops, twins[1], grad, ids.clone(), hp, unique_indices=True)
    _apply(ops, twins[2], grad, ids, hp)
    for k in range(2):
      r0 = _np(ops.kv_variable_gather_or_zeros_v2(twins[0][k], ids))
      for j in (1, 2):
        assert _bits(r0, _np(ops.kv_variable_gather_or_zeros_v2(twins[j][k], ids))), (t, j, k)
        assert ops.kv_get_meta(twins[j][k], ids) == ops.kv_get_meta(twins[0][k], ids)


def test_broken_unique_promise_is_reported(ops):
  from tfplus_amd import _lib
  rng = np.random.default_rng(9)
  D = 16
  hs = _pair(ops, D, rng)
  ids = np.array([1, 2, 3, 2, 5], np.int64)
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  _apply(ops, hs, grad, ids, _hp(0), unique_indices=True)
  with pytest.raises(_lib.InvalidArgumentError):
    _apply(ops, hs, grad[:1], ids[:1], _hp(0))
    torch.cuda.synchronize()


# ---- 4. repeated ids -----------------------------------------------------------------------------------------------------
def _reorder_bound(x, sl, u_s, g_abs, cnt, hp):
  """tests/_reorder.py's method: the step in float64 at gsum, gsum - dg and gsum + dg, dg = (cnt - 1) 2^-24 sum|g| (every
  float32 order of the same addends stays inside) -> expected rows and, per element, twice the largest excursion plus the
  float32 evaluation of the step itself: 1e-6 of the value, and for m', for linear' = linear + rm - (rv - vhat) x and for
  the var -linear' / rv a few ulps (2^-22) of the largest of the terms that cancel (tests/_reorder.py adam_eval_err)."""
  D = x.shape[1]
  f64 = lambda s: R.group_radam(x, sl, s, *hp, dtype=np.float64)[:2]
  e0 = f64(u_s)
  dg = (cnt - 1)[:, None] * g_abs * 2.0 ** -24
  dev = [np.zeros_like(e) for e in e0]
  for sg in (1, -1):
    for d, a, b in zip(dev, e0, f64(u_s + sg * dg)):
      np.maximum(d, np.abs(b - a), out=d)
  z0, vh = sl[:, 2 * D:3 * D].astype(np.float64), sl[:, 3 * D:4 * D].astype(np.float64)
  z1, rv = e0[1][:, 2 * D:3 * D], e0[1][:, 3 * D:4 * D]
  rm = z1 - z0 + (rv - vh) * x
  # m' = b1 m + (1 - b1) g is itself a sum of two terms of opposite sign when the gradient turns against the momentum
  mterms = 2.0 ** -22 * (0.9 * np.abs(sl[:, :D].astype(np.float64)) + 0.1 * np.abs(u_s))
  c1 = float(R.host_scalars(hp[1], hp[2])[1])
  cancel = 2.0 ** -22 * (np.abs(z0) + np.abs(rm) + np.maximum(rv, vh) * np.abs(x)) + mterms / c1
  bound = [2 * dev[0] + 1e-6 * np.abs(e0[0]) + cancel / rv + 1e-12, 2 * dev[1] + 1e-6 * np.abs(e0[1]) + 1e-12]
  bound[1][:, :D] += mterms
  bound[1][:, 2 * D:3 * D] += cancel
  return e0, bound


def test_repeated_ids_default_and_occurrence_order(ops):
  rng = np.random.default_rng(31)
  D = 32
  for occ in (False, True):
    hs = _pair(ops, D, rng)
    if occ:
      ops.kv_set_deterministic(hs[0], ops.KV_ORDER_OCCURRENCE)
    for t in range(3):
      hp = _hp(t, tractable=t > 0, amsgrad=t > 1)
      ids = rng.zipf(1.2, 6000).astype(np.int64) % 2000
      grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
      ops.kv_variable_gather_or_insert_v2(hs[0], ids)
      u, s, _ = ko.dedup_segment_sum(ids, grad)                           # TF-core's occurrence order
      x, sl = _state(ops, hs, u)[:2]
      if occ:    # a repeated id's rows are added one by one in input order: the unique-id bar for every key
        ex, metas, _ = _expect(ops, hs, u, s, hp)
        _apply(ops, hs, grad, ids, hp)
        _check(ops, hs, u, ex, metas)
        continue
      order = np.argsort(u)
      pos = order[np.searchsorted(u[order], ids)]                          # every occurrence's row in u
      cnt = np.bincount(pos, minlength=u.size)
      ga = np.zeros((u.size, D)); np.add.at(ga, pos, np.abs(grad.astype(np.float64)))
      gs = np.zeros((u.size, D)); np.add.at(gs, pos, grad.astype(np.float64))
      ex, bound = _reorder_bound(x, sl, gs, ga, cnt, hp)
      _apply(ops, hs, grad, ids, hp)
      for h, e, b in zip(hs, ex, bound):
        got = _np(ops.kv_variable_gather_or_zeros_v2(h, u)).astype(np.float64)
        bad = np.abs(got - e) > b
        assert not bad.any(), (t, np.argwhere(bad)[:5], np.abs(got - e)[bad][:5], b[bad][:5])


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks(ops):
  from tfplus_amd import _lib
  rng = np.random.default_rng(2)
  D = 8
  hs = _pair(ops, D, rng)
  ids, g = np.arange(3, dtype=np.int64), np.zeros((3, D), F)
  for bad in (dict(lr=0.0), dict(lr=-1.0), dict(l1=-1.0), dict(l2=-1.0), dict(l21=-1.0)):
    with pytest.raises(_lib.InvalidArgumentError):
      _apply(ops, hs, g, ids, _hp(0, **bad))
  for mult in (1, 3, 4):                                    # only 5 x the var's dim is a slot row
    with pytest.raises(_lib.InvalidArgumentError):
      _apply(ops, [hs[0], _table(ops, mult * D, np.zeros((4, mult * D), F))], g, ids, _hp(0))
  with pytest.raises(_lib.FailedPreconditionError):
    _apply(ops, [hs[0], ops.kv_variable([5 * D])], g, ids, _hp(0))
  with pytest.raises(_lib.FailedPreconditionError):
    _apply(ops, [ops.kv_variable([D]), hs[1]], g, ids, _hp(0))
  _apply(ops, hs, g, ids, _hp(0))                             # ... and the pair itself is fine


# ---- 6. batched: bit-identical to the per-table op ---------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "tok", "unique"])
def test_batched_equals_per_table(ops, form):
  rng = np.random.default_rng(61)
  dims, lens = [8, 8, 32, 32, 64, 64], [700, 1300, 900, 400, 1100, 600]       # three dims, every table its own batch length
  single, multi = [], []
  for D in dims:
    init = _var_init(rng, D)
    single.append(_pair(ops, D, rng, init=init))
    multi.append(_pair(ops, D, rng, init=init))
  for t in range(2):
    hp = _hp(t, l1=1e-3, l2=1e-2, l21=1e-3, tractable=t > 0, amsgrad=True, nesterov=True)
    ids = [torch.from_numpy(rng.choice(4000, n, replace=False).astype(np.int64)).cuda() for n in lens]
    grads = [torch.from_numpy(rng.normal(0, 5e-2, (n, D)).astype(F)).cuda() for n, D in zip(lens, dims)]
    for k in range(len(dims)):
      ops.kv_variable_gather_or_insert_v2(single[k][0], ids[k].clone())
      _apply(ops, single[k], grads[k], ids[k].clone(), hp)
    for same_dim in (8, 32, 64):
      ks = [k for k, D in enumerate(dims) if D == same_dim]
      if form == "tok":                                       # the batched lookup's tokens go with these very tensors
        ops.kv_multi_gather_or_insert([multi[k][0] for k in ks], [ids[k] for k in ks])
        batch = [ids[k] for k in ks]
      else:
        for k in ks:
          ops.kv_variable_gather_or_insert_v2(multi[k][0], ids[k].clone())
        batch = [ids[k].clone() for k in ks]
      ops.kv_multi_group_sparse_apply_rectified_adam([multi[k][0] for k in ks], [multi[k][1] for k in ks],
                                                     [grads[k] for k in ks], batch, *hp, unique_indices=form == "unique")
    for k in range(len(dims)):
      for j in range(2):
        a = _np(ops.kv_variable_gather_or_zeros_v2(single[k][j], ids[k]))
        b = _np(ops.kv_variable_gather_or_zeros_v2(multi[k][j], ids[k]))
        assert _bits(a, b), (t, k, j)
        assert ops.kv_get_meta(single[k][j], ids[k]) == ops.kv_get_meta(multi[k][j], ids[k])


# ---- 7. sharded: optimizer code 6 through staged communicators --------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_matches_single_table(ops, world):
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76 + world)
  D = 16
  init = _var_init(rng, D)
  mk = lambda: [_table(ops, D, init, seed=3), _table(ops, 5 * D, np.zeros((16, 5 * D), F))]
  ref = mk()
  parts = [mk() for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  dev = torch.device("cuda", 0)
  bar = threading.Barrier(world, timeout=120)
  sent, vals = [None] * world, [0] * world

  def make_comm(r):
    def exchange(send, recv, per_peer):
      n = per_peer * world
      sent[r] = ops.KvCommStaged.raw(send, n, dev)
      torch.cuda.synchronize()
      bar.wait()
      dst = ops.KvCommStaged.raw(recv, n, dev)
      for p in range(world):
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
  for step in range(3):
    hp = _hp(step, l1=1e-3, l2=1e-2, l21=1e-3, tractable=step > 0, amsgrad=step > 1)
    ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
    grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]
    errs = []

    def rank_step(r):
      try:
        torch.cuda.set_device(0)
        ops.kv_multi_shard_lookup([shs[r]], comms[r], [torch.from_numpy(ids[r]).cuda()])
        torch.cuda.synchronize()
        ops.kv_multi_shard_apply([shs[r]], comms[r], ops.OPT_GROUP_RADAM, [[parts[r][1]]], [torch.from_numpy(grads[r]).cuda()],
                                 [float(v) for v in hp])
        torch.cuda.synchronize()
      except Exception as e:
        errs.append((r, repr(e)))
        bar.abort()
    ts = [threading.Thread(target=rank_step, args=(r,)) for r in range(world)]
    for t in ts:
      t.start()
    for t in ts:
      t.join()
    assert not errs, errs
    bar.reset()
    allids, allg = np.concatenate(ids), np.concatenate(grads)
    ops.kv_variable_gather_or_insert_v2(ref[0], allids)
    _apply(ops, ref, allg, allids, hp)
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r in range(world):
    mine = u[own == r]
    for j in range(2):                                     # the bars of the FTRL file's sharded test
      np.testing.assert_allclose(_np(ops.kv_variable_gather_or_zeros_v2(parts[r][j], mine)),
                                 _np(ops.kv_variable_gather_or_zeros_v2(ref[j], mine)), rtol=2e-5, atol=2e-6)
  del comms


# ---- 8. slot mirrors -----------------------------------------------------------------------------------------------------
def test_lean_applies_on_a_presized_pair_and_an_export_in_between(ops):
  """A pre-sized (single-chunk) pair: the applies work on the var rows' mirrors of the slot records.  Nobody reads a table
  between the steps (the restatement carries the state), except one export of the SLOT table, which ends the epoch: the
  dirty mirrors go back first, and the next apply starts a new epoch."""
  rng = np.random.default_rng(88)
  D, n = 32, 1500
  hs = _pair(ops, D, rng, cap=50_000)
  ids = rng.choice(10_000, n, replace=False).astype(np.int64)
  x = _np(ops.kv_variable_gather_or_insert_v2(hs[0], ids))
  sl = np.zeros((n, 5 * D), F)
  for t in range(4):
    hp = _hp(t, l1=1e-4, l2=1e-2, tractable=t > 0, amsgrad=True)
    grad = rng.normal(0, 5e-2, (n, D)).astype(F)
    x, sl, upd = R.group_radam(x, sl, grad, *hp)
    assert upd.all()
    _apply(ops, hs, grad, ids, hp, unique_indices=t == 1)
    if t == 1:
      e0 = ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_EPOCHS)
      keys, vals = ops.kv_variable_export(hs[1])[:2]
      o = np.argsort(_np(keys))
      assert _bits(_np(vals)[o], sl[np.argsort(ids)])
      assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_EPOCHS) > e0
  assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_APPLIES) >= 3
  assert _bits(_np(ops.kv_variable_gather_or_zeros_v2(hs[0], ids)), x)
  assert _bits(_np(ops.kv_variable_gather_or_zeros_v2(hs[1], ids)), sl)
  ms = ops.kv_get_meta(hs[1], ids)
  assert [m["freq"] for m in ms] == [4] * n and [m["day"] for m in ms] == [DAY] * n


# ---- 9. the Python optimizer and a captured step ---------------------------------------------------------------------
@pytest.mark.parametrize("regs", [False, True])
def test_group_rectified_adam_optimizer_trains(ops, regs):
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import kv_variable_ops, variable_scope as vs
  vs.reset_default_store()
  kv_variable_ops.set_training(True)
  D, n = 16, 40
  kw = dict(learning_rate=0.01, beta2=0.9, amsgrad=regs, use_nesterov=regs)
  kv = vs.get_kv_variable("radam_fused_%d" % regs, embedding_dim=D, initializer=vs.ones_initializer)
  opt = training.GroupRectifiedAdamOptimizer(l1_regularization_strength=1e-3 if regs else 0.0,
                                             l2_regularization_strength=1e-2 if regs else 0.0, **kw)
  if not regs:   # all regularisers 0: the composite optimizer computes the same step from generic ops
    kvc = vs.get_kv_variable("radam_composite", embedding_dim=D, initializer=vs.ones_initializer)
    comp = training.RectifiedAdamOptimizer(**kw)
  ids = torch.arange(n)
  rng = np.random.default_rng(3)
  x, sl = np.ones((n, D), F), np.zeros((n, 5 * D), F)
  tol = np.zeros((n, D))
  tract = []

  def rows(var):
    keys, vals = var._read_variable_op()
    return vals.cpu().numpy()[np.argsort(keys.cpu().numpy())]

  for t in range(10):
    g = torch.from_numpy(rng.normal(0, 0.1, (n, D)).astype(F))
    opt._init_accumulators()
    lr_t, _, sma_t, tractable, r_t = opt._step_scalars()               # the host scalars this step is driven with
    tract.append(tractable)
    hp = (lr_t, opt._beta1_power, opt._beta2_power, 0.9, 0.9, 1e-7, 1e-3 if regs else 0.0, 1e-2 if regs else 0.0, 0.0, r_t,
          tractable, regs, regs)
    vh = sl[:, 3 * D:4 * D].copy()
    x1, sl, upd = R.group_radam(x, sl, g.numpy(), *hp)
    assert upd.all()
    opt.apply_gradients([(kv_variable_ops.IndexedSlices(g, ids, None), kv)])
    assert _bits(rows(kv), x1), (t, np.abs(rows(kv) - x1).max())
    assert _bits(rows(opt.get_slot(kv, "opt")), sl), t
    if not regs:
      comp.apply_gradients([(kv_variable_ops.IndexedSlices(g, ids, None), kvc)])
      tol += R.composite_step_tolerance(x, x1, sl[:, 3 * D:4 * D], vh)
      diff = np.abs(rows(kvc).astype(np.float64) - x1)
      print("step %d tractable %d: max |fused - composite| %.3g (tolerance there %.3g)" % (t + 1, tractable, diff.max(),
                                                                                         tol.flat[diff.argmax()]))
      assert (diff <= tol).all(), (t, diff.max(), tol.flat[diff.argmax()])
    x = x1
  assert opt.get_slot_names() == ["opt"] and opt.get_slot(kv, "opt").embedding_dim == 5 * D
  # beta2 = 0.9: sma_t passes the threshold 5 at step 6 (19 - 2 t 0.9^t / (1 - 0.9^t) = 4.58, 5.40 at t = 5, 6)
  assert tract == [False] * 5 + [True] * 5, tract


def test_captured_tok_step_replays(ops):
  dev = torch.device("cuda", 0)
  gen = torch.Generator(device=dev).manual_seed(3)
  D, n = 32, 20_000
  ids = torch.randperm(100_000, device=dev, generator=gen)[:n]
  grad = torch.randn(n, D, device=dev, generator=gen) * 1e-2
  hp = _hp(3, l1=1e-4, l2=1e-2, l21=1e-4, tractable=True, amsgrad=True)

  def pair():
    hs = [_table(ops, D, np.full((16, D), 0.01, F), cap=4 * n), _table(ops, 5 * D, np.zeros((16, 5 * D), F), cap=4 * n)]
    ops.kv_variable_gather_or_insert_v2(hs[0], ids)
    _apply(ops, hs, grad, ids, hp)                             # warm-up outside the capture: rows, hints, workspace
    return hs

  cap, eag = pair(), pair()
  torch.cuda.synchronize()
  for h in cap:
    ops.kv_prepare_capture(h, 4 * n)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=side):
    ops.kv_variable_gather_or_insert_v2(cap[0], ids)
    _apply(ops, cap, grad, ids, hp)
  for _ in range(3):
    g.replay()
    ops.kv_variable_gather_or_insert_v2(eag[0], ids)
    _apply(ops, eag, grad, ids, hp)
  torch.cuda.synchronize()
  for a, b in zip(cap, eag):
    assert torch.equal(ops.kv_variable_gather_or_zeros_v2(a, ids), ops.kv_variable_gather_or_zeros_v2(b, ids))
  assert ops.kv_variable_frequency(cap[1]) == ops.kv_variable_frequency(eag[1])
