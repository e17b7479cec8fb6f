"""GPU checks of the fused plain-Adam op (kvhip.h kv_apply_adam and its forms) against tests/_adam_ref.py, the float32
restatement of the reference's chain gather_or_insert(m_v) -> scatter_update(m_v) -> scatter_sub(var): rows, frequency
words and flags of both tables bit for bit on unique ids; the bookkeeping the group optimizers do differently; the plain /
_tok / _unique / batched / counted / sharded forms against each other; repeated ids in the three reduction orders; the
argument checks; the wrappers against the C ABI by hand; slot mirrors; AdamOptimizer(fused=True) against the composition."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _adam_ref as A  # noqa: E402
import _reorder  # noqa: E402

DAY = 20000
SEED = 5
F = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
vp, u64, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _table(ops, D, init, thr=0, seed=SEED, cap=0, key_dtype=torch.int64):
  h = ops.kv_variable([D], key_dtype=key_dtype, enter_threshold=thr, capacity_hint=cap)
  ops.kv_set_clock_days(h, DAY)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, np.asarray(init, F))
  return h


def _var_init(rng, D):
  return rng.uniform(-0.5, 0.5, (64, D)).astype(F)


def _pair(ops, D, rng, thr=0, cap=0, init=None, key_dtype=torch.int64, model=True):
  """-> ([var, m_v] handles, (var, m_v) models of tests/_adam_ref.py on the same init tables, seed and day)."""
  init = _var_init(rng, D) if init is None else init
  sinit = np.zeros((16, 2 * D), F)
  hs = [_table(ops, D, init, thr, cap=cap, key_dtype=key_dtype), _table(ops, 2 * D, sinit, cap=cap, key_dtype=key_dtype)]
  return hs, ((A.Table(D, init, SEED, DAY, thr), A.Table(2 * D, sinit, SEED, DAY)) if model else None)


def _beta_pows(t):
  p1, p2 = F(B1), F(B2)
  for _ in range(t):
    p1, p2 = F(p1 * F(B1)), F(p2 * F(B2))
  return float(p1), float(p2)


def _hp(t, lr=0.05):
  """The op's six scalars in its order, the powers those of step t."""
  return (lr,) + _beta_pows(t) + (B1, B2, EPS)


def _apply(ops, hs, grad, ids, hp, **kw):
  ops.kv_variable_sparse_apply_adam(hs[0], hs[1], grad, ids, *hp, **kw)


def _lookup(ops, hs, model, ids):
  ops.kv_variable_gather_or_insert_v2(hs[0], ids)
  if model:
    model[0].lookup(np.asarray(ids).reshape(-1))


def _bits(a, b):
  return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _check(ops, hs, model, keys):
  """Rows, frequency words, flags and blacklists at `keys` and the key count, of both tables, against the models."""
  keys = np.asarray(keys, np.int64)
  for h, m in zip(hs, model):
    got, want = _np(ops.kv_variable_gather_or_zeros_v2(h, keys)), m.read(keys)
    assert _bits(got, want), (np.argwhere(got != want)[:5], np.abs(got - want).max())
    assert ops.kv_get_meta(h, keys) == m.metas(keys)
    assert int(ops.kv_variable_shape_v2(h)[0]) == len(m.rows)


def _same_tables(ops, a, b, keys):
  for x, y in zip(a, b):
    assert _bits(_np(ops.kv_variable_gather_or_zeros_v2(x, keys)), _np(ops.kv_variable_gather_or_zeros_v2(y, keys)))
    assert ops.kv_get_meta(x, keys) == ops.kv_get_meta(y, keys)
    assert int(ops.kv_variable_shape_v2(x)[0]) == int(ops.kv_variable_shape_v2(y)[0])


# ---- 1. parity with the restatement at the op boundary (unique ids) ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 2049])                         # 2049 crosses one 2048-id tile
@pytest.mark.parametrize("D", [4, 8, 32, 64, 128, 256, 1, 5, 12, 260])   # entry-list kernels; 1, 5, 12, 260: the fallback
def test_parity_unique_ids(ops, D, n):
  rng = np.random.default_rng(1000 + D + n)
  hs, model = _pair(ops, D, rng)
  seen = []
  for t in range(3):                                                # three steps with advancing powers
    ids = (rng.choice(3 * n + 40 + n * t, n, replace=False).astype(np.int64) - n // 2)        # negative keys; new ones each step
    grad = (rng.normal(0, 1, (n, D)) * rng.choice([1e-1, 1e-3], (n, 1))).astype(F)
    _lookup(ops, hs, model, ids[::2])                               # half come from a lookup, the others the op inserts
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t))
    seen.append(ids)
    _check(ops, hs, model, np.unique(np.concatenate(seen)))
  assert ops.kv_variable_frequency(hs[1]) == sum((m["freq"] for m in model[1].metas(list(model[1].rows))))


def test_parity_int32_keys(ops):
  rng = np.random.default_rng(32)
  D, n = 8, 300
  hs, model = _pair(ops, D, rng, key_dtype=torch.int32)
  for t in range(3):
    ids = rng.choice(900, n, replace=False).astype(np.int32) - 200
    grad = rng.normal(0, 0.1, (n, D)).astype(F)
    _lookup(ops, hs, model, ids[::2])
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t), unique_indices=t == 1)
    _check(ops, hs, model, np.arange(-200, 700))


# ---- 2. the bookkeeping the group ops do differently ---------------------------------------------------------------------
@pytest.mark.parametrize("D,cap", [(8, 0), (8, 4096), (5, 0)])        # general path, slot mirrors (pre-sized), fallback pipeline
def test_enter_threshold_var_is_updated_all_the_same(ops, D, cap):
  rng = np.random.default_rng(70 + D)
  hs, model = _pair(ops, D, rng, thr=3, cap=cap)
  ids = rng.choice(2000, 500, replace=False).astype(np.int64)
  _lookup(ops, hs, model, ids)                                       # frequency 1: below the threshold of 3
  before = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], ids))
  for t in range(3):                                                 # (the pre-sized pair's later steps run on the mirrors)
    grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t), unique_indices=t == 2)
  _check(ops, hs, model, ids)
  assert (_np(ops.kv_variable_gather_or_zeros_v2(hs[0], ids)) != before).all()
  assert [m["freq"] for m in ops.kv_get_meta(hs[0], ids)] == [1] * ids.size      # no frequency of the var's is touched


def _blacklist(ops, h, m, keys, black):
  """The table re-imported with `black` on the blacklist; the model follows."""
  fw = np.array([m.rows[int(k)].freq for k in keys], np.uint32)
  ops.kv_variable_import(h, keys, m.read(keys), blacklist=black, freq_keys=keys, freq_values=fw)
  for k in black:
    m.blacklist(k)


@pytest.mark.parametrize("D,cap", [(8, 0), (8, 4096), (5, 0)])
def test_blacklisted_keys_stay_blacklisted_and_unwritten(ops, D, cap):
  rng = np.random.default_rng(80 + D)
  hs, model = _pair(ops, D, rng, cap=cap)
  ids = rng.choice(2000, 300, replace=False).astype(np.int64)
  _lookup(ops, hs, model, ids)
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  A.adam_step(model[0], model[1], ids, grad, *_hp(0))
  _apply(ops, hs, grad, ids, _hp(0))
  vb, sb = [int(k) for k in ids[:5]], [int(k) for k in ids[3:9]]       # var keys, slot keys; 3 and 4 in both tables
  _blacklist(ops, hs[0], model[0], ids, vb)
  _blacklist(ops, hs[1], model[1], ids, sb)
  _check(ops, hs, model, ids)                                         # the set-up itself
  for t in range(1, 4):
    grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t), unique_indices=t == 2)
    if not cap:                                                       # (a read ends the mirrors' epoch: the pre-sized pair is
      _check(ops, hs, model, ids)                                     #  read at the end only, its later steps run on the mirrors)
  _check(ops, hs, model, ids)
  if cap:
    assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_APPLIES) >= 2
  mv, ms = ops.kv_get_meta(hs[0], vb), ops.kv_get_meta(hs[1], sb)
  assert all(m["blacklist"] and m["under_threshold"] for m in mv + ms)
  assert not _np(ops.kv_variable_gather_or_zeros_v2(hs[0], vb)).any()
  assert not _np(ops.kv_variable_gather_or_zeros_v2(hs[1], sb)).any()
  assert [m["freq"] for m in ms] == [4] * len(sb)                     # ... while the gather's hit is counted


@pytest.mark.parametrize("form", ["plain", "unique"])
@pytest.mark.parametrize("D", [8, 5])
def test_key_the_var_does_not_hold_is_inserted_then_updated(ops, D, form):
  rng = np.random.default_rng(90 + D)
  hs, model = _pair(ops, D, rng)
  ids = rng.choice(5000, 400, replace=False).astype(np.int64) - 1000
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  A.adam_step(model[0], model[1], ids, grad, *_hp(0))
  _apply(ops, hs, grad, ids, _hp(0), unique_indices=form == "unique")
  _check(ops, hs, model, ids)
  mv, ms = ops.kv_get_meta(hs[0], ids), ops.kv_get_meta(hs[1], ids)
  assert all(m["freq"] == 1 and m["day"] == 0 for m in mv)            # a scatter's insert
  assert all(m["freq"] == 1 and m["day"] == DAY for m in ms)          # a gather's insert


# ---- 3. the three forms agree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 12, 32])
def test_plain_unique_tok_forms_agree(ops, D):
  rng = np.random.default_rng(50 + D)
  init = _var_init(rng, D)
  twins = [_pair(ops, D, rng, init=init, model=False)[0] for _ in range(3)]
  model = _pair(ops, D, rng, init=init)[1]
  seen = []
  for t in range(3):
    ids = torch.from_numpy(rng.choice(4000, 1500, replace=False).astype(np.int64)).cuda()
    grad = torch.from_numpy(rng.normal(0, 0.05, (ids.numel(), D)).astype(F)).cuda()
    for tw in twins[:2]:
      ops.kv_variable_gather_or_insert_v2(tw[0], ids.clone())
    ops.kv_variable_gather_or_insert_v2(twins[2][0], ids)                    # the lookup's token goes with these ids
    assert ops._token_for(twins[2][0], ids) != 0                             # ... a real kv_gather_or_insert_tok's
    model[0].lookup(_np(ids))
    A.adam_step(model[0], model[1], _np(ids), _np(grad), *_hp(t))
    _apply(ops, twins[0], grad, ids.clone(), _hp(t))
    _apply(ops, twins[1], grad, ids.clone(), _hp(t), unique_indices=True)
    _apply(ops, twins[2], grad, ids, _hp(t))
    seen.append(_np(ids))
    keys = np.unique(np.concatenate(seen))
    _check(ops, twins[0], model, keys)
    for j in (1, 2):
      _same_tables(ops, twins[0], twins[j], keys)


def test_broken_unique_promise_is_reported(ops):
  from tfplus_amd import _lib
  rng = np.random.default_rng(9)
  D = 16
  hs, _ = _pair(ops, D, rng, model=False)
  ids = np.array([1, 2, 3, 2, 5], np.int64)
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  _apply(ops, hs, grad, ids, _hp(0), unique_indices=True)
  with pytest.raises(_lib.InvalidArgumentError):
    _apply(ops, hs, grad[:1], ids[:1], _hp(0))
    torch.cuda.synchronize()


# ---- 4. repeated ids -----------------------------------------------------------------------------------------------------
def _zipf_batch(rng, n=5000, keys=300):
  """n ids over `keys` keys, Zipf-like, one id filling more than half the batch: several tiles, a hot key."""
  ids = rng.zipf(1.3, n).astype(np.int64) % keys - 20
  ids[rng.permutation(n)[:n // 2 + 100]] = 7
  return ids


def _slot_bound(m0, v0, gsum, gabs, cnt):
  """m' = b1 m + (1 - b1) g and v' = b2 v + (1 - b2) g^2 when the summed gradient moves by dg = (cnt - 1) 2^-24 sum|g|
  (tests/_reorder.py's interval), doubled, plus the float32 evaluation: a few ulps of the larger term."""
  b1, b2 = float(F(B1)), float(F(B2))
  dg = (cnt[:, None] - 1).clip(min=0) * 2.0 ** -24 * gabs
  m1, v1 = b1 * m0 + (1 - b1) * gsum, b2 * v0 + (1 - b2) * gsum * gsum
  bm = 2 * (1 - b1) * dg + 2.0 ** -22 * (np.abs(b1 * m0) + np.abs((1 - b1) * gsum)) + 1e-12
  bv = 2 * (1 - b2) * (2 * np.abs(gsum) * dg + dg * dg) + 2.0 ** -22 * v1 + 1e-14
  return np.concatenate([m1, v1], 1), np.concatenate([bm, bv], 1)


def test_repeated_ids_default_order_within_the_reorder_bound(ops):
  rng = np.random.default_rng(31)
  D = 32
  hs, _ = _pair(ops, D, rng, model=False)
  for t in range(3):
    ids = _zipf_batch(rng)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    assert np.bincount(ids + 20).max() > ids.size // 2 and ids.size > 2 * 2048
    ops.kv_variable_gather_or_insert_v2(hs[0], ids)
    u, inv, cnt = np.unique(ids, return_inverse=True, return_counts=True)
    x0 = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], u)).astype(np.float64)
    s0 = _np(ops.kv_variable_gather_or_zeros_v2(hs[1], u)).astype(np.float64)
    m0, v0 = s0[:, :D], s0[:, D:]
    _apply(ops, hs, grad, ids, _hp(t))
    hp = _reorder.adam_hp(0.05, *_beta_pows(t), eps=float(F(EPS)))
    # tests/_reorder.py steps GroupAdam V4, whose linear slot carries -(sqrt(v) + eps) x once beta1 > beta1_power: with that z
    # (and z = 0 on the first step) its update IS x - lr_t m' / (sqrt(v') + eps)
    z0 = -(np.sqrt(v0) + hp["eps"]) * x0 if hp["b1"] > hp["b1p"] else np.zeros_like(x0)
    x1 = _np(ops.kv_variable_gather_or_zeros_v2(hs[0], u))
    _reorder.adam_reorder_check(x0, m0, v0, z0, ids, grad, x1, hp, what="adam step %d" % t)
    g64 = grad.astype(np.float64)
    gsum = np.zeros((u.size, D)); np.add.at(gsum, inv, g64)
    gabs = np.zeros((u.size, D)); np.add.at(gabs, inv, np.abs(g64))
    want, bound = _slot_bound(m0, v0, gsum, gabs, cnt)
    s1 = _np(ops.kv_variable_gather_or_zeros_v2(hs[1], u)).astype(np.float64)
    bad = np.abs(s1 - want) > bound
    assert not bad.any(), (t, np.argwhere(bad)[:5], np.abs(s1 - want)[bad][:5], bound[bad][:5])


def test_repeated_ids_occurrence_order_equals_the_restatement(ops):
  rng = np.random.default_rng(33)
  D = 32
  hs, model = _pair(ops, D, rng)
  ops.kv_set_deterministic(hs[0], ops.KV_ORDER_OCCURRENCE)
  for t in range(3):
    ids = _zipf_batch(rng)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    _lookup(ops, hs, model, ids)
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t))
    _check(ops, hs, model, np.unique(ids))


def test_repeated_ids_fixed_order_is_reproducible(ops):
  rng = np.random.default_rng(35)
  D = 32
  init = _var_init(rng, D)
  runs = [_pair(ops, D, rng, init=init, model=False)[0] for _ in range(2)]
  for hs in runs:
    ops.kv_set_deterministic(hs[0], ops.KV_ORDER_FIXED)
  keys = []
  for t in range(2):
    ids = _zipf_batch(rng)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    keys.append(ids)
    for hs in runs:
      ops.kv_variable_gather_or_insert_v2(hs[0], ids)
      _apply(ops, hs, grad, ids, _hp(t))
  _same_tables(ops, runs[0], runs[1], np.unique(np.concatenate(keys)))


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks(ops):
  from tfplus_amd import _lib
  rng = np.random.default_rng(2)
  D = 8
  hs, model = _pair(ops, D, rng)
  ids, g = np.arange(3, dtype=np.int64), np.full((3, D), 0.1, F)
  inv, pre = _lib.InvalidArgumentError, _lib.FailedPreconditionError
  cases = [
      (hs, (0.0,) + _hp(0)[1:], inv, "lr is not a positive scalar"),
      (hs, (-1.0,) + _hp(0)[1:], inv, "lr is not a positive scalar"),
      (hs, (0.05, 1.0, 0.999, B1, B2, EPS), inv, "beta1_power"),
      (hs, (0.05, 0.9, 1.5, B1, B2, EPS), inv, "beta2_power"),
      ([hs[0], hs[0]], _hp(0), inv, "same table"),
      ([hs[0], _table(ops, D, np.zeros((4, D), F))], _hp(0), inv, "m_v must be 2x"),
      ([hs[0], _table(ops, 3 * D, np.zeros((4, 3 * D), F))], _hp(0), inv, "m_v must be 2x"),
      ([hs[0], ops.kv_variable([2 * D])], _hp(0), pre, "m_v"),
      ([ops.kv_variable([D]), hs[1]], _hp(0), pre, "var"),
  ]
  for tabs, hp, exc, word in cases:
    for kw in ({}, {"unique_indices": True}):
      with pytest.raises(exc, match=word):
        _apply(ops, tabs, g, ids, hp, **kw)
  # (the device test is the one line GroupAdam and group RAdam share in apply_one; the second table needs a second device)
  if torch.cuda.device_count() > 1:
    other = ops.kv_variable([2 * D], device=1)
    ops.init_kv_variable_v2(other, np.zeros((4, 2 * D), F))
    with pytest.raises(inv, match="different devices"):
      _apply(ops, [hs[0], other], g, ids, _hp(0))
  with pytest.raises(inv, match="lr is not a positive scalar"):
    ops.kv_multi_sparse_apply_adam([hs[0]], [hs[1]], [g], [ids], 0.0, *_hp(0)[1:])
  for kw in ({}, {"unique_indices": True}):                           # the batched forms' own shape check
    with pytest.raises(inv, match="m_v must be 2x"):
      ops.kv_multi_sparse_apply_adam([hs[0]], [_table(ops, 3 * D, np.zeros((4, 3 * D), F))], [g], [ids], *_hp(0), **kw)
  with pytest.raises(inv):
    ops.kv_variable_sparse_apply_adam(hs[0], hs[1], g, ids, 0.05, 1.0, 0.999, B1, B2, EPS,
                                      unique_count=torch.tensor([3], dtype=torch.int64, device="cuda"))
  torch.cuda.synchronize()
  for h in hs:                                                        # nothing was queued by any of the refusals
    assert int(ops.kv_variable_shape_v2(h)[0]) == 0 and ops.kv_variable_frequency(h) == 0
  A.adam_step(model[0], model[1], ids, g, *_hp(0))
  _apply(ops, hs, g, ids, _hp(0))                                     # ... and the pair itself is fine
  _check(ops, hs, model, ids)


# ---- 6. batched: bit-identical to the per-table op ---------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "tok", "unique"])
def test_batched_equals_per_table(ops, form):
  rng = np.random.default_rng(61)
  D, lens = 8, [700, 0, 1300]                                        # unequal n, one table with none
  single, multi = [], []
  for _ in lens:
    init = _var_init(rng, D)
    single.append(_pair(ops, D, rng, init=init, model=False)[0])
    multi.append(_pair(ops, D, rng, init=init, model=False)[0])
  seen = [[] for _ in lens]
  for t in range(2):
    ids = [torch.from_numpy(rng.choice(4000, n, replace=False).astype(np.int64)).cuda() for n in lens]
    grads = [torch.from_numpy(rng.normal(0, 5e-2, (n, D)).astype(F)).cuda() for n in lens]
    for k in range(len(lens)):
      ops.kv_variable_gather_or_insert_v2(single[k][0], ids[k].clone())
      _apply(ops, single[k], grads[k], ids[k].clone(), _hp(t))
      seen[k].append(_np(ids[k]))
    if form == "tok":                                                # the batched lookup's tokens go with these very tensors
      ops.kv_multi_gather_or_insert([m[0] for m in multi], ids)
      batch = ids
    else:
      for k in range(len(lens)):
        ops.kv_variable_gather_or_insert_v2(multi[k][0], ids[k].clone())
      batch = [i.clone() for i in ids]
    ops.kv_multi_sparse_apply_adam([m[0] for m in multi], [m[1] for m in multi], grads, batch, *_hp(t),
                                   unique_indices=form == "unique")
    for k in range(len(lens)):
      _same_tables(ops, single[k], multi[k], np.unique(np.concatenate(seen[k])))
  assert int(ops.kv_variable_shape_v2(multi[1][0])[0]) == 0


# ---- 7. binding forms: the wrapper against the C ABI written out by hand ---------------------------------------------
HAND = (0.05, 0.81, 0.998, 0.9, 0.999, 1e-7)          # lr, beta1_power, beta2_power, beta1, beta2, epsilon: all distinct


def _hand_batch(k, n=64, D=8):
  rng = np.random.default_rng(7 + k)
  return (torch.from_numpy(rng.choice(1000, n, replace=False).astype(np.int64) - 100).cuda(),
          torch.from_numpy(rng.normal(0, 0.1, (n, D)).astype(F)).cuda())


def _hand_tables(ops, k, D=8):
  rng = np.random.default_rng(40 + k)
  return _pair(ops, D, rng, model=False)[0]


@pytest.mark.parametrize("form", ["tok", "plain", "unique"])
def test_single_table_wrapper_equals_the_call_by_hand(ops, form):
  from tfplus_amd import _lib
  L = _lib.lib()
  D, n = 8, 64
  a, b = _hand_tables(ops, 0), _hand_tables(ops, 0)
  ids, grad = _hand_batch(0)
  before = ops.kv_variable_gather_or_insert_v2(a[0], ids if form == "tok" else ids.clone())
  ops.kv_variable_sparse_apply_adam(a[0], a[1], grad, ids, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, unique_indices=form == "unique")
  ids_b, st = ids.clone(), vp(torch.cuda.current_stream().cuda_stream)
  out, tok = torch.empty((n, D), dtype=torch.float32, device=ids.device), u64(0)
  assert L.kv_gather_or_insert_tok(vp(b[0].ptr), vp(ids_b.data_ptr()), None, n, vp(out.data_ptr()), ctypes.byref(tok), st) == 0
  assert form != "tok" or tok.value != 0
  args = (vp(b[0].ptr), vp(b[1].ptr), vp(grad.data_ptr()), vp(ids_b.data_ptr()), n, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7)
  if form == "tok":
    rc = L.kv_apply_adam_tok(*args, u64(tok.value), st)
  elif form == "plain":
    rc = L.kv_apply_adam(*args, st)
  else:
    rc = L.kv_apply_adam_unique(*args, st)
  assert rc == 0, L.kv_last_error()
  _same_tables(ops, a, b, _np(ids))
  assert not torch.equal(ops.kv_variable_gather_or_zeros_v2(a[0], ids), before)
  # ... and every scalar is where the formulas want it
  model = _pair(ops, D, np.random.default_rng(40))[1]
  model[0].lookup(_np(ids))
  A.adam_step(model[0], model[1], _np(ids), _np(grad), *HAND)
  _check(ops, a, model, _np(ids))


@pytest.mark.parametrize("form", ["tok", "plain", "unique"])
def test_batched_wrapper_equals_the_call_by_hand(ops, form):
  from tfplus_amd import _lib
  L = _lib.lib()
  D, n = 8, 64
  a, b = [_hand_tables(ops, k) for k in range(2)], [_hand_tables(ops, k) for k in range(2)]
  ids, grads = zip(*[_hand_batch(k) for k in range(2)])
  if form == "tok":
    ops.kv_multi_gather_or_insert([t[0] for t in a], list(ids))
  else:
    for t, i in zip(a, ids):
      ops.kv_variable_gather_or_insert_v2(t[0], i.clone())
  ops.kv_multi_sparse_apply_adam([t[0] for t in a], [t[1] for t in a], list(grads), list(ids), 0.05, 0.81, 0.998, 0.9, 0.999,
                                 1e-7, unique_indices=form == "unique")
  ids_b, st = [i.clone() for i in ids], vp(torch.cuda.current_stream().cuda_stream)
  outs = [torch.empty((n, D), dtype=torch.float32, device=ids[0].device) for _ in range(2)]
  arr = lambda ps: (vp * 2)(*ps)
  roles = [arr([t[j].ptr for t in b]) for j in range(2)]
  idp, gp, ns = arr([i.data_ptr() for i in ids_b]), arr([g.data_ptr() for g in grads]), (i64 * 2)(n, n)
  toks = (u64 * 2)()
  assert L.kv_multi_gather_or_insert_tok(2, roles[0], idp, None, ns, arr([o.data_ptr() for o in outs]), toks, st) == 0
  assert form != "tok" or (toks[0] != 0 and toks[1] != 0)
  args = (2, roles[0], roles[1], gp, idp, ns, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7)
  if form == "tok":
    rc = L.kv_multi_apply_adam_tok(*args, toks, st)
  elif form == "plain":
    rc = L.kv_multi_apply_adam(*args, st)
  else:
    rc = L.kv_multi_apply_adam_unique(*args, st)
  assert rc == 0, L.kv_last_error()
  for k in range(2):
    _same_tables(ops, a[k], b[k], _np(ids[k]))


# ---- 8. counted: the id count stays on the device --------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 32, 256])
def test_counted_equals_unique(ops, D):
  rng = np.random.default_rng(900 + D)
  init = _var_init(rng, D)
  hc, hu = _pair(ops, D, rng, init=init, model=False)[0], _pair(ops, D, rng, init=init, model=False)[0]
  seen = []
  for t in range(3):
    u0 = rng.choice(6000, 2000, replace=False).astype(np.int64) - 500
    ids = np.concatenate([u0, u0[:1000]])                             # none more than twice: a + b == b + a in every order
    rng.shuffle(ids)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    for h in (hc[0], hu[0]):
      ops.kv_variable_gather_or_insert_v2(h, ids)
    u, s, _, nu = ops.kv_dedup_segment_sum(hc[0], ids, grad, sync=False)
    assert u.numel() == ids.size and nu.is_cuda
    _apply(ops, hc, s, u, _hp(t), unique_count=nu)
    uu, su, _ = ops.kv_dedup_segment_sum(hu[0], ids, grad)
    assert int(nu.item()) == uu.numel() == 2000
    _apply(ops, hu, su, uu, _hp(t), unique_indices=True)
    seen.append(ids)
    _same_tables(ops, hc, hu, np.unique(np.concatenate(seen)))


# ---- 9. sharded: optimizer code 7 through staged communicators ---------------------------------------------------------
@pytest.mark.parametrize("world,api", [(2, "multi"), (4, "multi"), (2, "single")])   # kv_multi_shard_apply / kv_shard_apply
def test_sharded_matches_single_table(ops, world, api):
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76 + world)
  D = 16
  init = _var_init(rng, D)
  mk = lambda: [_table(ops, D, init, seed=3), _table(ops, 2 * D, np.zeros((16, 2 * D), F))]
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
    hp = _hp(step)
    ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
    grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]
    errs = []

    def rank_step(r):
      try:
        torch.cuda.set_device(0)
        if api == "multi":
          ops.kv_multi_shard_lookup([shs[r]], comms[r], [torch.from_numpy(ids[r]).cuda()])
          torch.cuda.synchronize()
          ops.kv_multi_shard_apply([shs[r]], comms[r], ops.OPT_ADAM, [[parts[r][1]]], [torch.from_numpy(grads[r]).cuda()],
                                   [float(v) for v in hp])
        else:
          shs[r].lookup(comms[r], torch.from_numpy(ids[r]).cuda())
          torch.cuda.synchronize()
          shs[r].apply(comms[r], ops.OPT_ADAM, [parts[r][1]], torch.from_numpy(grads[r]).cuda(), [float(v) for v in hp])
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
    for j in range(2):                                     # the comparison and bars of the RAdam file's sharded test
      np.testing.assert_allclose(_np(ops.kv_variable_gather_or_zeros_v2(parts[r][j], mine)),
                                 _np(ops.kv_variable_gather_or_zeros_v2(ref[j], mine)), rtol=2e-5, atol=2e-6)
  del comms


def test_shard_apply_serve_takes_code_7(ops):
  """kv_shard_apply_serve called directly, the exchanges made between two shards of one process (kv_shard_exchange_local)."""
  from tfplus_amd import _lib
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(79)
  D, world = 16, 2
  init = _var_init(rng, D)
  mk = lambda: [_table(ops, D, init, seed=3), _table(ops, 2 * D, np.zeros((16, 2 * D), F))]
  ref, parts = mk(), [mk() for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  for step in range(2):
    hp = _hp(step)
    ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
    grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]
    for r in range(world):
      shs[r].lookup_route(torch.from_numpy(ids[r]).cuda())
    ops.kv_shard_exchange_local(shs, 0)
    for r in range(world):
      shs[r].lookup_serve()
    ops.kv_shard_exchange_local(shs, 1)
    for r in range(world):
      shs[r].lookup_finish()
      shs[r].apply_route(torch.from_numpy(grads[r]).cuda())
    ops.kv_shard_exchange_local(shs, 1)
    for r in range(world):
      if step == 0:                                       # the optimizer's own checks come through the generic entry point
        with pytest.raises(_lib.InvalidArgumentError, match="beta1_power"):
          shs[r].apply_serve(ops.OPT_ADAM, [parts[r][1]], (0.05, 1.0, 0.999, B1, B2, EPS))
        with pytest.raises(_lib.InvalidArgumentError, match="optimizer 8"):
          shs[r].apply_serve(8, [parts[r][1]], hp)
      shs[r].apply_serve(ops.OPT_ADAM, [parts[r][1]], hp)
    allids, allg = np.concatenate(ids), np.concatenate(grads)
    ops.kv_variable_gather_or_insert_v2(ref[0], allids)
    _apply(ops, ref, allg, allids, hp)
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r in range(world):
    mine = u[own == r]
    for j in range(2):
      np.testing.assert_allclose(_np(ops.kv_variable_gather_or_zeros_v2(parts[r][j], mine)),
                                 _np(ops.kv_variable_gather_or_zeros_v2(ref[j], mine)), rtol=2e-5, atol=2e-6)
    assert ops.kv_get_meta(parts[r][1], mine) == ops.kv_get_meta(ref[1], mine)


# ---- 10. slot mirrors -----------------------------------------------------------------------------------------------------
def test_lean_applies_on_a_presized_pair_and_an_export_in_between(ops):
  """A pre-sized (single-chunk) pair: the applies work on the var rows' mirrors of the slot records.  Nobody reads a table
  between the steps (the restatement carries the state), except one export of the SLOT table, which ends the epoch: the
  dirty mirrors go back first — the export sees the flushed frequency words — and the next apply starts a new epoch."""
  rng = np.random.default_rng(88)
  D, n = 32, 1500
  hs, model = _pair(ops, D, rng, cap=50_000)
  ids = rng.choice(10_000, n, replace=False).astype(np.int64)
  _lookup(ops, hs, model, ids)
  for t in range(4):
    grad = rng.normal(0, 5e-2, (n, D)).astype(F)
    A.adam_step(model[0], model[1], ids, grad, *_hp(t))
    _apply(ops, hs, grad, ids, _hp(t), unique_indices=t == 1)
    if t == 1:
      e0 = ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_EPOCHS)
      keys, vals, _, fk, fv = ops.kv_variable_export(hs[1])
      o = np.argsort(_np(keys))
      assert _bits(_np(vals)[o], model[1].read(np.sort(ids)))
      fo = np.argsort(_np(fk))
      assert np.array_equal(_np(fk)[fo], np.sort(ids))
      assert (_np(fv)[fo].view(np.uint32) == ((DAY << 16) | 2)).all()          # two hits each, both flushed
      assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_EPOCHS) > e0
  assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_APPLIES) >= 3
  _check(ops, hs, model, ids)
  ms = ops.kv_get_meta(hs[1], ids)
  assert [m["freq"] for m in ms] == [4] * n and [m["day"] for m in ms] == [DAY] * n


# ---- 11. the optimizer ---------------------------------------------------------------------------------------------------
def _table_state(kv):
  """key -> (row, frequency word) of every key, and the blacklist, from a full export."""
  k, v, bl, fk, fv = (_np(t) for t in kv.export(first_n=6))
  rows = dict(zip(k.tolist(), v))
  return rows, dict(zip(fk.tolist(), fv.view(np.uint32).tolist())), sorted(bl.tolist())


def _assert_twins(ops, a, b, tol):
  """(var, m_v) twins: key sets, frequency words, flags and blacklists EQUAL; rows within rtol 1e-6 / atol 1e-9, widened per
  element by tol: key -> [var, m, v] reorder bounds ([D] each)."""
  for j, (x, y) in enumerate(zip(a, b)):
    rx, fx, bx = _table_state(x)
    ry, fy, by = _table_state(y)
    assert fx == fy and bx == by and sorted(rx) == sorted(ry)
    keys = np.array(sorted(fx), np.int64)
    assert ops.kv_get_meta(x.handle, keys) == ops.kv_get_meta(y.handle, keys)
    gx, gy = _np(ops.kv_variable_gather_or_zeros_v2(x.handle, keys)), _np(ops.kv_variable_gather_or_zeros_v2(y.handle, keys))
    D = gx.shape[1] // (j + 1)
    zero = [np.zeros(D)] * 3
    extra = np.stack([tol.get(int(k), zero)[0] if j == 0 else np.concatenate(tol.get(int(k), zero)[1:]) for k in keys])
    bad = np.abs(gx.astype(np.float64) - gy) > 1e-6 * np.abs(gy) + 1e-9 + extra
    assert not bad.any(), (j, np.argwhere(bad)[:5], np.abs(gx - gy)[bad][:5], extra[bad][:5])


def test_adam_optimizer_fused_equals_the_composition(ops, tmp_path):
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import kv_variable_ops, variable_scope as vs
  vs.reset_default_store()
  kv_variable_ops.set_training(True)
  D = 16
  kvf = vs.get_kv_variable("adam_fused", embedding_dim=D, initializer=vs.ones_initializer)
  kvc = vs.get_kv_variable("adam_composed", embedding_dim=D, initializer=vs.ones_initializer)
  optf, optc = training.AdamOptimizer(0.01, fused=True), training.AdamOptimizer(0.01, fused=False)
  rng = np.random.default_rng(3)
  model = (A.Table(D, np.ones((1, D), F), 0, 0), A.Table(2 * D, np.zeros((1, 2 * D), F), 0, 0))
  tol = {}

  def step(t, pairs):
    ids = np.arange(40, dtype=np.int64) if t == 0 else rng.integers(0, 60, 200).astype(np.int64)      # repeated from step 2 on
    g = rng.normal(0, 0.1, (ids.size, D)).astype(F)
    for opt, kv in pairs:
      opt.apply_gradients([(kv_variable_ops.IndexedSlices(torch.from_numpy(g), torch.from_numpy(ids), None), kv)])
    return ids, g

  def widen(ids, g, hp):
    """A step with repeated ids: the fused op sums a key's gradient rows in tile order, the composition's dedup in its own.
    tests/_reorder.py's interval: every float32 order of the same addends stays within dg = (cnt - 1) 2^-24 sum|g| of the
    exact sum, so the two differ by at most 2 dg.  The bound is the largest change of (var, m', v') in float64 when the
    summed gradient moves by 2 dg and the moments the step starts from by the bounds they carry from earlier steps (all sign
    combinations); the var's adds up over the steps, the moments' replace the carried ones."""
    u, inv, cnt = np.unique(ids, return_inverse=True, return_counts=True)
    g64 = g.astype(np.float64)
    gsum = np.zeros((u.size, D)); np.add.at(gsum, inv, g64)
    gabs = np.zeros((u.size, D)); np.add.at(gabs, inv, np.abs(g64))
    dg = 2 * (cnt[:, None] - 1) * 2.0 ** -24 * gabs
    s0 = model[1].read(u).astype(np.float64)
    m0, v0 = s0[:, :D], s0[:, D:]
    zero = [np.zeros(D)] * 3
    tm, tv = (np.stack([tol.get(k, zero)[i] for k in u.tolist()]) for i in (1, 2))
    lr_t, omb1, omb2 = (float(v) for v in A.host_scalars(*hp[:5]))

    def f(gs, m, v):
      m1 = float(F(B1)) * m + gs * omb1
      v1 = float(F(B2)) * np.maximum(v, 0) + gs * gs * omb2
      return lr_t * m1 / (float(F(EPS)) + np.sqrt(v1)), m1, v1
    base = f(gsum, m0, v0)
    dev = [np.zeros((u.size, D)) for _ in range(3)]
    for sg in (1, -1):
      for sm in (1, -1):
        for sv in (1, -1):
          for d, a_, b_ in zip(dev, base, f(gsum + sg * dg, m0 + sm * tm, v0 + sv * tv)):
            np.maximum(d, np.abs(b_ - a_), out=d)
    for i, k in enumerate(u.tolist()):
      tol[k] = [tol.get(k, zero)[0] + dev[0][i], dev[1][i], dev[2][i]]

  for t in range(4):
    hp = (0.01, float(optf._beta1_power or F(B1)), float(optf._beta2_power or F(B2)), B1, B2, EPS)
    ids, g = step(t, [(optf, kvf), (optc, kvc)])
    if t > 0:
      widen(ids, g, hp)
    A.adam_step(model[0], model[1], ids, g, *hp)                    # carries the state the bound is evaluated at
    _assert_twins(ops, (kvf, optf.get_slot(kvf, "m_v")), (kvc, optc.get_slot(kvc, "m_v")), tol)
    if t == 1:
      # a checkpoint written under one setting continues under the other
      kvf.save(str(tmp_path / "var.npz")); optf.get_slot(kvf, "m_v").save(str(tmp_path / "m_v.npz"))
      kvr = vs.get_kv_variable("adam_restored", embedding_dim=D, initializer=vs.ones_initializer)
      optr = training.AdamOptimizer(0.01, fused=False)
      optr._create_slots([kvr])
      kvr.load(str(tmp_path / "var.npz")); optr.get_slot(kvr, "m_v").load(str(tmp_path / "m_v.npz"))
      optr._beta1_power, optr._beta2_power = optf._beta1_power, optf._beta2_power
      rng_state = rng.bit_generator.state
  assert optf.get_slot_names() == ["m_v"] and optf.get_slot(kvf, "m_v").embedding_dim == 2 * D
  # the restored, composed optimizer takes steps 3 and 4 on the same batches and ends where the two ended
  rng.bit_generator.state = rng_state
  for t in (2, 3):
    step(t, [(optr, kvr)])
  # (it started from the fused twin's state of step 2: the same bounds as between the twins)
  _assert_twins(ops, (kvr, optr.get_slot(kvr, "m_v")), (kvc, optc.get_slot(kvc, "m_v")), tol)


def test_captured_tok_step_replays(ops):
  dev = torch.device("cuda", 0)
  gen = torch.Generator(device=dev).manual_seed(3)
  D, n = 32, 4000
  ids = torch.randperm(8000, device=dev, generator=gen)[:n]
  grad = torch.randn(n, D, device=dev, generator=gen) * 1e-2
  hp = _hp(3)

  def pair():
    hs = [_table(ops, D, np.full((16, D), 0.01, F), cap=4 * n), _table(ops, 2 * D, np.zeros((16, 2 * D), F), cap=4 * n)]
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
