"""CPU checks of tests/_adam_ref.py, the definition the GPU tests of kv_apply_adam compare against: the restatement equals,
bit for bit, the reference's chain run on the oracle (gather_or_insert on the slot table, NumPy float32 arithmetic,
scatter_update, scatter_sub), rows and bookkeeping alike, and it agrees with the float64 closed form of TF Adam."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _adam_ref as A  # noqa: E402
import make_golden as G  # noqa: E402
from oracle import kv_oracle as ko  # noqa: E402

F = np.float32
DAY = 20000
SEED = 5
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-8


def _pows(t):
  return tuple(float(p) for p in G.beta_powers(B1, B2, t + 1))


def _tables(D, rng, thr=0):
  """Twin (var, m_v) pairs: the model and the oracle, same init tables, seed and day."""
  vinit = rng.uniform(-0.5, 0.5, (16, D)).astype(F)
  sinit = np.zeros((4, 2 * D), F)
  model = (A.Table(D, vinit, SEED, DAY, thr), A.Table(2 * D, sinit, SEED, DAY))
  orc = (ko.OracleKv(D, thr, vinit, day=DAY, picker=1, seed=SEED), ko.OracleKv(2 * D, 0, sinit, day=DAY, picker=1, seed=SEED))
  return model, orc


def _oracle_chain(ov, os_, ids, grad, lr, b1p, b2p, b1, b2, eps):
  """python/training/adam.py:93-163 on the oracle's tables."""
  D = ov.dim
  u, g, _ = ko.dedup_segment_sum(ids, grad)                 # TF-core: first-occurrence order, occurrence-order sums
  mv = os_.gather_or_insert(u)
  lr_t, omb1, omb2 = A.host_scalars(lr, b1p, b2p, b1, b2)
  m = F(b1) * mv[:, :D] + g * omb1
  v = F(b2) * mv[:, D:] + (g * g) * omb2
  os_.scatter_update(u, np.concatenate([m, v], axis=1), op=0)
  ov.scatter_update(u, (lr_t * m) / (F(eps) + np.sqrt(v)), op=2)


def _same(model, orc, universe):
  """Rows, frequency words, flags, blacklists and key sets of both tables."""
  for t, o in zip(model, orc):
    assert [o.meta(int(k)) for k in universe] == t.metas(universe)
    assert o.map_size() == len(t.rows)
    got, want = o.gather_or_zeros(universe), t.read(universe)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("repeated", [False, True])
@pytest.mark.parametrize("D", [1, 4, 5, 32])
def test_restatement_equals_the_chain_on_the_oracle(D, repeated):
  rng = np.random.default_rng(100 + D + repeated)
  model, orc = _tables(D, rng)
  universe = np.arange(-40, 260, dtype=np.int64)
  for t in range(3):                                        # three steps with advancing powers; new keys arrive in each
    if repeated:
      ids = rng.integers(-30, 80 + 60 * t, 400).astype(np.int64)
    else:
      ids = rng.choice(np.arange(-30, 100 + 60 * t), 90, replace=False).astype(np.int64)
    grad = (rng.normal(0, 1, (ids.size, D)) * rng.choice([1e-1, 1e-3], (ids.size, 1))).astype(F)
    seen = np.unique(ids)[::2]                              # half the keys come from a lookup, the rest the step inserts
    model[0].lookup(seen); orc[0].gather_or_insert(seen)
    hp = (LR,) + _pows(t) + (B1, B2, EPS)
    u = A.adam_step(model[0], model[1], ids, grad, *hp)
    _oracle_chain(orc[0], orc[1], ids, grad, *hp)
    assert sorted(u) == sorted(np.unique(ids))
    _same(model, orc, universe)
  ms = model[1].metas(universe)
  assert any(m and m["freq"] == 3 for m in ms) and all(m is None or m["day"] == DAY for m in ms)


def test_keys_below_the_enter_threshold_are_updated():
  rng = np.random.default_rng(7)
  D = 4
  model, orc = _tables(D, rng, thr=3)
  ids = np.arange(20, dtype=np.int64)
  model[0].lookup(ids); orc[0].gather_or_insert(ids)        # frequency 1 < 3
  before = model[0].read(ids)
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  hp = (LR,) + _pows(0) + (B1, B2, EPS)
  A.adam_step(model[0], model[1], ids, grad, *hp)
  _oracle_chain(orc[0], orc[1], ids, grad, *hp)
  _same(model, orc, ids)
  assert (model[0].read(ids) != before).all()
  assert [m["freq"] for m in model[0].metas(ids)] == [1] * ids.size          # ... and the var's frequency word is untouched


def test_blacklisted_var_key_stays_untouched_and_blacklisted():
  rng = np.random.default_rng(8)
  D = 4
  model, orc = _tables(D, rng)
  ids = np.arange(10, dtype=np.int64)
  model[0].lookup(ids)
  vals = model[0].read(ids)
  orc[0].gather_or_insert(ids)
  fk = ids
  fv = np.full(ids.size, (DAY << 16) | 1, np.uint32)
  orc[0].import_(ids, vals, blacklist=[3], freq_keys=fk, freq_values=fv)      # the oracle's way to a blacklisted key
  model[0].blacklist(3)
  assert orc[0].meta(3) == model[0].rows[3].meta()
  for t in range(2):
    grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
    hp = (LR,) + _pows(t) + (B1, B2, EPS)
    A.adam_step(model[0], model[1], ids, grad, *hp)
    _oracle_chain(orc[0], orc[1], ids, grad, *hp)
    _same(model, orc, ids)
  m3 = model[0].rows[3].meta()
  assert m3["blacklist"] and m3["under_threshold"] and not model[0].read([3]).any()
  assert model[1].rows[3].meta()["freq"] == 2 and model[1].read([3]).any()   # its moments are kept all the same


def test_key_missing_from_the_var_is_inserted_then_updated():
  rng = np.random.default_rng(9)
  D = 5
  model, orc = _tables(D, rng)
  ids = np.array([11, -4, 11, 9], np.int64)
  grad = rng.normal(0, 0.1, (ids.size, D)).astype(F)
  hp = (LR,) + _pows(0) + (B1, B2, EPS)
  A.adam_step(model[0], model[1], ids, grad, *hp)
  _oracle_chain(orc[0], orc[1], ids, grad, *hp)
  _same(model, orc, np.array([11, -4, 9, 0], np.int64))
  for k in (11, -4, 9):
    assert model[0].rows[k].meta() == {"freq": 1, "day": 0, "blacklist": False, "under_threshold": False}
    assert model[1].rows[k].meta()["freq"] == 1 and model[1].rows[k].meta()["day"] == DAY
    assert (model[0].rows[k].row != model[0].init_row(k)).all()


def test_two_steps_agree_with_the_closed_form_of_tf_adam():
  """tests/golden/make_golden.py tf_adam_step in float64; the tolerance of
  tests/test_gpu_python_api.py::test_adam_optimizer_equals_tf_adam (rtol 1e-5, atol 1e-8)."""
  rng = np.random.default_rng(10)
  D, n = 8, 12
  var = A.Table(D, np.ones((2, D), F), SEED, DAY)
  slot = A.Table(2 * D, np.zeros((2, 2 * D), F), SEED, DAY)
  ids = np.arange(n, dtype=np.int64)
  x, m, v = np.ones((n, D)), 0.0, 0.0
  for t in (1, 2):
    g = rng.random((n, D)).astype(F)
    b1p, b2p = G.beta_powers(B1, B2, t)
    A.adam_step(var, slot, ids, g, 0.1, b1p, b2p, B1, B2, EPS)
    x, m, v = G.tf_adam_step(x, m, v, g.astype(np.float64), 0.1, B1, B2, EPS, t)
    np.testing.assert_allclose(var.read(ids), x, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(slot.read(ids), np.concatenate([m, v], axis=1), rtol=1e-5, atol=1e-8)
