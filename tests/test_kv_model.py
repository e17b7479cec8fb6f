"""CPU checks of tests/_kv_model.py, before it judges a kernel (tests/test_gpu_fuzz_optimizers.py): random programs of the
table ops on the model and on the oracle side by side — key sets, records, sizes and sums equal, rows bit for bit after
every op, blacklisted keys included; the optimizer steps where the oracle can follow (plain Adam as the reference's chain,
FTRL-V2 without l1 as SparseGroupFtrl without l1 and l21); for every seed the GPU test runs, the program generator's own
conditions, from the model alone; and the allowance the lasso programs carry, against float64 evaluations of their steps."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _adam_ref as A  # noqa: E402
import _ftrl_ref as RF  # noqa: E402
import _kv_model as M  # noqa: E402
import _radam_ref as RR  # noqa: E402
from oracle import kv_oracle as ko  # noqa: E402

F = np.float32
DAY = 20000


def _bits(a, b):
  return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _twin(D, thr, table, seed):
  return M.Table(D, table, seed, DAY, thr), ko.OracleKv(D, thr, table, day=DAY, picker=1, seed=seed)


def _same(m, o, universe, tag, rows=True):
  assert [o.meta(int(k)) for k in universe] == m.metas(universe), tag
  assert (o.map_size(), o.size(), o.sum_freq()) == (m.map_size(), m.size(), m.sum_freq()), tag
  assert np.array_equal(o.get_count(universe), m.get_count(universe)), tag
  assert np.array_equal(o.get_timestamp(universe), m.get_timestamp(universe)), tag
  if rows:
    got, want = m.gather_or_zeros(universe), o.gather_or_zeros(universe)
    assert _bits(got, want), (tag, np.argwhere(got != want)[:5])


def _import_blacklist(m, o, black):
  """The oracle's way to a blacklisted key: the table re-imported with `black` on the blacklist (ImportValues leaves
  under_threshold unset on the rows it loads); the model follows with blacklist()."""
  keys = np.array(sorted(m.rows), np.int64)
  black = sorted(set(black) | {k for k, r in m.rows.items() if r.black})
  fw = np.array([m.rows[int(k)].freq for k in keys], np.uint32)
  o.import_(keys, m.read(keys), blacklist=black, freq_keys=keys, freq_values=fw)
  for k in keys.tolist():
    if k in black:
      m.blacklist(k)
    else:
      m.rows[k].under = False


# ---- 1. the table ops ----------------------------------------------------------------------------------------------------
TABLE_OPS = ["lookup", "lookup_counts", "zeros", "scatter", "insert", "delete", "expire", "day", "blacklist"]


@pytest.mark.parametrize("seed", range(8))
def test_table_ops_equal_the_oracle(seed):
  rng = np.random.default_rng(500 + seed)
  D = int(rng.choice([1, 5, 8]))
  thr = int(rng.choice([0, 2, 3]))
  ks = int(rng.choice([12, 60]))
  universe = np.arange(-ks - 3, ks + 3, dtype=np.int64)
  m, o = _twin(D, thr, rng.standard_normal((8, D)).astype(F) * F(rng.choice([1.0, 1e-21])), seed)   # (1e-21: rows under the cutoff)
  day = DAY
  seen = set()
  for step in range(60):
    op = str(rng.choice(TABLE_OPS, p=[.2, .1, .1, .15, .1, .1, .1, .05, .1]))
    seen.add(op)
    n = int(rng.choice([1, 5, 40]))
    ids = rng.integers(-ks, ks, n).astype(np.int64)
    tag = "seed %d step %d %s" % (seed, step, op)
    if op == "lookup":
      assert _bits(m.gather_or_insert(ids), o.gather_or_insert(ids)), tag
    elif op == "lookup_counts":
      c = rng.choice([1, 3, 30000, 65535, 70000], n).astype(np.int32)           # saturating, and saturated on the way in
      assert _bits(m.gather_or_insert(ids, c), o.gather_or_insert(ids, c)), tag
    elif op == "zeros":
      assert _bits(m.gather_or_zeros(ids), o.gather_or_zeros(ids)), tag
    elif op == "scatter":
      u = np.unique(ids)
      upd = rng.uniform(0.5, 2.0, (u.size, D)).astype(F) * F(rng.choice([1.0, -1.0, 0.0], p=[.7, .2, .1]))
      which = int(rng.integers(0, 7))
      m.scatter_update(u, upd, which); o.scatter_update(u, upd, which)
    elif op == "insert":
      u = np.unique(ids)
      vals = rng.standard_normal((u.size, D)).astype(F) * F(rng.choice([1.0, 0.0], p=[.8, .2]))
      m.insert(u, vals); o.insert(u, vals)
    elif op == "delete":
      assert m.delete(ids) == o.delete(ids), tag
    elif op == "expire":
      t = int(rng.integers(1, 4))
      assert m.delete_with_timestamp(t) == sorted(o.delete_with_timestamp(t).tolist()), tag
    elif op == "day":
      day += int(rng.integers(1, 3))
      m.set_day(day); o.set_day(day)
    elif m.rows:
      _import_blacklist(m, o, rng.choice(sorted(m.rows), min(3, len(m.rows)), replace=False).tolist())
    _same(m, o, universe, tag)
  assert len(seen) >= 7


# ---- 2. the optimizer steps where the oracle can follow ------------------------------------------------------------------
def _oracle_adam_chain(ov, os_, u, g, lr, b1p, b2p, b1, b2, eps):
  """python/training/adam.py:93-163 on the oracle's tables (tests/test_adam_ref.py _oracle_chain), on unique ids."""
  D = ov.dim
  mv = os_.gather_or_insert(u)
  lr_t, omb1, omb2 = A.host_scalars(lr, b1p, b2p, b1, b2)
  mm = F(b1) * mv[:, :D] + g * omb1
  v = F(b2) * mv[:, D:] + (g * g) * omb2
  os_.scatter_update(u, np.concatenate([mm, v], axis=1), op=0)
  ov.scatter_update(u, (lr_t * mm) / (F(eps) + np.sqrt(v)), op=2)


def _table_traffic(rng, step, tabs, ks):
  """What a program does between applies, on [(model, oracle), ...] of one var and its slot tables: lookups, and deletes
  that fall on a random subset of the tables."""
  ids = rng.integers(-ks, ks, int(rng.choice([3, 30]))).astype(np.int64)
  if step % 3 == 0:
    c = rng.integers(1, 4, ids.size).astype(np.int32)
    assert _bits(tabs[0][0].gather_or_insert(ids, c), tabs[0][1].gather_or_insert(ids, c))
  if step % 3 == 1:
    mask = int(rng.integers(1, 1 << len(tabs)))
    for j, (m, o) in enumerate(tabs):
      if mask >> j & 1:
        assert m.delete(ids[:8]) == o.delete(ids[:8])


@pytest.mark.parametrize("seed", range(4))
def test_adam_steps_equal_the_chain_on_the_oracle(seed):
  rng = np.random.default_rng(600 + seed)
  D, ks = int(rng.choice([1, 4, 5])), 50
  thr = int(rng.choice([0, 3]))
  universe = np.arange(-ks - 2, ks + 2, dtype=np.int64)
  tabs = [_twin(D, thr, rng.uniform(-0.5, 0.5, (16, D)).astype(F), seed), _twin(2 * D, 0, np.zeros((4, 2 * D), F), seed)]
  b1p, b2p = F(0.9), F(0.999)
  for step in range(12):
    _table_traffic(rng, step, tabs, ks)
    if step == 5:
      for m, o in tabs:
        _import_blacklist(m, o, rng.choice(sorted(m.rows), 3, replace=False).tolist())
    ids = rng.integers(-ks, ks, 60).astype(np.int64)
    u, s = M.dedup_sum(ids, (rng.normal(0, 1, (60, D)) * rng.choice([1e-1, 1e-3], (60, 1))).astype(F))
    ou, os_, _ = ko.dedup_segment_sum(ids, np.zeros((60, D), F))
    assert np.array_equal(u, ou)
    hp = (0.05, float(b1p), float(b2p), 0.9, 0.999, 1e-8)
    res = M.apply_step("adam", tabs[0][0], [tabs[1][0]], u, s, hp)
    assert res["keys"] == u.tolist() and not res["filtered"]              # the chain has no filter
    _oracle_adam_chain(tabs[0][1], tabs[1][1], u, s, *hp)
    b1p, b2p = F(b1p * F(0.9)), F(b2p * F(0.999))
    for m, o in tabs:
      _same(m, o, universe, "seed %d step %d" % (seed, step))


def test_dedup_sum_equals_the_oracle():
  rng = np.random.default_rng(3)
  ids = rng.integers(-20, 20, 500).astype(np.int64)
  g = rng.normal(0, 1, (500, 6)).astype(F)
  u, s = M.dedup_sum(ids, g)
  ou, os_, _ = ko.dedup_segment_sum(ids, g)
  assert np.array_equal(u, ou) and _bits(s, os_)


# tests/test_ftrl_v2.py's bars between the restatement and the recorded reference step (A4): var, accum, linear
FTRL_BARS = [dict(rtol=1e-5, atol=1e-8), dict(rtol=1e-6), dict(rtol=1e-5, atol=1e-6)]


@pytest.mark.parametrize("family", ["ftrl_v2", "group_ftrl_v2"])
@pytest.mark.parametrize("seed", range(3))
def test_ftrl_v2_without_l1_equals_sparse_group_ftrl(family, seed):
  """With l1 = l21 = 0 and every linear row non-zero SparseGroupFtrl's update is FTRL-V2's (tests/test_gpu_ftrl_v2.py
  test_equals_sparse_group_ftrl_without_l1): rows at tests/test_ftrl_v2.py's bars, every step from the oracle's own state
  of the step before; frequency words, days, blacklists, key sets, sizes and sums exactly.  Group FTRL-V2 adds the squared
  gradient to accum twice, so its rows are not SparseGroupFtrl's, but its bookkeeping is, under_threshold included (both
  recompute it from the rows they write, and no row here is near the cutoff): every record exactly."""
  rng = np.random.default_rng(700 + seed)
  D, ks = int(rng.choice([1, 5, 8])), 60
  thr = [0, 2, 2][seed]
  universe = np.arange(-ks - 2, ks + 2, dtype=np.int64)
  tabs = [_twin(D, thr, rng.standard_normal((16, D)).astype(F) * F(0.05), seed), _twin(D, 0, np.full((4, D), 0.1, F), seed),
          _twin(D, 0, np.zeros((4, D), F), seed)]
  hp = (0.1, 0.0, 1e-2, 1e-2, -0.5)
  filtered = 0
  for step in range(10):
    _table_traffic(rng, step, tabs, ks)
    ids = rng.integers(-ks, ks, 80).astype(np.int64)
    u, s = M.dedup_sum(ids, rng.normal(0, 0.1, (80, D)).astype(F))
    res = M.apply_step(family, tabs[0][0], [tabs[1][0], tabs[2][0]], u, s, hp)
    filtered += len(res["filtered"])
    assert res["updated"] is None or all(res["updated"])
    ko.apply_sparse_group_ftrl(tabs[0][1], tabs[1][1], tabs[2][1], s, u, 0.1, 0.0, 1e-2, 0.0, 1e-2, -0.5)
    for (m, o), bar in zip(tabs, FTRL_BARS):
      tag = "%s seed %d step %d" % (family, seed, step)
      if family == "group_ftrl_v2":
        _same(m, o, universe, tag, rows=False)
      else:
        want = [o.meta(int(k)) for k in universe]
        got = m.metas(universe)
        strip = lambda ms: [None if x is None else (x["freq"], x["day"], x["blacklist"]) for x in ms]
        assert strip(got) == strip(want), tag
        assert (o.map_size(), o.size(), o.sum_freq()) == (m.map_size(), m.size(), m.sum_freq()), tag
        np.testing.assert_allclose(m.gather_or_zeros(universe), o.gather_or_zeros(universe), err_msg=tag, **bar)
      for k, r in m.rows.items():                            # the next step starts from the oracle's rows, bit for bit
        r.row = o.gather_or_zeros(np.array([k]))[0].copy()
  assert thr == 0 or filtered > 0


def test_group_steps_blacklist_lift_and_filter():
  """The rules the oracle's ops share with the group ops, on a hand-made case: a filtered key is untouched and gets no slot
  rows; a key the apply inserts is not filtered; the norm under the threshold blacklists, the next pass lifts."""
  D = 4
  var = M.Table(D, np.full((2, D), 0.01, F), 1, DAY, 2)
  slots = [M.Table(D, np.full((2, D), 0.1, F), 1, DAY), M.Table(D, np.zeros((2, D), F), 1, DAY)]
  var.gather_or_insert([1, 2, 2])                            # key 1: frequency 1 < 2; key 2 passes
  hp = (0.1, 0.5, 0.0, 0.0, -0.5)
  res = M.apply_step("group_ftrl_v2", var, slots, [1, 2, 3], np.full((3, D), 1e-3, F), hp)
  assert res["filtered"] == [1] and res["keys"] == [2, 3] and list(res["updated"]) == [False, False]
  assert slots[0].meta(1) is None and slots[1].meta(1) is None and var.meta(1)["freq"] == 1
  assert var.meta(3) == {"freq": 1, "day": 0, "blacklist": True, "under_threshold": True}
  assert slots[0].meta(2) == {"freq": 1, "day": 0, "blacklist": False, "under_threshold": False}
  assert not var.gather_or_zeros([2, 3]).any() and var.size() == 0
  res = M.apply_step("group_ftrl_v2", var, slots, [2, 3], np.full((2, D), 5.0, F), hp)
  assert res["lifted"] == [2] and res["filtered"] == [3] and list(res["updated"]) == [True]      # key 3 now has frequency 1 < 2
  assert var.meta(2)["blacklist"] is False and var.meta(2)["under_threshold"] is False and var.gather_or_zeros([2]).all()
  assert slots[0].meta(2) == {"freq": 2, "day": DAY, "blacklist": False, "under_threshold": False}


# ---- 3. the program generator: the conditions, for the seeds the GPU test runs -------------------------------------------
def _run(family, seed, occ):
  p = M.Program(family, seed, occ)
  kinds = [s["op"] for s in p.steps()]
  assert len(kinds) == M.Program.STEPS
  return p


def test_programs_are_deterministic_in_the_seed():
  a, b = M.Program("group_radam", 1, False), M.Program("group_radam", 1, False)
  for x, y in zip(a.steps(), b.steps()):
    assert x["op"] == y["op"] and all(np.array_equal(i, j) for i, j in zip(x["check"], y["check"]))
  for ta, tb in zip(a.sets[0].tables, b.sets[0].tables):
    assert sorted(ta.rows) == sorted(tb.rows) and _bits(ta.read(a.universe), tb.read(b.universe))


@pytest.mark.parametrize("family", M.FAMILIES)
def test_generator_conditions(family):
  progs = [_run(family, seed, occ) for occ in (False, True) for seed in M.SEEDS[family]]
  assert len(M.SEEDS[family]) >= 6
  st = [p.stats for p in progs]
  assert set().union(*(s["ops"] for s in st)) == set(M.OPS)
  assert set().union(*(s["forms"] for s in st)) == set(M.FORMS)
  assert {p.D for p in progs} & {5, 6} and any(p.int32 for p in progs) and any(p.thr == 2 for p in progs)
  assert sum(s["orphan_apply"] for s in st) > 0                        # an apply met a key whose slot row alone was deleted
  assert sum(s["filtered_apply"] for s in st) > 0
  for p in progs:                                                      # every program, not only their union
    s = p.stats
    assert s["applies"] > 0
    assert s["max_acc"] <= 1e-3 and s["max_rel"] <= 1e-3, (p.seed, p.occ, s["max_acc"], s["max_rel"])     # what the GPU test allows
    if p.lasso:
      assert s["worst_margin"] >= M.MARGIN, (p.seed, p.occ, s["worst_margin"])
    if p.exact:
      assert s["max_acc"] == 0.0 and s["max_rel"] == 0.0
  if family in ("group_ftrl_v2", "group_radam"):
    assert any(p.lasso for p in progs) and any(not p.lasso for p in progs)
    assert sum(s["lasso_steps"] for s in st) > 0 and set().union(*(s["branches"] for s in st)) == {True, False}
    for what in ("blacklisted", "black_lookup", "black_delete", "black_expire", "black_lift"):
      assert sum(s[what] for s in st) > 0, what
  if family == "group_radam":
    assert {p.branch for p in progs} == set(M.RADAM_BRANCHES) and {p.nesterov for p in progs} == {False, True}
    assert any(not p.lasso and p.stats["blacklisted"] for p in progs)     # the exact programs blacklist too (norm 0)


# ---- 4. the allowance against float64 ----------------------------------------------------------------------------------------
def _f64_step(family, x, srows, g, hp):
  if family == "group_ftrl_v2":
    return RF.group_ftrl_v2(x, srows[0], srows[1], g, *hp, dtype=np.float64)
  x1, s1, upd = RR.group_radam(x, srows[0], g, *hp, dtype=np.float64)
  return x1, s1, upd


@pytest.mark.parametrize("family", ["group_ftrl_v2", "group_radam"])
def test_allowance_holds_against_float64(family):
  """The error algebra of tests/_kv_model.py step_allowance, on every group step of every program that carries an
  allowance: the step in float64 at inputs moved by their allowances (all up, all down, random signs) against the step in
  float64 at the inputs themselves.  No output may move further than its allowance (which holds the var's bar and the
  rounding terms on top: moved inputs alone must fit), no decision may change, and the allowance is not idle: somewhere an
  output moves by more than half of it.  Float64 on both sides keeps the float32 model's own rounding out of the
  comparison: kernel and model round alike from equal inputs, which is what the exact programs assert bit for bit."""
  rng = np.random.default_rng(11)
  worst = [0.0]

  def on_allow(fam, hp, a):
    D = a["x"].shape[1]
    base = _f64_step(fam, a["x"], a["srows"], a["g"], hp)
    upd = a["upd"]
    assert np.array_equal(base[-1], upd)
    for sign in ("up", "down", "random"):
      mv = [t * (1.0 if sign == "up" else -1.0 if sign == "down" else rng.choice([-1.0, 1.0], t.shape)) for t in a["tin"]]
      ins = [a["x"].astype(np.float64) + mv[0]] + [s.astype(np.float64) + m for s, m in zip(a["srows"], mv[1:])]
      out = _f64_step(fam, ins[0], ins[1:], a["g"], hp)
      assert np.array_equal(out[-1], upd)                     # no decision within reach of an allowance
      for j, tout in enumerate(a["tout"]):
        err, tol = np.abs(out[j] - base[j]), tout
        if j == 0:
          err, tol = err[upd], tol[upd]
        ok = err <= tol * (1 + 1e-6)                          # (first order: the margin is for the second)
        assert ok.all(), (fam, sign, j, float((err[~ok] / tol[~ok]).max()))
        has = tol > 0
        if has.any():
          worst[0] = max(worst[0], float((err[has] / tol[has]).max()))

  n = 0
  for occ in (False, True):
    for seed in M.SEEDS[family]:
      p = M.Program(family, seed, occ, on_allow=on_allow)
      if not p.exact:
        n += sum(1 for _ in p.steps())
  print("%s: worst moved / allowed %.3g" % (family, worst[0]))
  assert n > 0 and 0.5 <= worst[0] <= 1.0 + 1e-6
