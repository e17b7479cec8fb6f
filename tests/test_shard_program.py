"""The premise of tests/test_gpu_fuzz_sharded.py, held on the host for exactly the seeds it runs: every program of
tests/_shard_program.py runs on ShardedModel (one model per owner, fed per sending rank that rank's distinct ids as
(id, count) records) next to the unsharded model the program carries, and after every step the union of the owners' tables is
the unsharded table — keys, rows bit for bit, frequency words, flags, sizes.  Then the generator's conditions: the exactness
bound of the gradient sums and the lossy no-overflow bound (asserted inside the generator, every step), and that every step
kind, driver, world and owner rule, a late capacity raise, a raise on one table of a multi call, a touch whose rank owns keys
of the batch, a blacklisted key looked up and a key filtered by the enter threshold all occur across the seeds."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _shard_program as SP  # noqa: E402

CASES = [(f, s) for f in SP.FAMILIES for s in SP.SEEDS[f]]


def _same_table(p, parts, whole, i, keys, tag):
  """the union of the owners' tables i is the unsharded one: key sets, sizes, and the state on `keys` (None: every key)"""
  want_keys = whole.tables[i].keys()
  got_keys = []
  for o, part in enumerate(parts):
    k = part.tables[i].keys()
    assert not k or np.all(p.owner(k) == o), (tag, o)          # an owner holds its own keys only
    got_keys += k
  assert sorted(got_keys) == want_keys, tag
  for fig in ("map_size", "size", "sum_freq"):
    assert sum(getattr(part.tables[i], fig)() for part in parts) == getattr(whole.tables[i], fig)(), (tag, fig)
  keys = np.array(want_keys if keys is None else keys, np.int64)
  own = p.owner(keys) if keys.size else keys
  for o, part in enumerate(parts):
    mine = keys[own == o]
    _, rows, metas = SP.table_state(part.tables[i], mine)
    _, wrows, wmetas = SP.table_state(whole.tables[i], mine)
    assert np.array_equal(rows.view(np.uint32), wrows.view(np.uint32)), (tag, o)
    assert metas == wmetas, (tag, o, [(int(k), g, w) for k, g, w in zip(mine, metas, wmetas) if g != w][:5])
    if mine.size:
      assert np.array_equal(part.tables[i].get_timestamp(mine), whole.tables[i].get_timestamp(mine)), (tag, o)


def _side_by_side(p, sm):
  """p's steps on ShardedModel sm next to the unsharded model p carries, compared after every step"""
  for st in p.steps():
    tag = "%s seed %d step %d %s" % (p.family, p.seed, st["step"], st["kind"])
    got = sm.take(st)
    if st["kind"] in ("expire", "delete"):                        # the union of the keys the owners removed / their numbers
      assert got == [a["gone"] for a in st["sets"]], tag
    full = st["step"] == p.STEPS - 1 or p.keyspace <= 400
    for j in range(2):
      for i in range(len(p.sets[j].tables)):
        _same_table(p, sm.sets[j], p.sets[j], i, None if full else st["check"][j], "%s set %d table %d" % (tag, j, i))


@functools.lru_cache(maxsize=None)
def _program(family, seed):
  """one program, run once side by side; its statistics are kept for the conditions"""
  p = SP.ShardProgram(family, seed)
  _side_by_side(p, SP.ShardedModel(p))
  return p


@pytest.mark.parametrize("family,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_the_owners_tables_are_the_unsharded_table(family, seed):
  p = _program(family, seed)
  assert p.stats["applies"] > 0 and p.stats["max_abs_sum"] < 2 ** 24
  assert all(ts.var.map_size() > 0 for ts in p.sets)


def test_counts_saturate_alike_across_the_ranks_records():
  """The programs' counts stay far below 65535, so saturation is seeded: every key of the universe starts at 65500 on the
  unsharded model and on its owner, and the program's lookups then push the hot keys over the top — one occurrence after the
  other on the unsharded table, as one (id, count) record per sending rank on the owners."""
  p = SP.ShardProgram("adam", 10)                                 # keyspace 50, world 2: about 25 occurrences per key, rank and lookup
  assert p.keyspace == 50 and p.world > 1
  sm = SP.ShardedModel(p)
  for j, ts in enumerate(p.sets):
    counts = np.full(p.universe.size, 65500, np.int32)
    ts.var.gather_or_insert(p.universe, counts)
    for o, part in enumerate(sm.sets[j]):
      part.var.gather_or_insert(p.owned(o), counts[:p.owned(o).size])
  _side_by_side(p, sm)
  for j, ts in enumerate(p.sets):
    held = np.array(ts.var.keys(), np.int64)
    c = ts.var.get_count(held)
    assert np.sum(c == 65535) >= 3 and np.sum(c < 65535) >= 1, (j, int(np.sum(c == 65535)))


@pytest.mark.parametrize("own", [None, "part"])
def test_the_host_tables_round_trip_is_the_oracles(own):
  """HostTable.roundtrip (the exact families' model of export -> import) against OracleKv.export / import_ /
  import_delta on a table with blacklisted, under-threshold and low-frequency keys, whole and for one owner's keys; and the
  lookup behind it, which evaluates the flags the import left alone."""
  from oracle import kv_oracle as ko
  D, thr, rng = 8, 2, np.random.default_rng(9)
  init = rng.standard_normal((16, D)).astype(np.float32)
  h = SP.HostTable(D, init, 5, SP.DAY0, thr)
  o = SP.OracleTable(D, init, 5, SP.DAY0, thr)
  slot = ko.OracleKv(3 * D, 0, np.zeros((4, 3 * D), np.float32), day=SP.DAY0, picker=1, seed=5)
  keys = np.arange(0, 60, dtype=np.int64)
  counts = np.where(keys % 5 == 0, 1, 3).astype(np.int32)         # every fifth key stays under the enter threshold
  zero = keys[(keys % 7 == 1) & (keys % 5 != 0)]                  # rows of zeros: under_threshold set by the insert
  black = keys[(keys % 4 == 2) & (keys % 5 != 0)]
  for t in (h, o):
    t.gather_or_insert(keys, counts)
    t.insert(zero, np.zeros((zero.size, D), np.float32))
  ko.apply_group_adam(o.o, slot, np.ones((black.size, D), np.float32), black, 0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 1e6)
  for k in black:
    h.blacklist(k)

  def same(tag):
    hk, hr, hm = SP.table_state(h)
    ok, orow, om = SP.table_state(o)
    assert hk == ok, tag
    assert np.array_equal(hr.view(np.uint32), orow.view(np.uint32)) and hm == om, (tag, [(k, a, b) for k, a, b in zip(hk, hm, om) if a != b][:5])
    assert (h.map_size(), h.size(), h.sum_freq()) == (o.map_size(), o.size(), o.sum_freq()), tag
  same("before")
  st = {m["blacklist"] for m in h.metas(black)}, {m["under_threshold"] for m in h.metas(zero)}
  assert st == ({True}, {True}) and min(h.get_count(keys)) < thr
  mine = None if own is None else set(keys[keys % 3 == 1].tolist())
  h.roundtrip(mine)
  o.roundtrip(mine)
  same("after the round trip")
  assert h.map_size() < keys.size                                  # the low-frequency and under-threshold keys were not exported
  for t in (h, o):
    t.gather_or_insert(keys)
  same("after the next lookup")


def test_generator_conditions():
  ps = [_program(f, s) for f, s in CASES]
  assert len(ps) >= 16 and all(len(SP.SEEDS[f]) >= 4 for f in SP.FAMILIES)
  kinds = set().union(*[p.stats["kinds"] for p in ps])
  assert kinds == set(SP.KINDS), set(SP.KINDS) - kinds
  drivers = set().union(*[p.stats["drivers"] for p in ps])
  for kind in SP.LOOKS + ("eval",):                               # every lookup kind under every driver
    for d in SP.DRIVERS:
      assert (kind, d) in drivers, (kind, d)
  assert {p.world for p in ps} == {1, 2, 3, 4} and {p.rule for p in ps} == {"hash", "mod"}
  assert {p.same_dim for p in ps} == {True, False} and {p.det for p in ps} == {True, False}
  assert {p.lossless for p in ps} == {True, False} and {p.thr for p in ps} == {0, 2}
  forms = set().union(*[p.stats["forms"] for p in ps])
  assert {"plain", "zeros"} <= forms
  for kind in ("sparse", "sparse_zeros"):
    assert {c for f in forms if isinstance(f, tuple) and f[0] == kind for c in [f[1]]} == {"sum", "mean", "sqrtn"}, kind
    assert {f[2] for f in forms if isinstance(f, tuple) and f[0] == kind} == {True, False}, kind
  raises = [r for p in ps for r in p.stats["raises"]]
  assert any(step >= 5 for step, _, _, _ in raises), raises       # a capacity raise after applies, not on a first lookup
  assert any(not train for _, _, _, train in raises)              # ... and one by a read-only lookup
  assert sum(p.stats["multi_one_raise"] for p in ps) > 0          # one table of a multi call grows, the other keeps its buffers
  assert sum(p.stats["touch_owned"] for p in ps) > 0
  assert sum(p.stats["black_lookup"] for p in ps) > 0
  assert sum(p.stats["filtered_apply"] for p in ps) > 0
  assert sum(p.stats["single_owner"] for p in ps) > 0
  for p in ps:                                                    # lossy programs cannot overflow (asserted per lookup too)
    assert p.lossless or p.stats["max_need"] <= p.cap0


def test_programs_are_deterministic():
  a, b = SP.ShardProgram("adam", 1), SP.ShardProgram("adam", 1)
  for x, y in zip(a.steps(), b.steps()):
    assert x["kind"] == y["kind"] and x["driver"] == y["driver"]
    for lx, ly in zip((x["lookup"] or x["read"] or {"sets": []})["sets"], (y["lookup"] or y["read"] or {"sets": []})["sets"]):
      assert all(np.array_equal(i, j) for i, j in zip(lx["ids"], ly["ids"]))
      assert all(np.array_equal(i.view(np.uint32), j.view(np.uint32)) for i, j in zip(lx["rows"], ly["rows"]))
