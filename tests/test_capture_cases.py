"""tests/_capture_cases.py on the CPU: the batches are disjoint, the new-key counts the rules give are the ones the references
count, every trajectory meets its conditions by the reference alone (both branches of every group step, no row near its
threshold, FTRL-V2's l1 zeroes some elements and not all), the prepared room covers what it must, and the inequalities of
the two bounds cases hold for the growth chunk the sources state."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _capture_cases as C  # noqa: E402
import _kv_model as M  # noqa: E402
import _row_geometry as G  # noqa: E402


def test_batches_are_disjoint_and_reach_every_branch():
  rb = C.replay_batches(C.SEEDS)
  batches = rb["batches"]
  assert len(batches) == C.TABLES * (C.R + 1) and rb["n"] == 2172 > G.TILE
  keys = np.concatenate([b["keys"] for b in batches])
  assert np.unique(keys).size == keys.size == 144 * len(batches)                # pairwise disjoint
  early = C.early_victims()
  assert np.intersect1d(early, keys).size == 0 and np.unique(early).size == early.size
  for b in batches:
    c = b["counts"]
    assert b["ids"].size == rb["n"] and set(np.unique(b["pre"]).tolist()) == set(b["keys"][::2].tolist())
    assert np.intersect1d(b["new"], b["pre"]).size == 0 and b["new"].size + np.unique(b["pre"]).size == b["keys"].size
    # cold keys of one and of several occurrences, the last cold count, hot keys of one chunk and of several, both tiles
    assert (c == 1).any() and (c == G.LCOLD).any() and (c == G.LCOLD + 1).any() and (c == G.HC).any() and (c > G.HC).any()
    at = np.flatnonzero(b["ids"] == b["span"])
    assert at[0] < G.TILE <= at[-1]
    # present keys at and above the threshold, present keys below it, new keys of one occurrence (below it behind the lookup)
    pre = dict(zip(*[a.tolist() for a in np.unique(b["pre"], return_counts=True)]))
    assert set(pre.values()) == {1, 2} and G.ENTER == 2
    occ = dict(zip(b["keys"].tolist(), c.tolist()))
    assert any(occ[int(k)] == 1 for k in b["new"]) and any(occ[int(k)] > 1 for k in b["new"])
  # a second call returns the same objects (the GPU module and this one see the same batches)
  assert C.replay_batches(C.SEEDS) is rb


def test_the_pipelines_of_the_dims():
  # (scalar rows: the entry-list kernels serve multiples of 4 only, so dim 7 is the sorted-position pipeline's scalar class)
  assert G.class_of("entry", 7) is None and G.class_of("sorted", 7) == (1, 8, 1)
  assert G.class_of("entry", 32) == (4, 8, 1)
  assert G.class_of("entry", 512) is None and G.class_of("sorted", 512) == (4, 64, 2)
  assert all(G.dim_supported(D) for D in C.DIMS)
  assert G.class_of("entry", C.CASE2_D) is not None and G.class_of("entry", 4) is not None


def test_init_rows_is_the_models_init_rule():
  rng = np.random.default_rng(3)
  init = rng.standard_normal((32, 4)).astype(np.float32)
  keys = np.concatenate([rng.integers(-(1 << 62), 1 << 62, 200), np.arange(-5, 5)]).astype(np.int64)
  for seed in (0, 7, (1 << 63) + 5):
    t = M.Table(4, init, seed)
    want = np.stack([t.init_row(int(k)) for k in keys])
    assert np.array_equal(C.init_rows(keys, seed, init).view(np.uint32), want.view(np.uint32))


CASES = sorted(set((f, D, C.has_lookup(s)) for f, D, s in C.CASE1))


@pytest.mark.parametrize("family,D,lookup", CASES, ids=["%s-%d-%s" % (f, D, "lookup" if l else "alone") for f, D, l in CASES])
def test_trajectory_conditions(family, D, lookup):
  _conditions(family, D, lookup, 1)


@pytest.mark.parametrize("family", C.CASE5)
def test_batched_trajectory_conditions(family):
  _conditions(family, 32, True, C.TABLES)


def _conditions(family, D, lookup, tables):
  tr = C.trajectory(family, D, lookup, tables)
  assert len(tr["tables"]) == tables
  n = C.replay_batches(C.SEEDS)["n"]
  for tb in tr["tables"]:
    assert len(tb["steps"]) == C.R + 1
    total = [0] * len(tb["steps"][0]["tables"])
    for k, st in enumerate(tb["steps"]):
      tag = "%s D=%d step %d" % (family, D, k)
      nvar, nslot = C.new_keys(st["batch"], family, lookup)
      got = [t["new"] for t in st["tables"]]
      assert got == [nvar] + [nslot] * (len(got) - 1), tag                     # the rules' counts are the reference's
      assert int(st["live"].sum()) == nslot and 0 < nvar < nslot, tag
      # present, new and — but for plain Adam, which has no filter — below-threshold keys in every step
      assert (nslot == st["batch"]["keys"].size) == (family == "adam"), tag
      if k:
        total = [a + b for a, b in zip(total, got)]
      assert st["clear"].all(), tag                                             # no row within SKIP_BELOW of its threshold
      if family in G.GROUP_FAMILIES:
        assert 0 < int(st["black"].sum()) < int(st["live"].sum()), tag           # both branches, by the reference alone
      if st["zeros"] is not None:
        assert 0 < st["zeros"][0] < st["zeros"][1], tag
      if lookup:                                                                # every row a lookup returns is an init-rule row
        want = C.init_rows(st["ids"], tb["seed"], tb["vinit"])
        assert np.array_equal(st["lookup"].view(np.uint32), want.view(np.uint32)), tag
      # repeated ids: gradients on the 2^-10 grid, so every order sums them to the same bits
      rep = np.isin(st["ids"], st["batch"]["keys"][st["batch"]["counts"] > 1])
      assert rep.any() and (~rep).any()
    # the room: the replays' new keys fit R n, and the captured calls' ids fit what is prepared on top of it
    for shape in C.SHAPES:
      if C.has_lookup(shape) == lookup:
        rv, rs = C.room(shape, n)
        cv, cs = C.captured_ids(shape, n)
        assert total[0] + cv <= rv and all(t + cs <= rs for t in total[1:])
        assert total[0] <= C.R * n and cv <= rv - C.R * n
  if family in G.GROUP_FAMILIES and family in G.ORACLE_FAMILIES:
    print("%s D=%d: ref_err %.3g" % (family, D, max(st["ref_err"] for tb in tr["tables"] for st in tb["steps"])))


@pytest.mark.parametrize("early,new_day", [(False, False), (True, False), (False, True)], ids=["a", "b", "c"])
def test_case2_model(early, new_day):
  tr = C.case2_trajectory(early, new_day)
  free = 0                                                    # the free list, by the ops' rules
  pops = []
  for k, st in enumerate(tr["steps"]):
    if k == 1 and early:
      free += tr["early"].size
    free += st["deleted"].size
    b = st["batch"]
    assert np.isin(st["deleted"], b["keys"]).all() and np.isin(st["deleted"], b["pre"]).all()
    inserted = b["new"].size + st["deleted"].size
    if k >= 1:
      pops.append(min(free, inserted) if early else 0)         # (a): the graph was captured without the list
      free -= pops[-1]
    # a key deleted and inserted again: its frequency is its occurrences in the batch, its day the capture's
    occ = dict(zip(b["keys"].tolist(), b["counts"].tolist()))
    for key in st["deleted"].tolist():
      m = st["tables"][0]["metas"][int(np.flatnonzero(b["keys"] == key)[0])]
      assert m["freq"] == occ[key] and m["day"] == G.DAY
    assert all(m["day"] == G.DAY for m in st["tables"][1]["metas"])
  if early:                                                   # the list runs empty inside a replay: pops, then fresh rows
    assert pops[0] == tr["steps"][1]["batch"]["new"].size and 0 < pops[1] < tr["steps"][2]["batch"]["new"].size + tr["steps"][2]["deleted"].size
    assert free == sum(st["deleted"].size for st in tr["steps"][3:]) - sum(pops[2:])
  elif not new_day:
    assert all(st["deleted"].size > 0 for st in tr["steps"][2:]) and tr["steps"][1]["deleted"].size == 0
  assert C.NEW_DAY != G.DAY


def test_bounds_case_inequalities():
  c = C.bounds_case()
  assert c["chunk"] == 1 << 16 and (c["n"], c["replays"], c["dim"]) == (4096, 3, 4)
  assert c["prepared"] == c["replays"] * c["n"] and c["lag"] == (c["replays"] - 1) * c["n"] >= c["n"]
  # the index: the host keeps its own bound of claimed entries at or below half of the capacity, a power of two; with a
  # prefill of 4 lag the capacity is at least 8 lag, so the device, `lag` entries ahead, stays below three quarters
  assert c["prefill"] >= 4 * c["lag"]
  cap = 1024
  while cap < 2 * c["prefill"]:
    cap *= 2
  assert cap >= 8 * c["lag"] and cap // 2 + c["lag"] <= 3 * cap // 4
  # more than two growth chunks of rows since the capture, all by calls that kept the contract
  assert (c["replays"] + c["eager"]) * c["n"] > 2 * c["chunk"] and (c["replays"] + c["eager"] - 1) * c["n"] <= 2 * c["chunk"]
  # a bound that lags by at least n lets the device cross the end of the slab one call before the host looks: walk the
  # host's old rule (refresh only when its own bound crosses) and see the device pass rows_cap first
  host = dev = 1 + c["prefill"] + c["n"]
  host, dev, rows_cap = host + c["n"], dev + c["replays"] * c["n"], C.slab_after(1, host, c["chunk"], c["chunk"])
  crossed = False
  for _ in range(c["eager"]):
    if host + c["n"] > rows_cap:
      break
    host, dev = host + c["n"], dev + c["n"]
    crossed |= dev > rows_cap
  assert crossed
  pre, warm, reps, eager = C.bounds_keys(c)
  assert (pre.size, warm.size, len(reps), len(eager)) == (c["prefill"], c["n"], c["replays"], c["eager"])
  assert all(k.size == c["n"] for k in reps + eager)


def test_refusal_case_inequalities():
  c = C.refusal_case()
  assert c["m"] % c["chunk"] == 0 and c["m"] >= c["chunk"]
  assert c["rows"] + c["m"] > c["rows_cap"] >= c["rows"] + c["after"]      # the m copies cannot fit; the op captured next can
  assert c["rows"] == 1 + c["small"] + c["m"]
