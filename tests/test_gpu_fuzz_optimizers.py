"""Randomised differential test of the four optimizer families tests/test_gpu_fuzz.py cannot drive (the oracle does not
restate them): FTRL-V2, group FTRL-V2, group RectifiedAdam and plain Adam.  A 40-step random program (tests/_kv_model.py
Program) of lookups, applies in five forms (plain, with the lookup's token, unique, counted, batched), scatters, inserts,
deletes that fall on a random subset of {var, slots}, expiries and read-only queries runs side by side on two sets of GPU
tables and on the host model, which carries the whole state by itself: nothing the device says is ever fed back.  After
every op, on the var and every slot table: map size, size, frequency sum, and on 200 sampled keys (the whole key universe
when it is small, and always after the last step) rows, counts, time stamps and the records of kv_get_meta — frequency
word, day, blacklist, under_threshold.

Unique mode hands the ops TF-core's unique ids and occurrence-ordered sums; occurrence mode (KV_ORDER_OCCURRENCE) the raw
ids.  Either way the summed gradient is exact (the counted form, whose sums the device makes in its own order, gets
gradients that any order sums exactly).  The library offers the counted and the batched ops for dims that are multiples
of 4 only, so the programs at D = 5 and 6 draw from the other three forms; and the batched ops refuse a var in occurrence
mode, so there the vars leave that mode for the one call, which gets the unique ids.

Plain Adam, FTRL-V2 and group RAdam with l21 = 0 are held bit for bit for the whole program.  Group FTRL-V2, and group
RAdam with l21 > 0 (seed % 3 == 1), within the allowance the model carries per key (tests/_kv_model.py); the generator's
conditions — no key within 0.5 % of a lasso threshold, no var row's allowance above 1e-3 of the row — and the allowance
itself against float64 evaluations are asserted on the CPU for exactly these seeds (tests/test_kv_model.py).

Worst observed / allowed on an MI355X over all seeds and both modes: group FTRL-V2 0.612 (seed 7, occurrence mode), group
RAdam 0.649 (seed 1, occurrence mode).
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _kv_model as M  # noqa: E402

F = np.float32

@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _single(ops, family):
  return {"ftrl_v2": ops.kv_variable_sparse_apply_ftrl_v2, "group_ftrl_v2": ops.kv_variable_group_sparse_apply_ftrl_v2,
          "group_radam": ops.kv_variable_group_sparse_apply_rectified_adam, "adam": ops.kv_variable_sparse_apply_adam}[family]


def _multi(ops, family):
  return {"ftrl_v2": ops.kv_multi_sparse_apply_ftrl_v2, "group_ftrl_v2": ops.kv_multi_group_sparse_apply_ftrl_v2,
          "group_radam": ops.kv_multi_group_sparse_apply_rectified_adam, "adam": ops.kv_multi_sparse_apply_adam}[family]


class Run(object):
  """One program on the GPU tables next to its models."""

  def __init__(self, ops, family, seed, occ):
    self.ops, self.prog = ops, M.Program(family, seed, occ)
    p = self.prog
    self.kd = torch.int32 if p.int32 else torch.int64
    self.sets = []
    for ts in p.sets:
      hs = []
      for t, init in zip(ts.tables, [ts.vinit] + ts.sinits):
        h = ops.kv_variable([t.dim], enter_threshold=t.enter_threshold, capacity_hint=64, key_dtype=self.kd)  # tiny hint: growth
        ops.kv_set_seed(h, ts.seed); ops.init_kv_variable_v2(h, init); ops.kv_set_clock_days(h, M.DAY0)
        hs.append(h)
      if occ:
        ops.kv_set_deterministic(hs[0], ops.KV_ORDER_OCCURRENCE)
      self.sets.append(hs)
    self.worst = 0.0

  def dev(self, ids):
    return torch.from_numpy(np.asarray(ids).astype(np.int32 if self.prog.int32 else np.int64)).cuda()

  def same_rows(self, got, want, tol, tag):
    got = np.asarray(got, F)
    if self.prog.exact:
      assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, np.argwhere(got != want)[:5])
      return
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= tol)                                      # (a NaN is over any allowance)
    assert not bad.any(), (tag, np.argwhere(bad)[:5], err[bad][:5], tol[bad][:5])
    if (tol > 0).any():
      self.worst = max(self.worst, float((err[tol > 0] / tol[tol > 0]).max()))

  def check(self, st, tag):
    ops = self.ops
    for hs, ts, keys in zip(self.sets, self.prog.sets, st["check"]):
      for j, (h, m) in enumerate(zip(hs, ts.tables)):
        t = "%s table %d" % (tag, j)
        assert (ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)) == \
            (m.map_size(), m.size(), m.sum_freq()), t
        self.same_rows(_np(ops.kv_variable_gather_or_zeros_v2(h, keys)), m.gather_or_zeros(keys), m.tols(keys), t)
        assert np.array_equal(_np(ops.kv_variable_get_count_v2(h, keys)), m.get_count(keys)), t
        assert np.array_equal(_np(ops.kv_variable_get_time_stamp(h, keys)), m.get_timestamp(keys)), t
        got, want = ops.kv_get_meta(h, keys), m.metas(keys)
        assert got == want, (t, [(int(k), g, w) for k, g, w in zip(keys, got, want) if g != w][:5])

  def apply(self, rep, tag):
    ops, p, form, hp = self.ops, self.prog, rep["form"], rep["hp"]
    fn = _single(ops, p.family)
    fed = [(a["ids"], a["grad"]) if p.occ else (a["u"], a["s"]) for a in rep["sets"]]     # the raw ids only where the op sums them itself
    if form == "batched":     # one call for A and B.  The batched ops refuse a table in occurrence-order mode: there the two vars
      # leave it for this call, which then gets the unique ids and their sums
      roles = [[hs[j] for hs in self.sets] for j in range(len(self.sets[0]))]
      for h in roles[0] if p.occ else []:
        ops.kv_set_deterministic(h, ops.KV_ORDER_ARRIVAL)
      _multi(ops, p.family)(*roles, [a["s"] for a in rep["sets"]], [a["u"] for a in rep["sets"]], *hp)
      for h in roles[0] if p.occ else []:
        ops.kv_set_deterministic(h, ops.KV_ORDER_OCCURRENCE)
      return
    for hs, a, (ids, g) in zip(self.sets, rep["sets"], fed):
      if form == "plain":
        fn(*hs, g, ids, *hp)
      elif form == "tok":                                    # a training lookup of a CUDA tensor, then the very same tensor object
        t = self.dev(ids)
        self.same_rows(_np(ops.kv_variable_gather_or_insert_v2(hs[0], t)), a["tok_rows"], a["tok_tol"], tag + " tok lookup")
        fn(*hs, torch.from_numpy(g).cuda(), t, *hp)
      elif form == "unique":
        fn(*hs, a["s"], a["u"], *hp, unique_indices=True)
      else:                                                  # counted: the unique count stays on the device
        if a["variant"] == 0:
          uu, ss, _, nu = ops.kv_dedup_segment_sum(hs[0], a["ids"], a["grad"], sync=False)
        else:
          uu, _, inv, nu = ops.kv_unique(hs[0], a["ids"], sync=False)
          ss = ops.kv_unsorted_segment_sum(hs[0], a["grad"], inv, a["ids"].size)
        fn(*hs, ss, uu, *hp, unique_count=nu)

  def step(self, st):
    ops, p, op = self.ops, self.prog, st["op"]
    tag = "%s seed %d %s step %d %s D=%d" % (p.family, p.seed, "occ" if p.occ else "uniq", st["step"], op, p.D)
    if op == "apply":
      for r, rep in enumerate(st["reps"]):
        self.apply(rep, "%s %s rep %d" % (tag, st["form"], r))
      tag += " " + st["form"]
    elif op == "expire":
      for hs, a in zip(self.sets, st["sets"]):
        for h in hs:
          ops.kv_set_clock_days(h, st["day"])
        assert sorted(_np(ops.kv_variable_delete_with_timestamp(hs[0], st["thr_days"])).tolist()) == a["gone"], tag
    else:
      for hs, a in zip(self.sets, st["sets"]):
        ids = a["ids"]
        if op == "lookup":
          self.same_rows(_np(ops.kv_variable_gather_or_insert_v2(hs[0], ids)), a["rows"], a["tol"], tag)
        elif op == "lookup_counts":
          self.same_rows(_np(ops.kv_variable_gather_or_insert_with_counts(hs[0], ids, a["counts"])), a["rows"], a["tol"], tag)
        elif op == "scatter":
          [ops.kv_variable_scatter_update_v2, ops.kv_variable_scatter_add_v2, ops.kv_variable_scatter_sub_v2,
           ops.kv_variable_scatter_mul_v2, ops.kv_variable_scatter_div_v2, ops.kv_variable_scatter_min_v2,
           ops.kv_variable_scatter_max_v2][a["which"]](hs[0], ids, a["upd"])
        elif op == "insert":
          ops.kv_variable_insert_v2(hs[0], ids, a["vals"])
        elif op == "delete":
          assert [ops.kv_variable_delete(hs[j], ids) for j in a["tables"]] == a["gone"], tag
        elif a["table"] == 0:                                # query: the fused serving lookup, every id its own segment
          got = ops.kv_variable_lookup_sparse_zeros(hs[0], ids, np.arange(ids.size), None, ids.size, "sum")
          self.same_rows(_np(got) + F(0), a["rows"] + F(0), a["tol"], tag)          # (+ 0: a sum may turn -0 into +0)
        else:
          self.same_rows(_np(ops.kv_variable_gather_or_zeros_v2(hs[a["table"]], ids)), a["rows"], a["tol"], tag)
    self.check(st, tag)


CASES = [(f, s, occ) for f in M.FAMILIES for occ in (False, True) for s in M.SEEDS[f]]


@pytest.mark.parametrize("family,seed,occ", CASES, ids=["%s-%d-%s" % (f, s, "occ" if o else "uniq") for f, s, o in CASES])
def test_random_program_matches_model(ops, family, seed, occ):
  run = Run(ops, family, seed, occ)
  for st in run.prog.steps():
    run.step(st)
  p = run.prog
  if not p.exact:
    print("%s seed %d %s: worst observed / allowed %.3g" % (family, seed, "occ" if occ else "uniq", run.worst))
    assert run.worst <= 1.0
  # a one-slot family at a dim of the entry-list kernels: the program has met the applies that work on the slot mirrors
  assert p.stats["applies"] > 0
  if family in ("group_radam", "adam") and p.D % 4 == 0:
    for hs in run.sets:
      assert ops.kv_get_stat(hs[0], ops.KV_STAT_MIRROR_APPLIES) > 0
