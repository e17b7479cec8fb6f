"""Graph replays that do what a capture is for: every replay runs on ids other than those of its capture.

The five older capture tests replay one buffer of unique ids that were all inserted before the capture, against an eager
twin alone.  Here (tests/_capture_cases.py builds the cases, tests/test_capture_cases.py holds their conditions on the CPU)
a replay inserts keys (the init rule, enter_threshold, the row allocator and the free list run from a graph), sees repeated
ids (the cold, hot and chunked branches of the apply kernels), and is held against oracle.kv_oracle or tests/_kv_model.py
carrying the captured step — with the scalars of its capture — over batch 0, 1, ... R - 1, AND against an eager twin fed the
same batches, bit for bit (the repeated ids' gradients are on a 2^-10 grid: every order sums them to the same bits, whatever
partition count either side picked).

  1. fresh ids per replay, one table set: eight families at dim 32, three of them at 7 and 512 (_capture_cases.DIMS), the
     captured step in four shapes (_capture_cases.SHAPES);
  2. state changed between replays: kv_delete of keys the next replay inserts again, with the free list outside (a) and
     inside (b) the graph; (c) kv_set_clock_days between replays: the day travels by value, a replay stamps the day of
     its capture (include/kvhip.h kv_prepare_capture says so);
  3. the host's bounds after replays: eager calls behind replays that inserted more than the capture told the host, past two
     growth chunks, with no figure call in between that would refresh the bounds by accident;
  4. a captured call that needs more room than kv_prepare_capture settled: KV_FAILED_PRECONDITION before anything is queued,
     the capture stays valid;
  5. the batched forms over three tables.

Every capture is on a side stream, behind one warm-up of the same step and length outside it and kv_prepare_capture on every
table; batch k's ids and gradient rows are copied into the captured buffers before replay k.

Case 4's setup: the warm-up (a lookup of m copies of one present key) makes the host grow the slab for m new rows and
inserts none, so right behind it m new rows WOULD fit; one eager lookup of m fresh keys takes that room first.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _capture_cases as C  # noqa: E402
import _row_geometry as G  # noqa: E402

F = np.float32
R = C.R


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _table(ops, D, init, thr=0, seed=0, cap=64):
  h = ops.kv_variable([D], enter_threshold=thr, capacity_hint=cap)
  ops.kv_set_clock_days(h, G.DAY)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, init)
  return h


def _single(ops, family):
  return {"group_adam_v4": ops.kv_variable_group_sparse_apply_adam_v4, "group_adam_v3": ops.kv_variable_group_sparse_apply_adam_v3,
          "sparse_group_ftrl": ops.kv_variable_sparse_group_sparse_apply_ftrl_v2, "ftrl_v2": ops.kv_variable_sparse_apply_ftrl_v2,
          "group_ftrl_v2": ops.kv_variable_group_sparse_apply_ftrl_v2,
          "group_radam": ops.kv_variable_group_sparse_apply_rectified_adam, "adam": ops.kv_variable_sparse_apply_adam}[family]


def _apply(ops, family, hs, grad, ids, hp, **kw):
  if family == "adagrad":
    return ops.kv_variable_sparse_apply_adagrad(hs[0], hs[1], hp[0], grad, ids, update_slots=hp[1], **kw)
  if family.startswith("group_adam"):
    hp = hp[:9]
  return _single(ops, family)(*hs, grad, ids, *hp, **kw)


def _apply_multi(ops, family, sets, grads, idl, hp):
  roles = [[hs[j] for hs in sets] for j in range(len(sets[0]))]
  if family.startswith("group_adam"):
    return ops.kv_multi_group_sparse_apply_adam(*roles, grads, idl, *hp[:9], version=hp[9])
  return {"ftrl_v2": ops.kv_multi_sparse_apply_ftrl_v2}[family](*roles, grads, idl, *hp)


def _capture(fn):
  """fn recorded into a graph on a side stream."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=side):
    fn()
  return g


def _same_bits(got, want, tag):
  got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
  assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, np.argwhere(got != want)[:5])


class Rig(object):
  """One table set (var, slot tables) with every batch's `pre` lookup done, and the buffers its step reads: the captured
  step's arguments are these buffers, so a replay runs on whatever load() put there."""

  def __init__(self, ops, family, D, tb, shape, hp):
    self.ops, self.family, self.shape, self.hp = ops, family, shape, hp
    self.hs = [_table(ops, D, tb["vinit"], thr=G.ENTER, seed=tb["seed"])] + \
              [_table(ops, d, i, seed=tb["seed"]) for d, i in zip(G.slot_dims(family, D), tb["sinits"])]
    for pre in tb["pre"]:
      ops.kv_variable_gather_or_insert_v2(self.hs[0], pre)
    st = tb["steps"][0]
    self.n = int((st["u"] if shape == "unique" else st["ids"]).size)
    self.ids = torch.zeros(self.n, dtype=torch.int64, device="cuda")
    self.ids2 = torch.zeros_like(self.ids)                   # the same ids in another tensor: an apply that gets no token
    self.grad = torch.zeros(self.n, D, device="cuda")
    self.out = None

  def load(self, st):
    ids, grad = (st["u"], st["s"]) if self.shape == "unique" else (st["ids"], st["grad"])
    assert ids.size == self.n
    self.ids.copy_(torch.from_numpy(np.ascontiguousarray(ids)))
    self.ids2.copy_(self.ids)
    self.grad.copy_(torch.from_numpy(np.ascontiguousarray(grad)))

  def step(self, warm=False):
    """warm: the warm-up of the "unique" shape is the plain op on the same unique ids — under capture the _unique op runs
    the batch pipeline (same bits), whose workspace only the plain op sizes; a captured call cannot (it would be refused)."""
    ops = self.ops
    if C.has_lookup(self.shape):
      self.out = ops.kv_variable_gather_or_insert_v2(self.hs[0], self.ids)
    _apply(ops, self.family, self.hs, self.grad, self.ids if self.shape == "tok" else self.ids2, self.hp,
           unique_indices=self.shape == "unique" and not warm)

  def prepare(self):
    torch.cuda.synchronize()
    rv, rs = C.room(self.shape, self.n)
    for h, m in zip(self.hs, [rv] + [rs] * (len(self.hs) - 1)):
      self.ops.kv_prepare_capture(h, m)

  def lookup_is(self, st, tag):
    if C.has_lookup(self.shape):
      _same_bits(_np(self.out), st["lookup"], tag + " lookup rows")


def _check_rows(ops, hs, st, exact, tag):
  """The rows, records and time stamps of one step's keys against the reference."""
  keys, clear = st["batch"]["keys"], st.get("clear")
  for j, (h, t) in enumerate(zip(hs, st["tables"])):
    got = _np(ops.kv_variable_gather_or_zeros_v2(h, keys))
    if exact:
      _same_bits(got, t["rows32"], "%s table %d" % (tag, j))
    else:
      g64 = got.astype(np.float64)
      ok = np.abs(g64 - t["rows32"]) <= t["tol"]             # the project's bar against the float32 reference, or
      if t["rows64"] is not None:                            # max(bar, 4 x the reference's own error) against float64, per row
        ok |= np.abs(g64 - t["rows64"]) <= t["widen"] * t["tol"]
      bad = ~ok & clear[:, None]
      assert not bad.any(), (tag, "table %d" % j, np.argwhere(bad)[:5], got[bad][:5], t["rows32"][bad][:5], t["tol"][bad][:5])
    gm = ops.kv_get_meta(h, keys)
    diff = [(int(k), a, e) for k, a, e in zip(keys, gm, t["metas"]) if a != e]
    assert not diff, (tag, "table %d" % j, diff[:5])
    days = [G.DAY if m is None else m["day"] for m in t["metas"]]          # (an absent key reads today)
    assert _np(ops.kv_variable_get_time_stamp(h, keys)).tolist() == days, (tag, j)


def _counters(ops, h):
  return (ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h))


def _same_tables(ops, a, b, keys, tag):
  """The captured rig and its eager twin: bit for bit."""
  for j, (x, y) in enumerate(zip(a, b)):
    assert torch.equal(ops.kv_variable_gather_or_zeros_v2(x, keys).view(torch.int32),
                       ops.kv_variable_gather_or_zeros_v2(y, keys).view(torch.int32)), (tag, j)
    assert ops.kv_get_meta(x, keys) == ops.kv_get_meta(y, keys), (tag, j)
    assert _counters(ops, x) == _counters(ops, y), (tag, j)


# ---- 1. fresh ids per replay -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,D,shape", C.CASE1, ids=["%s-%d-%s" % c for c in C.CASE1])
def test_replays_on_fresh_ids(ops, family, D, shape):
  tr = C.trajectory(family, D, C.has_lookup(shape))
  tb, hp = tr["tables"][0], tr["hp"]
  steps = tb["steps"]
  cap, twin = Rig(ops, family, D, tb, shape, hp), Rig(ops, family, D, tb, shape, hp)
  for rig in (cap, twin):                                    # the warm-up, outside the capture, on a batch of its own
    rig.load(steps[0])
    rig.step(warm=True)
    rig.lookup_is(steps[0], "warm-up")
  cap.prepare()
  g = _capture(cap.step)
  for k in range(1, R + 1):
    tag = "%s D=%d %s replay %d" % (family, D, shape, k - 1)
    cap.load(steps[k])
    g.replay()
    torch.cuda.synchronize()
    cap.lookup_is(steps[k], tag)
    twin.load(steps[k])
    twin.step()
    twin.lookup_is(steps[k], tag + " (twin)")
  for name, rig in (("captured", cap), ("twin", twin)):
    for k, st in enumerate(steps):
      _check_rows(ops, rig.hs, st, tr["exact"], "%s D=%d %s %s step %d" % (family, D, shape, name, k))
    for j, h in enumerate(rig.hs):
      assert _counters(ops, h) == tb["counters"][j], (family, D, shape, name, j)
  _same_tables(ops, cap.hs, twin.hs, np.concatenate([st["batch"]["keys"] for st in steps]), "%s D=%d %s" % (family, D, shape))


# ---- 2. state changed between replays ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["a", "b", "c"])
def test_state_changed_between_replays(ops, variant):
  """(a) the graph is captured before any delete (no free list in it: a replay takes fresh rows whatever was released since),
  (b) after one (the replays pop the list empty, then take fresh rows); either way kv_delete removes keys of the next batch
  between replays and the replay inserts them again through their tombstones: the init rule's row, the frequency afresh.
  (c) kv_set_clock_days between replays: the replays go on stamping the day of their capture."""
  early, new_day = variant == "b", variant == "c"
  tr = C.case2_trajectory(early, new_day)
  family, D, steps = C.CASE2_FAMILY, C.CASE2_D, tr["steps"]
  rigs = [Rig(ops, family, D, tr, "tok", tr["hp"]) for _ in range(1 if new_day else 2)]
  cap = rigs[0]
  for rig in rigs:
    ops.kv_variable_gather_or_insert_v2(rig.hs[0], tr["early"])
    rig.load(steps[0])
    rig.step(warm=True)
    rig.lookup_is(steps[0], "warm-up")
    if early:
      assert ops.kv_variable_delete(rig.hs[0], tr["early"]) == tr["early"].size
  cap.prepare()
  g = _capture(cap.step)
  for k in range(1, R + 1):
    st, tag = steps[k], "variant %s replay %d" % (variant, k - 1)
    for rig in rigs:
      if st["deleted"].size:
        assert ops.kv_variable_delete(rig.hs[0], st["deleted"]) == st["deleted"].size
      if new_day and k == 2:
        for h in rig.hs:
          ops.kv_set_clock_days(h, C.NEW_DAY)
      rig.load(st)
      if rig is cap:
        g.replay()
        torch.cuda.synchronize()
      else:
        rig.step()
      rig.lookup_is(st, tag)
      _check_rows(ops, rig.hs, st, True, tag)
      for j, h in enumerate(rig.hs):
        assert _counters(ops, h) == st["counters"][j], (tag, j)
  if new_day:                                                # the clock did move: an absent key reads today
    absent = np.array([(1 << 40) + 1], np.int64)
    assert _np(ops.kv_variable_get_time_stamp(cap.hs[0], absent)).tolist() == [C.NEW_DAY]
    assert all(m["day"] == G.DAY for st in steps[2:] for m in ops.kv_get_meta(cap.hs[0], st["batch"]["keys"]))
  else:
    _same_tables(ops, rigs[0].hs, rigs[1].hs, np.concatenate([st["batch"]["keys"] for st in steps] + [tr["early"]]), variant)


# ---- 3. the host's bounds after replays --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eager_op", ["lookup", "apply"])
def test_host_bounds_after_replays(ops, eager_op):
  """A captured call tells the host's bounds its n ids once; R replays on fresh ids insert R n rows.  The eager calls that
  follow must see the device's counts, not the host's stale ones: with a bound that lags, the device reaches the end of the
  slab one call before the host looks (tests/test_capture_cases.py walks it) and drops the batch.  No figure call (they
  refresh the bounds) between the capture and the end.  apply: the captured step is lookup + Adagrad, the eager op Adagrad
  alone (it inserts into the var and the slot table itself); gradients of zero, so every var row stays its init-rule row."""
  c = C.bounds_case()
  pre, warm, reps, eager = C.bounds_keys(c)
  n, D, with_apply = c["n"], c["dim"], eager_op == "apply"
  init = np.random.default_rng(17).standard_normal((32, D)).astype(F)
  var = _table(ops, D, init, seed=5, cap=0)                  # no capacity_hint: the slab grows chunk by chunk
  acc = _table(ops, D, np.full((4, D), 0.1, F), seed=5, cap=0)
  hs = [var, acc] if with_apply else [var]
  zeros = torch.zeros(n, D, device="cuda")
  ids = torch.zeros(n, dtype=torch.int64, device="cuda")
  box = {}

  def adagrad(i, g):
    ops.kv_variable_sparse_apply_adagrad(var, acc, 0.05, g, i)

  def step():
    box["out"] = ops.kv_variable_gather_or_insert_v2(var, ids)
    if with_apply:
      adagrad(ids, zeros)

  if with_apply:
    adagrad(torch.from_numpy(pre).cuda(), torch.zeros(pre.size, D, device="cuda"))
  else:
    ops.kv_variable_gather_or_insert_v2(var, pre)
  ids.copy_(torch.from_numpy(warm))
  step()
  torch.cuda.synchronize()
  for h in hs:
    ops.kv_prepare_capture(h, c["prepared"])
  g = _capture(step)
  for k, keys in enumerate(reps):
    ids.copy_(torch.from_numpy(keys))
    g.replay()
    torch.cuda.synchronize()
    _same_bits(_np(box["out"]), C.init_rows(keys, 5, init), "replay %d" % k)
  for keys in eager:                                         # every call returns KV_OK (anything else raises)
    if with_apply:
      adagrad(torch.from_numpy(keys).cuda(), zeros)
    else:
      ops.kv_variable_gather_or_insert_v2(var, keys)
  torch.cuda.synchronize()
  every = np.concatenate([pre, warm] + reps + eager)
  assert every.size == c["total"]
  _same_bits(_np(ops.kv_variable_gather_or_zeros_v2(var, every)), C.init_rows(every, 5, init), "every key's row")
  assert _counters(ops, var) == (c["total"], c["total"], c["total"])           # (a deferred error would be raised here)
  if with_apply:
    _same_bits(_np(ops.kv_variable_gather_or_zeros_v2(acc, every)), np.full((every.size, D), 0.1, F), "every slot row")
    assert _counters(ops, acc)[:2] == (c["total"], c["total"])


# ---- 4. a captured call beyond the prepared room -----------------------------------------------------------------------------
def test_captured_call_beyond_the_prepared_room_is_refused(ops):
  from tfplus_amd import _lib
  c = C.refusal_case()
  m, D = c["m"], c["dim"]
  init = np.random.default_rng(19).standard_normal((32, D)).astype(F)
  h = _table(ops, D, init, seed=9, cap=0)
  small = np.arange(1, c["small"] + 1, dtype=np.int64) * 7919
  fill = (np.arange(1, m + 1, dtype=np.int64) << 20) + 3
  ops.kv_variable_gather_or_insert_v2(h, small)
  copies = torch.full((m,), int(small[0]), dtype=torch.int64, device="cuda")
  ops.kv_variable_gather_or_insert_v2(h, copies)             # the warm-up: the workspace has its size, nothing is inserted
  ops.kv_variable_gather_or_insert_v2(h, fill)               # ... and the room the host made for it is taken
  assert ops.kv_variable_shape_v2(h)[0] == c["rows"] - 1
  freq = ops.kv_variable_frequency(h)
  torch.cuda.synchronize()
  ops.kv_prepare_capture(h, 0)
  present = torch.zeros(c["after"], dtype=torch.int64, device="cuda")
  box = {}

  def body():
    with pytest.raises(_lib.FailedPreconditionError):        # refused before anything is queued: the capture goes on
      ops.kv_variable_gather_or_insert_v2(h, copies)
    box["out"] = ops.kv_variable_gather_or_insert_v2(h, present)

  g = _capture(body)
  rng = np.random.default_rng(23)
  for rep in range(2):
    now = fill[rng.integers(0, m, c["after"])]
    present.copy_(torch.from_numpy(now))
    g.replay()
    torch.cuda.synchronize()
    _same_bits(_np(box["out"]), C.init_rows(now, 9, init), "replay %d" % rep)
  assert _counters(ops, h) == (c["rows"] - 1, c["rows"] - 1, freq + 2 * c["after"])


# ---- 5. the batched forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.CASE5)
def test_batched_forms_replay_on_fresh_ids(ops, family):
  D = 32
  tr = C.trajectory(family, D, True, C.TABLES)
  hp = tr["hp"]

  class Multi(object):
    def __init__(self):
      self.rigs = [Rig(ops, family, D, tb, "tok", hp) for tb in tr["tables"]]
      self.outs = None

    def load(self, k):
      for rig, tb in zip(self.rigs, tr["tables"]):
        rig.load(tb["steps"][k])

    def step(self):
      self.outs = ops.kv_multi_gather_or_insert([r.hs[0] for r in self.rigs], [r.ids for r in self.rigs])
      _apply_multi(ops, family, [r.hs for r in self.rigs], [r.grad for r in self.rigs], [r.ids for r in self.rigs], hp)

    def lookups_are(self, k, tag):
      for i, (o, tb) in enumerate(zip(self.outs, tr["tables"])):
        _same_bits(_np(o), tb["steps"][k]["lookup"], "%s table set %d" % (tag, i))

  cap, twin = Multi(), Multi()
  for m in (cap, twin):
    m.load(0)
    m.step()
    m.lookups_are(0, "warm-up")
  for rig in cap.rigs:
    rig.prepare()
  g = _capture(cap.step)
  for k in range(1, R + 1):
    cap.load(k)
    g.replay()
    torch.cuda.synchronize()
    cap.lookups_are(k, "replay %d" % (k - 1))
    twin.load(k)
    twin.step()
    twin.lookups_are(k, "replay %d (twin)" % (k - 1))
  for name, m in (("captured", cap), ("twin", twin)):
    for i, (rig, tb) in enumerate(zip(m.rigs, tr["tables"])):
      for k, st in enumerate(tb["steps"]):
        _check_rows(ops, rig.hs, st, tr["exact"], "%s %s set %d step %d" % (family, name, i, k))
      for j, h in enumerate(rig.hs):
        assert _counters(ops, h) == tb["counters"][j], (family, name, i, j)
  for a, b, tb in zip(cap.rigs, twin.rigs, tr["tables"]):
    _same_tables(ops, a.hs, b.hs, np.concatenate([st["batch"]["keys"] for st in tb["steps"]]), family)
