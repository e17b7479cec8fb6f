"""Random programs for SHARDED tables, carried on one unsharded host model: the premise of every sharded test — the shards
of a table behave together as the one unsharded table fed every rank's ids — held step after step.

  ShardProgram   a 24-step random program of one optimizer family on two table sets A and B (a var and its slot tables
                 each), deterministic in (family, seed).  It carries ONE UNSHARDED model per set and yields every step after
                 the model has taken it, as _kv_model.Program.steps() does: what the step was, what every rank feeds, what
                 every rank must get back.  Nothing the device says is fed back.
  ShardedModel   `world` models per table set, one per owner, fed what the owners are fed: per sending rank its distinct ids
                 as (id, count) records; applies go to each owner with its keys.  tests/test_shard_program.py runs it next to
                 the unsharded model and holds the union of the owners' tables equal to the unsharded table, bit for bit.

Families: ftrl_v2 (optimizer code 4, two slot tables), adam (7) and group_radam with l21 = 0 (6, whose l1 = median rule
gives the blacklist / lift cycle) are carried by _kv_model.apply_step and hold bit for bit; group_adam_v4 (0, the headline
op) is carried by oracle.kv_oracle.OracleKv and holds at tests/test_gpu_fuzz.py's bar.

Gradients are multiples of _kv_model.GQ of both signs, and for every step and key the sum of |g| / GQ over all ranks'
occurrences stays below 2^24 (asserted): every partial sum is then a float32, so the per-rank pre-sum and the owner's sum
across ranks are exact in any order and the model applies the sum of the concatenated batches.

Which ops between a lookup and its apply make the owner's serve token stale (kv_batch_index.h, the batch.drop() sites):
STALE below — delete, scatter and insert of at least one id drop the table's batch index; gather_or_zeros, get_count and
kv_get_meta enter through join_side, which settles the pending partition pass and keeps the token.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
  if _p not in sys.path:
    sys.path.insert(0, _p)
import _kv_model as M  # noqa: E402

F = np.float32
GQ = M.GQ
DAY0 = M.DAY0
FAMILIES = ("ftrl_v2", "adam", "group_radam", "group_adam_v4")
EXACT = ("ftrl_v2", "adam", "group_radam")
OPT_CODE = {"ftrl_v2": 4, "adam": 7, "group_radam": 6, "group_adam_v4": 0}
RTOL, ATOL = 1e-6, 1e-7                     # tests/test_gpu_fuzz.py's bar: GroupAdam V4 against the oracle, exact summed gradient
DIMS = [4, 8, 20, 32, 64, 100]
SIZES, SIZE_P = [0, 1, 7, 300, 2500], [.1, .15, .2, .35, .2]
MAX_IDS, CAP0 = 4096, 16
DRIVERS = ("phase", "single", "multi")      # the phase calls in one process; the whole ops per table; kv_multi_shard_* over A and B
KINDS = ("train", "lookup_only", "peek", "touch", "eval", "eval_between", "delete", "expire", "scatter", "insert", "roundtrip",
         "reserve")
KIND_P = [.22, .06, .08, .10, .08, .08, .10, .05, .07, .06, .05, .05]
LOOKS = ("train", "lookup_only", "peek", "touch", "eval_between")     # the kinds that start with a training lookup
STALE = ("delete", "scatter", "insert")     # the ops of a touch
# the seeds tests/test_gpu_fuzz_sharded.py runs; tests/test_shard_program.py asserts the generator's conditions on exactly these
SEEDS = {"ftrl_v2": [2, 4, 7, 8, 9], "adam": [1, 3, 8, 10], "group_radam": [3, 4, 9, 11], "group_adam_v4": [1, 4, 6, 8]}


def slot_dims(family, D):
  return [3 * D] if family == "group_adam_v4" else M.slot_dims(family, D)


# ---- the model tables: _kv_model.Table, or the oracle behind the same interface -----------------------------------------------
class HostTable(M.Table):
  def keys(self):
    return sorted(self.rows)

  def blacks(self, keys):
    return sum(1 for k in keys if k in self.rows and self.rows[k].black)

  def roundtrip(self, own=None):
    """export (first_n = 6) -> import of the keys in `own` (None: all), as oracle/kv_oracle.cc kvo_export / kvo_import state
    it: a blacklisted key stays blacklisted, a key under the enter threshold or with under_threshold set is not exported,
    every other key keeps its row; frequency words are restored; under_threshold is left false."""
    for k in [k for k in self.rows if own is None or k in own]:
      r = self.rows[k]
      if not r.black and (self.low_freq(r) or r.under):
        del self.rows[k]
        continue
      n = M.Row(np.zeros(self.dim, F) if r.black else r.row, r.freq, r.black)
      n.under = False
      self.rows[k] = n


class OracleTable(object):
  """oracle.kv_oracle.OracleKv behind _kv_model.Table's interface"""

  def __init__(self, dim, init_table, seed=0, day=0, enter_threshold=0):
    from oracle import kv_oracle as ko
    self.o = ko.OracleKv(dim, enter_threshold, init_table, day=day, picker=1, seed=seed)
    self.dim, self.day, self.enter_threshold = int(dim), int(day), int(enter_threshold)

  def set_day(self, day):
    self.day = int(day)
    self.o.set_day(day)

  def gather_or_insert(self, ids, counts=None):
    return self.o.gather_or_insert(np.asarray(ids).reshape(-1), counts)

  def gather_or_zeros(self, keys):
    return self.o.gather_or_zeros(np.asarray(keys).reshape(-1))

  def scatter_update(self, ids, upd, op=0):
    self.o.scatter_update(ids, upd, op)

  def insert(self, ids, vals):
    self.o.insert(ids, vals)

  def delete(self, ids):
    return self.o.delete(ids)

  def delete_with_timestamp(self, threshold):
    return sorted(self.o.delete_with_timestamp(threshold).tolist())

  def get_count(self, keys):
    return self.o.get_count(np.asarray(keys).reshape(-1))

  def get_timestamp(self, keys):
    return self.o.get_timestamp(np.asarray(keys).reshape(-1))

  def size(self):
    return self.o.size()

  def sum_freq(self):
    return self.o.sum_freq()

  def map_size(self):
    return self.o.map_size()

  def meta(self, key):
    return self.o.meta(key)

  def metas(self, keys):
    return [self.o.meta(k) for k in np.asarray(keys).reshape(-1).tolist()]

  def keys(self):
    return sorted(self.o.export(6)[3].tolist())

  def blacks(self, keys):
    return 0                                                 # (GroupAdam V4 runs without regularisers: it blacklists nothing)

  def roundtrip(self, own=None):
    k, v, bl, fk, fv = self.o.export(6)
    if own is None:
      self.o.import_(k, v, bl, fk, fv)
      return
    mk, mb, mf = (np.array([int(x) in own for x in a], bool) for a in (k, bl, fk))
    self.o.delete(fk[mf])                                    # the owner's import clears its table ...
    self.o.import_delta(k[mk], v[mk], bl[mb], fk[mf], fv[mf], (), first_n=6)   # ... and files what its export held


class ModelSet(object):
  """One var and its slot tables on the host."""

  def __init__(self, family, D, thr, vinit, sinits, seed, day=DAY0):
    T = OracleTable if family == "group_adam_v4" else HostTable
    self.family = family
    self.var = T(D, vinit, seed, day, thr)
    self.slots = [T(d, t, seed, day, 0) for d, t in zip(slot_dims(family, D), sinits)]

  @property
  def tables(self):
    return [self.var] + self.slots

  def apply(self, u, s, hp):
    if not len(u):
      return
    if self.family == "group_adam_v4":
      from oracle import kv_oracle as ko
      ko.apply_group_adam(self.var.o, self.slots[0].o, s, u, *hp)
    else:
      M.apply_step(self.family, self.var, self.slots, u, s, hp)


def table_state(t, keys=None):
  """(keys, rows, meta records) of a model table: all of it, or on `keys`"""
  keys = t.keys() if keys is None else [int(k) for k in keys]
  rows = t.gather_or_zeros(np.array(keys, np.int64)) if keys else np.zeros((0, t.dim), F)
  return keys, np.asarray(rows, F), t.metas(keys)


def exact_sum(ids, grad):
  """(sorted unique ids, their summed gradient rows): the sums are exact (the module docstring), so float64 makes them in
  any order; -> also the largest sum of |g| / GQ of a key and element."""
  ids = np.asarray(ids, np.int64).reshape(-1)
  u, inv = np.unique(ids, return_inverse=True)
  s = np.zeros((u.size, grad.shape[1]))
  a = np.zeros((u.size, grad.shape[1]))
  np.add.at(s, inv, grad.astype(np.float64))
  np.add.at(a, inv, np.abs(grad.astype(np.float64)) / GQ)
  out = (s + 0.0).astype(F)
  assert np.array_equal(out.astype(np.float64), s)
  return u, out, float(a.max()) if a.size else 0.0


class ShardProgram(object):
  """A 24-step random program of one family on two table sets, carried on one unsharded model per set (self.sets).  Drawn
  per program: world, owner rule, the two dims (equal in about half the programs), enter threshold, keyspace, deterministic
  mode, lossless (initial capacity CAP0) or lossy (a capacity no segment can exceed).  Every step acts on both sets; a
  touch falls on set A's var of one rank.  self.stats collects what the generator's conditions are asserted on."""
  STEPS = 24

  def __init__(self, family, seed):
    assert family in FAMILIES
    self.family, self.seed = family, int(seed)
    rng = self.rng = np.random.default_rng([FAMILIES.index(family), self.seed, 4242])
    self.world = int(rng.choice([1, 2, 3, 4]))
    self.rule = str(rng.choice(["hash", "mod"]))
    DA = int(rng.choice(DIMS))
    self.same_dim = bool(rng.integers(0, 2))      # the same D: the grouped launches of the multi forms; else the per-table fallback
    self.D = [DA, DA if self.same_dim else int(rng.choice([d for d in DIMS if d != DA]))]
    self.thr = int(rng.choice([0, 0, 2]))
    self.keyspace = ks = int(rng.choice([50, 400, 5000]))
    self.det = bool(rng.integers(0, 2))
    self.lossless = bool(rng.integers(0, 2))
    # lossy: a segment holds at most every distinct id of the largest batch; lossless: small, so raises come when the ids demand
    self.cap0 = CAP0 if self.lossless else min(2 * ks, SIZES[-1]) + 8
    self.cap = [self.cap0, self.cap0]                        # the capacity as kv_shard.hip's rule predicts it (for the conditions only)
    self.branch = str(rng.choice(sorted(M.RADAM_BRANCHES)))
    self.nesterov = bool(rng.integers(0, 2))
    self.universe = np.arange(-ks - 5, ks + 5, dtype=np.int64)
    import torch
    from tfplus_amd.kv_variable.python.ops import sharded
    self.own_univ = sharded.owner_of(torch.from_numpy(self.universe), self.world, self.rule).numpy().astype(np.int64)
    self.inits = []
    for i, D in enumerate(self.D):
      if family == "adam":
        vinit, sinits = rng.uniform(-0.5, 0.5, (32, D)).astype(F), [np.zeros((4, 2 * D), F)]
      elif family == "group_adam_v4":
        vinit, sinits = rng.standard_normal((32, D)).astype(F), [np.zeros((4, 3 * D), F)]
      else:       # rows of two magnitudes, as _kv_model.Program
        vinit = rng.uniform(0.5, 1.0, (32, D)) * 0.05
        vinit[::2] *= 1e-3
        vinit = vinit.astype(F)
        sinits = [np.zeros((4, 5 * D), F)] if family == "group_radam" else [np.full((4, D), 0.1, F), np.zeros((4, D), F)]
      self.inits.append((vinit, sinits, 10 * self.seed + i + 1))
    self.sets = [self.make_set(j) for j in range(2)]
    self.day = DAY0
    self.b1p, self.b2p = F(0.9), F(0.999)
    self.stats = {"kinds": set(), "drivers": set(), "forms": set(), "raises": [], "multi_one_raise": 0, "touch_owned": 0,
                  "black_lookup": 0, "filtered_apply": 0, "applies": 0, "single_owner": 0, "max_abs_sum": 0.0, "max_need": 0}

  def make_set(self, j):
    vinit, sinits, seed = self.inits[j]
    return ModelSet(self.family, self.D[j], self.thr, vinit, sinits, seed)

  def owner(self, ids):
    return self.own_univ[np.asarray(ids, np.int64).reshape(-1) + self.keyspace + 5]

  def owned(self, o):
    return self.universe[self.own_univ == o]

  # ---- pieces ---------------------------------------------------------------------------------------------------------
  def _hp(self, ctxs):
    fam = self.family
    if fam == "ftrl_v2":
      return (0.1, 2e-3, 1e-2, 1e-2, -0.5)
    if fam == "adam":
      return (0.05, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-8)
    if fam == "group_adam_v4":
      return (1e-2, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
    tract, ams = M.RADAM_BRANCHES[self.branch]
    hp0 = (0.1, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-7, 0.0, 1e-2, 0.0, 0.4, tract, ams, self.nesterov)
    # l1 = the median |linear'| over both sets (_kv_model.Program._hp_fn): about half the elements clamped, a row with every
    # element clamped is blacklisted — the blacklist / lifting cycle with no rounding involved
    z = [np.abs(M.linear_norms(fam, c["x"], c["srows"], c["g"], hp0)[1]).reshape(-1) for c in ctxs if c["x"].shape[0]]
    if not z:
      return hp0
    return hp0[:6] + (float(np.median(np.concatenate(z))),) + hp0[7:]

  def _batches(self):
    rng, ks, out = self.rng, self.keyspace, []
    for _ in range(2):
      ids = [rng.integers(-ks, ks, int(rng.choice(SIZES, p=SIZE_P))).astype(np.int64) for _ in range(self.world)]
      if rng.random() < 0.3:                                 # one rank's batch belongs to a single owner
        r, pool = int(rng.integers(0, self.world)), self.owned(int(rng.integers(0, self.world)))
        if ids[r].size:
          ids[r] = pool[rng.integers(0, pool.size, ids[r].size)]
          self.stats["single_owner"] += 1
      out.append(ids)
    return out

  def _need(self, ids):
    """the largest number of distinct ids any (rank, owner) segment holds"""
    need = 0
    for b in ids:
      if b.size:
        need = max(need, int(np.bincount(self.owner(np.unique(b)), minlength=self.world).max()))
    return need

  def _lookup(self, step, driver, train):
    """a lookup of both sets on the model: training (inserted, every occurrence counted) or read-only"""
    rng = self.rng
    L = {"combiner": str(rng.choice(["sum", "mean", "sqrtn"])), "sets": []}
    raised = []
    for j, (ts, ids) in enumerate(zip(self.sets, self._batches())):
      cat = np.concatenate(ids)
      self.stats["black_lookup"] += ts.var.blacks(np.unique(cat).tolist())
      rows = ts.var.gather_or_insert(cat) if train else ts.var.gather_or_zeros(cat)
      rows = np.asarray(rows, F).reshape(cat.size, self.D[j])
      cuts = np.cumsum([b.size for b in ids])[:-1]
      a = {"ids": ids, "rows": np.split(rows, cuts), "sparse": None, "need": self._need(ids), "raise": False}
      if rng.random() < 0.4:                                 # the combining finish: segments of about three positions
        weighted = bool(rng.integers(0, 2))
        nseg = [max(1, b.size // 3) for b in ids]
        a["sparse"] = {"nseg": nseg, "seg": [np.sort(rng.integers(0, m, b.size)).astype(np.int64) for b, m in zip(ids, nseg)],
                       "w": [rng.uniform(0.5, 1.5, b.size).astype(F) if weighted else None for b in ids]}
        self.stats["forms"].add(("sparse" if train else "sparse_zeros", L["combiner"], weighted))
      else:
        self.stats["forms"].add("plain" if train else "zeros")
      self.stats["max_need"] = max(self.stats["max_need"], a["need"])
      if self.lossless:
        if a["need"] > self.cap[j]:
          a["raise"] = True
          self.cap[j] = min(MAX_IDS, a["need"] + a["need"] // 4 + 64)
          self.stats["raises"].append((step, j, driver, train))
          raised.append(j)
      else:
        assert a["need"] <= self.cap0, (a["need"], self.cap0)          # lossy: no segment can overflow
      L["sets"].append(a)
    if driver == "multi" and len(raised) == 1:
      self.stats["multi_one_raise"] += 1
    return L

  def _grads(self, L):
    rng = self.rng
    out = []
    for j, a in enumerate(L["sets"]):
      gs = []
      for b in a["ids"]:
        g = rng.normal(0, 1, (b.size, self.D[j])) * rng.choice([1e-1, 1e-3], (b.size, 1))
        gs.append((np.round(g / GQ) * GQ + 0.0).astype(F))   # (+ 0: no negative zeros)
      out.append(gs)
    return out

  def _apply(self, L, grads, skip):
    """the apply of the batch L on the model: the sum of the concatenated batches; set A without the keys `skip` owns"""
    per = []
    for j, a in enumerate(L["sets"]):
      u, s, big = exact_sum(np.concatenate(a["ids"]), np.concatenate(grads[j]))
      assert big < 2 ** 24, big                              # the exactness bound
      self.stats["max_abs_sum"] = max(self.stats["max_abs_sum"], big)
      if j == 0 and skip is not None:
        keep = self.owner(u) != skip
        u, s = u[keep], s[keep]
      if self.thr and u.size:
        c = self.sets[j].var.get_count(u)
        self.stats["filtered_apply"] += int(np.sum((c > 0) & (c < self.thr)))
      per.append({"grad": grads[j], "u": u, "s": s})
    if self.family == "group_adam_v4":
      hp = self._hp(None)
      for ts, p in zip(self.sets, per):
        ts.apply(p["u"], p["s"], hp)
    else:       # both sets are resolved first: the scalars (one set for A and B) are placed by the rows both start from
      ctxs = [M.resolve_step(self.family, ts.var, ts.slots, p["u"], p["s"]) for ts, p in zip(self.sets, per)]
      hp = self._hp(ctxs)
      for ts, ctx in zip(self.sets, ctxs):
        M.finish_step(self.family, ts.var, ts.slots, ctx, hp)
    self.stats["applies"] += 1
    if self.family != "ftrl_v2":
      self.b1p, self.b2p = F(self.b1p * F(0.9)), F(self.b2p * F(0.999))
    return {"hp": hp, "sets": per, "skip": skip}

  def _touch(self, L):
    """one rank's var of set A gets a mutating op between the lookup and the apply"""
    rng = self.rng
    t = int(rng.integers(0, self.world))
    batch = np.unique(np.concatenate(L["sets"][0]["ids"]))
    mine = batch[self.owner(batch) == t] if batch.size else batch
    self.stats["touch_owned"] += int(mine.size > 0)
    pool = self.owned(t)
    ids = pool[rng.integers(0, pool.size, int(rng.integers(1, 40)))]
    if mine.size:
      ids = np.concatenate([ids, mine[rng.integers(0, mine.size, int(rng.integers(1, 20)))]])
    ids = np.unique(ids)
    b = {"kind": "touch", "rank": t, "op": str(rng.choice(STALE)), "ids": ids}
    var = self.sets[0].var
    if b["op"] == "delete":
      var.delete(ids)
    elif b["op"] == "scatter":
      b["upd"], b["which"] = rng.uniform(0.5, 2.0, (ids.size, self.D[0])).astype(F), int(rng.integers(0, 7))
      var.scatter_update(ids, b["upd"], b["which"])
    else:
      b["vals"] = rng.standard_normal((ids.size, self.D[0])).astype(F)
      var.insert(ids, b["vals"])
    return b

  def _owner_op(self, kind, st):
    rng, ks = self.rng, self.keyspace
    if kind == "expire":
      self.day += int(rng.integers(1, 5))
      st["day"], st["thr_days"] = self.day, int(rng.integers(2, 8))
      for ts in self.sets:
        for t in ts.tables:
          t.set_day(self.day)
        st["sets"].append({"gone": ts.var.delete_with_timestamp(st["thr_days"])})
      return
    for j, ts in enumerate(self.sets):
      ids = rng.integers(-ks, ks, int(rng.choice([1, 7, 300]))).astype(np.int64)
      a = {"ids": ids}
      if kind == "scatter":
        a["ids"] = np.unique(ids)
        a["upd"], a["which"] = rng.uniform(0.5, 2.0, (a["ids"].size, self.D[j])).astype(F), int(rng.integers(0, 7))
        ts.var.scatter_update(a["ids"], a["upd"], a["which"])
      elif kind == "insert":
        a["ids"] = np.unique(ids)
        a["vals"] = rng.standard_normal((a["ids"].size, self.D[j])).astype(F)
        ts.var.insert(a["ids"], a["vals"])
      elif kind == "delete":                                 # a random non-empty subset of {var, slots}
        nt = len(ts.tables)
        mask = int(rng.integers(1, 1 << nt))
        a["tables"] = [i for i in range(nt) if mask >> i & 1]
        a["gone"] = [ts.tables[i].delete(ids) for i in a["tables"]]
      elif kind == "roundtrip":                              # export -> import of one owner's var
        a["owner"] = int(rng.integers(0, self.world))
        ts.var.roundtrip(set(self.owned(a["owner"]).tolist()))
      else:                                                  # reserve: one owner's var re-sized; no state changes
        a["owner"], a["capacity"] = int(rng.integers(0, self.world)), int(rng.choice([1000, 20000]))
      st["sets"].append(a)

  # ---- the program ----------------------------------------------------------------------------------------------------
  def steps(self):
    rng = self.rng
    for step in range(self.STEPS):
      kind = "train" if step == 0 else str(rng.choice(KINDS, p=KIND_P))
      self.stats["kinds"].add(kind)
      st = {"step": step, "kind": kind, "driver": None, "sets": [], "lookup": None, "between": None, "apply": None, "read": None}
      if kind in LOOKS or kind == "eval":
        st["driver"] = str(rng.choice(DRIVERS))
        self.stats["drivers"].add((kind, st["driver"]))
      if kind == "eval":
        st["read"] = self._lookup(step, st["driver"], False)
      elif kind in LOOKS:
        L = st["lookup"] = self._lookup(step, st["driver"], True)
        if kind != "lookup_only":
          grads = self._grads(L)
          skip = None
          if kind == "peek":
            st["between"] = {"kind": "peek"}
          elif kind == "touch":
            st["between"] = self._touch(L)
            skip = st["between"]["rank"]
          elif kind == "eval_between":                       # the read-only lookup voids the batch: every apply is refused
            st["between"] = {"kind": "eval", "driver": str(rng.choice(DRIVERS))}
            st["read"] = self._lookup(step, st["between"]["driver"], False)
          if kind == "eval_between":
            st["apply"] = {"hp": self._hp_refused(), "sets": [{"grad": g} for g in grads], "skip": None, "refused": True}
          else:
            st["apply"] = self._apply(L, grads, skip)
            st["apply"]["refused"] = False
      else:
        self._owner_op(kind, st)
      last = step == self.STEPS - 1
      st["check"] = [self.universe if (last or self.keyspace <= 400) else
                     rng.integers(-self.keyspace - 5, self.keyspace + 5, 200).astype(np.int64) for _ in self.sets]
      yield st

  def _hp_refused(self):
    """scalars for an apply that must be refused before it reads them"""
    if self.family == "group_radam":
      tract, ams = M.RADAM_BRANCHES[self.branch]
      return (0.1, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-7, 0.0, 1e-2, 0.0, 0.4, tract, ams, self.nesterov)
    return self._hp(None)


class ShardedModel(object):
  """`world` ModelSets per table set, one per owner, fed what the owners are fed."""

  def __init__(self, prog):
    self.p = prog
    self.sets = [[prog.make_set(j) for _ in range(prog.world)] for j in range(2)]

  def _lookup(self, L):
    p = self.p
    for parts, a in zip(self.sets, L["sets"]):
      recs = []
      for b in a["ids"]:                                     # per sending rank: its distinct ids as (id, count) records
        u, c = np.unique(b, return_counts=True)
        recs.append((u, c, p.owner(u)))
      for o, part in enumerate(parts):
        for u, c, own in recs:                               # the owner serves the segments in rank order
          m = own == o
          if m.any():
            part.var.gather_or_insert(u[m], c[m])

  def take(self, st):
    p, kind = self.p, st["kind"]
    if st["lookup"] is not None:
      self._lookup(st["lookup"])
    b = st["between"]
    if b is not None and b["kind"] == "touch":
      var = self.sets[0][b["rank"]].var
      if b["op"] == "delete":
        var.delete(b["ids"])
      elif b["op"] == "scatter":
        var.scatter_update(b["ids"], b["upd"], b["which"])
      else:
        var.insert(b["ids"], b["vals"])
    ap = st["apply"]
    if ap is not None and not ap["refused"]:
      for j, (parts, a) in enumerate(zip(self.sets, ap["sets"])):
        own = p.owner(a["u"])
        for o, part in enumerate(parts):
          m = own == o
          part.apply(a["u"][m], a["s"][m], ap["hp"])
    if kind == "expire":
      gone = []
      for parts, a in zip(self.sets, st["sets"]):
        g = []
        for part in parts:
          for t in part.tables:
            t.set_day(st["day"])
          g += part.var.delete_with_timestamp(st["thr_days"])
        gone.append(sorted(g))
      return gone
    if kind in ("scatter", "insert", "delete", "roundtrip"):
      gone = []
      for parts, a in zip(self.sets, st["sets"]):
        if kind == "roundtrip":
          parts[a["owner"]].var.roundtrip()
          continue
        own = p.owner(a["ids"])
        g = [0] * len(a.get("tables", ()))
        for o, part in enumerate(parts):
          m = own == o
          if not m.any():
            continue
          if kind == "scatter":
            part.var.scatter_update(a["ids"][m], a["upd"][m], a["which"])
          elif kind == "insert":
            part.var.insert(a["ids"][m], a["vals"][m])
          else:
            for i, ti in enumerate(a["tables"]):
              g[i] += part.tables[ti].delete(a["ids"][m])
        gone.append(g)
      return gone
    return None
