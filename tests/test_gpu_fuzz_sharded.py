"""Stateful random-program test of the SHARDED tables (kv_shard.hip, kv_route.h) against one unsharded host model.

A 24-step program (tests/_shard_program.py ShardProgram) runs on `world` shards of two table sets A and B — a var and its slot
tables each, every shard with the same seed, init table and clock — and on ONE unsharded model per set, which carries the
whole state by itself: nothing the device says is fed back.  The steps: training lookups (plain, or sparse with a combiner
and weights) and their applies, driven by the phase calls in one process (lookup_route / kv_shard_agree_local /
kv_shard_exchange_local / lookup_serve / lookup_finish[_sparse] / apply_route / apply_serve), by the whole ops with ranks as
threads over KvCommStaged, or by kv_multi_shard_* over A and B in one call; lookups nobody applies; harmless reads on the
owners between a lookup and its apply (the apply must still take the lookup's index); a mutating op on one rank's var in
between (that rank's apply is refused — "another op used the table" — with all its exchanges queued, the others apply, the
model applies the keys the touched rank does not own); read-only lookups, alone (nothing changes) and between a lookup and
its apply (every form of the apply is refused on every rank, nothing is exchanged); and owner-side deletes, expiries,
scatters, inserts, export -> import round trips and reserves.

After every step, on every owner's var and slot tables: the key set is the model's keys that owner_of gives that rank; map
size, size and frequency sum add up to the model's; on 200 sampled keys (the whole universe when it is small, and always
after the last step) rows, counts, time stamps and the kv_get_meta records.  The rows every lookup returned to every rank
are compared too.  In lossless programs the capacity is raised exactly at the lookups whose largest (rank, owner) segment
exceeds it, to one value >= that need on all ranks; lossy programs cannot overflow (tests/test_shard_program.py).

Gradients lie on a grid that any summation order adds exactly, so ftrl_v2, adam and group_radam (l21 = 0) hold BIT FOR BIT,
and GroupAdam V4 — carried by the oracle — at tests/test_gpu_fuzz.py's bar for this op with an exact summed gradient
(rtol 1e-6, atol 1e-7).  tests/test_shard_program.py holds the premise (the owners' tables together are the unsharded table)
and the generator's conditions on the host for exactly these seeds.

Worst observed / allowed for GroupAdam V4 on an MI355X over its four seeds: 0 — with an exact summed gradient the shards' rows
are the oracle's bit for bit.

What the programs found is kept reduced at the end of the file: an import left under_threshold neither evaluated nor marked
stale, so the next lookup did not evaluate it (kv_kernels.h, MODE_MARK / the import's scatter); and kv_shard_apply_route
answered a rank whose voided training batch was empty with an argument error instead of the documented refusal.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _shard_program as SP  # noqa: E402
import _sparse_zeros_ref as SZ  # noqa: E402
from _ranks import Ranks  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _lib():
  from tfplus_amd import _lib as L
  return L


def _np(t):
  return t.detach().cpu().numpy()


class Run(object):
  """One program on the shards next to its model."""

  def __init__(self, ops, family, seed):
    self.ops, self.prog = ops, SP.ShardProgram(family, seed)
    p = self.prog
    rule = {"hash": ops.KV_OWNER_HASH, "mod": ops.KV_OWNER_MOD}[p.rule]
    self.tabs, self.shards = [], []                          # [set][rank] -> [var, slot ...] / KvShard
    for j, (vinit, sinits, tseed) in enumerate(p.inits):
      dims = [p.D[j]] + SP.slot_dims(family, p.D[j])
      tabs, shards = [], []
      for r in range(p.world):
        hs = []
        for i, (d, init) in enumerate(zip(dims, [vinit] + sinits)):
          h = ops.kv_variable([d], enter_threshold=p.thr if i == 0 else 0, capacity_hint=64)     # tiny hint: growth
          ops.kv_set_seed(h, tseed); ops.init_kv_variable_v2(h, init); ops.kv_set_clock_days(h, SP.DAY0)
          if p.det:
            ops.kv_set_deterministic(h, 1)
          hs.append(h)
        sh = ops.KvShard(hs[0], p.world, r, rule, max_ids=SP.MAX_IDS, peer_capacity=p.cap0)
        sh.set_lossless(p.lossless)
        tabs.append(hs); shards.append(sh)
      self.tabs.append(tabs); self.shards.append(shards)
    self.ranks = Ranks(ops, p.world)
    self.code = SP.OPT_CODE[family]
    self.exact = family in SP.EXACT
    self.worst = 0.0

  def close(self):
    """everything the run made is destroyed here, in one order, on this thread: the shards, the communicators, the tables —
    nothing of it is left to the cyclic collector (tests/_ranks.py)"""
    torch.cuda.synchronize()
    self.shards = None
    self.ranks.close()
    self.tabs = None

  @staticmethod
  def dev(ids):
    return torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda()

  # ---- comparisons ----------------------------------------------------------------------------------------------------
  def same_rows(self, got, want, tag):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if self.exact:
      assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, np.argwhere(got != want)[:5])
      return
    err = np.abs(got.astype(np.float64) - want)
    tol = SP.ATOL + SP.RTOL * np.abs(want.astype(np.float64))
    bad = ~(err <= tol)                                      # (a NaN is over any allowance)
    assert not bad.any(), (tag, np.argwhere(bad)[:5], err[bad][:5], tol[bad][:5])
    if err.size:
      self.worst = max(self.worst, float((err / tol).max()))

  def same_out(self, got, a, r, comb, tag):
    sp = a["sparse"]
    if sp is None:
      return self.same_rows(got, a["rows"][r], tag)
    # the combine of the model's rows in float32 position order (kvhip.h kv_lookup_sparse_zeros): its float64 value and the
    # sequential-summation bound of tests/_sparse_zeros_ref.py; the oracle-carried family adds what its rows are allowed
    # (an empty batch has no weights to point at — weights == NULL — so its segments follow the unweighted empty-segment
    #  rule, zero rows: kvhip.h kv_lookup_sparse_zeros, "n == 0 with num_segments > 0")
    w = sp["w"][r] if a["ids"][r].size else None
    want, tol = SZ.combine(a["rows"][r], sp["seg"][r], w, sp["nseg"][r], comb)
    if not self.exact:
      allow = SP.ATOL + SP.RTOL * np.abs(a["rows"][r].astype(np.float64))
      tol = tol + np.nan_to_num(SZ.combine(allow, sp["seg"][r], w, sp["nseg"][r], comb)[0])
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    SZ.check(got, want, tol, tag)

  def export(self, h):
    k, v, bl, fk, fv = self.ops.kv_variable_export(h, first_n=6)
    o, fo = torch.argsort(k), torch.argsort(fk)
    return (_np(k[o]).tobytes(), _np(v[o]).tobytes(), np.sort(_np(bl)).tobytes(), _np(fk[fo]).tobytes(), _np(fv[fo]).tobytes())

  def snapshot(self):
    ops = self.ops
    torch.cuda.synchronize()
    return [[[(self.export(h), ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h))
              for h in hs] for hs in tabs] for tabs in self.tabs]

  def check(self, st, tag):
    ops, p = self.ops, self.prog
    for j, (tabs, ts, keys) in enumerate(zip(self.tabs, p.sets, st["check"])):
      keys = np.unique(keys)
      kown = p.owner(keys)
      for i, m in enumerate(ts.tables):
        t = "%s set %d table %d" % (tag, j, i)
        mkeys = np.array(m.keys(), np.int64)
        mown = p.owner(mkeys) if mkeys.size else mkeys
        figs = [0, 0, 0]
        for r in range(p.world):
          h = tabs[r][i]
          held = np.sort(_np(ops.kv_variable_export(h, first_n=6)[3]))
          assert np.array_equal(held, mkeys[mown == r]), (t, r, held.size, int(np.sum(mown == r)))
          for f, v in enumerate((ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h))):
            figs[f] += int(v)
          mine = keys[kown == r]
          if not mine.size:
            continue
          self.same_rows(_np(ops.kv_variable_gather_or_zeros_v2(h, mine)), m.gather_or_zeros(mine), t + " rank %d" % r)
          assert np.array_equal(_np(ops.kv_variable_get_count_v2(h, mine)), m.get_count(mine)), (t, r)
          assert np.array_equal(_np(ops.kv_variable_get_time_stamp(h, mine)), m.get_timestamp(mine)), (t, r)
          got, want = ops.kv_get_meta(h, mine), m.metas(mine)
          assert got == want, (t, r, [(int(k), g, w) for k, g, w in zip(mine, got, want) if g != w][:5])
        assert tuple(figs) == (m.map_size(), m.size(), m.sum_freq()), (t, figs)

  # ---- lookups --------------------------------------------------------------------------------------------------------
  def phase_lookup(self, j, ids, sp, comb, ro):
    ops, shs = self.ops, self.shards[j]

    def route():
      for sh, t in zip(shs, ids):
        sh.lookup_route(t)
    route()
    if self.prog.lossless and ops.kv_shard_agree_local(shs):
      route()                                                # the capacity was raised on all of them
    ops.kv_shard_exchange_local(shs, 0)
    for sh in shs:
      sh.lookup_serve_zeros() if ro else sh.lookup_serve()
    ops.kv_shard_exchange_local(shs, 1)
    outs = []
    for r, sh in enumerate(shs):
      o = sh.lookup_finish() if sp is None else sh.lookup_finish_sparse(sp["seg"][r], sp["w"][r], sp["nseg"][r], comb)
      outs.append(_np(o))
    return outs

  def lookup(self, L, driver, ro, tag):
    ops, p, W, comb = self.ops, self.prog, self.prog.world, L["combiner"]
    before = [self.shards[j][0].peer_capacity for j in range(2)]
    ids = [[self.dev(b) for b in a["ids"]] for a in L["sets"]]
    sp = [a["sparse"] for a in L["sets"]]
    if driver == "phase":
      outs = [self.phase_lookup(j, ids[j], sp[j], comb, ro) for j in range(2)]
    elif driver == "single":
      outs = []
      for j in range(2):
        def one(r, comm, j=j):
          sh = self.shards[j][r]
          if sp[j] is None:
            return _np((sh.lookup_zeros if ro else sh.lookup)(comm, ids[j][r]))
          fn = sh.lookup_sparse_zeros if ro else sh.lookup_sparse
          return _np(fn(comm, ids[j][r], sp[j]["seg"][r], sp[j]["w"][r], sp[j]["nseg"][r], comb))
        outs.append(self.ranks.run(one))
    else:
      def both(r, comm):
        shs, ii = [self.shards[j][r] for j in range(2)], [ids[j][r] for j in range(2)]
        if sp[0] is None and sp[1] is None:
          o = (ops.kv_multi_shard_lookup_zeros if ro else ops.kv_multi_shard_lookup)(shs, comm, ii)
        else:
          fn = ops.kv_multi_shard_lookup_sparse_zeros if ro else ops.kv_multi_shard_lookup_sparse
          o = fn(shs, comm, ii, [None if s is None else s["seg"][r] for s in sp], [None if s is None else s["w"][r] for s in sp],
                 [0 if s is None else s["nseg"][r] for s in sp], comb)
        return [_np(x) for x in o]
      res = self.ranks.run(both)
      outs = [[res[r][j] for r in range(W)] for j in range(2)]
    for j, a in enumerate(L["sets"]):
      for r in range(W):
        self.same_out(outs[j][r], a, r, comb, "%s set %d rank %d" % (tag, j, r))
      caps = {sh.peer_capacity for sh in self.shards[j]}
      assert len(caps) == 1, (tag, j, caps)                  # all ranks agree
      after = caps.pop()
      if p.lossless:       # raised exactly where the largest (rank, owner) segment exceeds the capacity, to at least that
        assert (after != before[j]) == (a["need"] > before[j]) and after >= a["need"], (tag, j, before[j], after, a["need"])
        # ... which is where the generator said it would be: the conditions tests/test_shard_program.py asserts on the
        # predicted raises (a late one, one by a read-only lookup, one table of a multi call) hold for the device too
        assert (after != before[j]) == a["raise"], (tag, j, before[j], after, a["need"])
      else:
        assert after == before[j] == p.cap0, (tag, j)

  # ---- applies --------------------------------------------------------------------------------------------------------
  def apply(self, ap, driver, touched, tag):
    ops, p, W, L = self.ops, self.prog, self.prog.world, _lib()
    hp = [float(v) for v in ap["hp"]]
    g = [[torch.from_numpy(x).cuda() for x in a["grad"]] for a in ap["sets"]]
    slots = lambda j, r: self.tabs[j][r][1:]
    if driver == "phase":
      for j in range(2):
        shs = self.shards[j]
        for r in range(W):
          shs[r].apply_route(g[j][r])
        ops.kv_shard_exchange_local(shs, 1)
        for r in range(W):
          if j == 0 and r == touched:                        # refused before anything is queued
            with pytest.raises(L.FailedPreconditionError, match="another op used"):
              shs[r].apply_serve(self.code, slots(j, r), hp)
          else:
            shs[r].apply_serve(self.code, slots(j, r), hp)
      return

    def guarded(r, call):
      """the touched rank's apply is refused once all its exchanges are queued: the barrier is never broken"""
      try:
        call()
      except L.FailedPreconditionError as e:
        if r != touched or "another op used" not in str(e):
          raise
        return "refused"
      return "applied"
    if driver == "single":
      for j in range(2):
        res = self.ranks.run(lambda r, comm, j=j: guarded(
            r if j == 0 else -1, lambda: self.shards[j][r].apply(comm, self.code, slots(j, r), g[j][r], hp)))
        assert res == ["refused" if (j == 0 and r == touched) else "applied" for r in range(W)], (tag, j, res)
    else:
      res = self.ranks.run(lambda r, comm: guarded(r, lambda: ops.kv_multi_shard_apply(
          [self.shards[j][r] for j in range(2)], comm, self.code, [slots(j, r) for j in range(2)], [g[j][r] for j in range(2)], hp)))
      assert res == ["refused" if r == touched else "applied" for r in range(W)], (tag, res)

  def refused(self, ap, tag):
    """behind a read-only lookup every form of the apply is refused on every rank, and nothing is exchanged"""
    ops, W, L = self.ops, self.prog.world, _lib()
    hp = [float(v) for v in ap["hp"]]
    g = [[torch.from_numpy(x).cuda() for x in a["grad"]] for a in ap["sets"]]
    torch.cuda.synchronize()
    exchanges = [c.exchanges for c in self.ranks.comms]
    for r in range(W):
      comm = self.ranks.comms[r]
      for j in range(2):
        sh, sl = self.shards[j][r], self.tabs[j][r][1:]
        with pytest.raises(L.FailedPreconditionError, match="read-only"):
          sh.apply(comm, self.code, sl, g[j][r], hp)
        with pytest.raises(L.FailedPreconditionError, match="read-only"):
          sh.apply_route(g[j][r])
        with pytest.raises(L.FailedPreconditionError, match="read-only"):
          ops.kv_multi_shard_apply([sh], comm, self.code, [sl], [g[j][r]], hp)
        with pytest.raises(L.FailedPreconditionError):
          sh.apply_serve(self.code, sl, hp)                  # (the serve token is void)
      with pytest.raises(L.FailedPreconditionError, match="read-only"):
        ops.kv_multi_shard_apply([self.shards[j][r] for j in range(2)], comm, self.code, [self.tabs[j][r][1:] for j in range(2)],
                                 [g[j][r] for j in range(2)], hp)
    torch.cuda.synchronize()
    assert [c.exchanges for c in self.ranks.comms] == exchanges, tag

  # ---- the ops on the owners ------------------------------------------------------------------------------------------------
  def scatter(self, h, ids, upd, which):
    ops = self.ops
    [ops.kv_variable_scatter_update_v2, ops.kv_variable_scatter_add_v2, ops.kv_variable_scatter_sub_v2,
     ops.kv_variable_scatter_mul_v2, ops.kv_variable_scatter_div_v2, ops.kv_variable_scatter_min_v2,
     ops.kv_variable_scatter_max_v2][which](h, ids, upd)

  def between(self, st, tag):
    ops, p, b = self.ops, self.prog, st["between"]
    if b["kind"] == "peek":       # reads on every owner's var: the pending pass is settled, the lookup's index stays
      for j in range(2):
        keys = np.unique(st["check"][j])[:200]
        for r in range(p.world):
          h = self.tabs[j][r][0]
          ops.kv_variable_gather_or_zeros_v2(h, keys); ops.kv_variable_get_count_v2(h, keys); ops.kv_get_meta(h, keys)
    elif b["kind"] == "touch":    # a mutating op on one rank's var of set A (SP.STALE: each drops the table's batch index)
      h = self.tabs[0][b["rank"]][0]
      if b["op"] == "delete":
        ops.kv_variable_delete(h, b["ids"])
      elif b["op"] == "scatter":
        self.scatter(h, b["ids"], b["upd"], b["which"])
      else:
        ops.kv_variable_insert_v2(h, b["ids"], b["vals"])
    else:                         # a read-only lookup: it voids the batch
      self.lookup(st["read"], b["driver"], True, tag + " read-only in between")

  def owner_op(self, st, tag):
    ops, p, kind = self.ops, self.prog, st["kind"]
    for j, (tabs, a) in enumerate(zip(self.tabs, st["sets"])):
      if kind == "expire":
        gone = []
        for hs in tabs:
          for h in hs:
            ops.kv_set_clock_days(h, st["day"])
          gone += _np(ops.kv_variable_delete_with_timestamp(hs[0], st["thr_days"])).tolist()
        assert sorted(gone) == a["gone"], (tag, j)           # the union of what the owners removed is what the model removed
        continue
      if kind in ("roundtrip", "reserve"):
        h = tabs[a["owner"]][0]
        if kind == "reserve":
          ops.kv_reserve(h, a["capacity"])
        else:
          k, v, bl, fk, fv = ops.kv_variable_export(h, first_n=6)
          ops.kv_variable_import(h, k, v, bl, fk, fv)
        continue
      own = p.owner(a["ids"])
      gone = [0] * len(a.get("tables", ()))
      for r, hs in enumerate(tabs):                          # each op is routed to the owners
        m = own == r
        if not m.any():
          continue
        if kind == "scatter":
          self.scatter(hs[0], a["ids"][m], a["upd"][m], a["which"])
        elif kind == "insert":
          ops.kv_variable_insert_v2(hs[0], a["ids"][m], a["vals"][m])
        else:
          for i, ti in enumerate(a["tables"]):
            gone[i] += ops.kv_variable_delete(hs[ti], a["ids"][m])
      if kind == "delete":
        assert gone == a["gone"], (tag, j)

  # ---- one step -------------------------------------------------------------------------------------------------------
  def step(self, st):
    p, kind = self.prog, st["kind"]
    tag = "%s seed %d step %d %s %s world %d %s D=%s" % (p.family, p.seed, st["step"], kind, st["driver"], p.world, p.rule, p.D)
    if kind == "eval":
      before = self.snapshot()
      self.lookup(st["read"], st["driver"], True, tag)
      assert self.snapshot() == before, tag                  # every table's exported state is unchanged
    elif kind in SP.LOOKS:
      self.lookup(st["lookup"], st["driver"], False, tag)
      if st["between"] is not None:
        self.between(st, tag)
      ap = st["apply"]
      if ap is not None and ap["refused"]:
        self.refused(ap, tag)
      elif ap is not None:
        self.apply(ap, st["driver"], ap["skip"], tag)
    else:
      self.owner_op(st, tag)
    self.check(st, tag)


def _run(ops, family, seed, steps=None):
  run = Run(ops, family, seed)
  try:
    for st in run.prog.steps():
      if steps is not None and st["step"] >= steps:
        break
      run.step(st)
    torch.cuda.synchronize()
  finally:
    run.close()
  return run


CASES = [(f, s) for f in SP.FAMILIES for s in SP.SEEDS[f]]


@pytest.mark.parametrize("family,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_random_sharded_program_matches_one_model(ops, family, seed):
  run = _run(ops, family, seed)
  assert run.prog.stats["applies"] > 0
  if not run.exact:
    print("%s seed %d: worst observed / allowed %.3g" % (family, seed, run.worst))
    assert run.worst <= 1.0


# ---- what the programs found, reduced ------------------------------------------------------------------------------------------
def _plain_shards(ops, world, D, table, rule="mod"):
  vars_, slots, shards = [], [], []
  for r in range(world):
    var, slot = ops.kv_variable([D]), ops.kv_variable([3 * D])
    for h, t in ((var, table), (slot, np.zeros((4, 3 * D), F))):
      ops.kv_set_seed(h, 3); ops.init_kv_variable_v2(h, t); ops.kv_set_clock_days(h, SP.DAY0)
    vars_.append(var); slots.append(slot)
    shards.append(ops.KvShard(var, world, r, {"hash": ops.KV_OWNER_HASH, "mod": ops.KV_OWNER_MOD}[rule], max_ids=1024, peer_capacity=64))
  return vars_, slots, shards


def _phases(ops, shards, batches, read_only=False):
  for sh, b in zip(shards, batches):
    sh.lookup_route(Run.dev(b))
  ops.kv_shard_exchange_local(shards, 0)
  for sh in shards:
    sh.lookup_serve_zeros() if read_only else sh.lookup_serve()
  ops.kv_shard_exchange_local(shards, 1)
  return [_np(sh.lookup_finish()) for sh in shards]


def test_the_lookup_after_an_import_evaluates_under_threshold(ops):
  """ftrl_v2 seed 4, reduced (train, round trip of one owner's var, lookup): ImportValues leaves under_threshold unevaluated
  (false), and the next lookup that finds the key evaluates it (find_func: UpdateUnderThreshold) — true for a row of zeros
  and for a blacklisted key.  The import left the flag neither evaluated nor marked stale, so the lookup kept it false."""
  from oracle import kv_oracle as ko
  world, D = 2, 8
  rng = np.random.default_rng(5)
  table = rng.standard_normal((8, D)).astype(F)
  keys, black = np.arange(0, 12, dtype=np.int64), np.arange(20, 24, dtype=np.int64)
  vals = rng.standard_normal((keys.size, D)).astype(F)
  vals[::3] = 0.0                                                 # rows of zeros: under the cutoff once somebody looks
  fk = np.concatenate([keys, black])
  fv = np.full(fk.size, (SP.DAY0 << 16) | 3, np.uint32)
  vars_, slots, shards = _plain_shards(ops, world, D, table)
  for r, var in enumerate(vars_):                                 # every owner imports what it owns ("mod": id % world)
    ops.kv_variable_import(var, keys[keys % world == r], vals[keys % world == r], black[black % world == r], fk[fk % world == r],
                           fv[fk % world == r])
  ref = ko.OracleKv(D, 0, table, day=SP.DAY0, picker=1, seed=3)
  ref.import_(keys, vals, black, fk, fv)
  metas = lambda: [ops.kv_get_meta(vars_[int(k) % world], [int(k)])[0] for k in fk]
  assert metas() == [ref.meta(int(k)) for k in fk]
  assert not any(m["under_threshold"] for m in metas())
  batches = [fk[::2], np.concatenate([fk[1::2], fk[:5]])]
  got = _phases(ops, shards, batches)
  want = ref.gather_or_insert(np.concatenate(batches))
  assert np.array_equal(np.concatenate(got).view(np.uint32), want.view(np.uint32))
  assert metas() == [ref.meta(int(k)) for k in fk]
  assert sum(m["under_threshold"] for m in metas()) == 4 + black.size


def test_the_apply_of_an_empty_batch_behind_a_read_only_lookup_is_refused_as_documented(ops):
  """ftrl_v2 seed 2, reduced: a rank whose training batch was empty has no gradient to name; behind a read-only lookup its
  kv_shard_apply_route must still be the documented refusal (KV_FAILED_PRECONDITION on every rank alike), not an argument error
  about the gradient of the read-only batch."""
  L = _lib()
  world, D = 2, 8
  table = np.random.default_rng(6).standard_normal((8, D)).astype(F)
  vars_, slots, shards = _plain_shards(ops, world, D, table)
  ids = np.arange(0, 40, dtype=np.int64)
  _phases(ops, shards, [ids, ids[:0]])                            # rank 1's training batch is empty
  _phases(ops, shards, [ids[:7], ids[5:30]], read_only=True)      # ... its read-only batch is not
  hp = [0.1, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0]
  for r, n in ((0, ids.size), (1, 0)):
    with pytest.raises(L.FailedPreconditionError, match="read-only"):
      shards[r].apply_route(torch.zeros((n, D), device="cuda"))
    with pytest.raises(L.FailedPreconditionError):
      shards[r].apply_serve(ops.OPT_GROUP_ADAM_V4, [slots[r]], hp)
