"""The cases of tests/test_gpu_capture_replay.py: a captured training step replayed on FRESH ids, with keys the replay has to
insert, repeated ids, state changed between replays, and the host's bounds afterwards (tests/test_capture_cases.py holds
this file's conditions on the CPU; nothing here asks a device for anything).

A replay runs no host code: what the host decided at the capture travels into every replay by value.  So
the reference of R replays is the captured step, WITH THE SCALARS OF ITS CAPTURE, applied to batch 0, 1, ... R - 1 in order
with the state carried — on oracle.kv_oracle for _row_geometry.ORACLE_FAMILIES, on tests/_kv_model.py for the other four.

  replay_batches(seeds)   one _row_geometry.draw_batch per seed (2 172 ids over 144 keys: just over one tile, every branch of the
                          apply kernels), the key sets pairwise disjoint, each with the `pre` lookup that inserts half of its
                          keys before the capture: with enter_threshold = ENTER a replay meets present keys, new keys and keys
                          below the threshold.
  new_keys(...)           by the rules of the ops alone, how many keys a step on a batch inserts into the var and into a slot
                          table; room(...) the max_new_ids of kv_prepare_capture from it.
  trajectory(...)         the reference: per table the warm-up step (eager, outside the capture, on a batch of its own) and
                          the R replays.  The scalars are fixed before the first step, as a capture fixes them: the group
                          families' lasso threshold by _kv_model.lasso_threshold (the rule of _row_geometry) over the norms of
                          ALL the steps — the batches are disjoint, so no step's rows depend on another step's, and the norms
                          do not depend on the threshold: one run with the threshold at zero shows them all.
  bounds_case(), refusal_case()   the sizes of the two cases about the host's bounds, from the growth chunk the sources state.

Bars (none of them new).  Ids, lookup output rows, frequency words, flags, time stamps and the three counters: exact.  Rows:
plain Adam, FTRL-V2 bit for bit (tests/test_gpu_fuzz_optimizers.py); group FTRL-V2 and group RAdam within the allowance the
model carries (_kv_model.step_allowance); the oracle's families rtol RTOL with the family's ATOL, a var that went through a
group norm (RTOL / scale) |x| + atol against the float32 reference or, failing that, max(bar, 4 x the reference's own
error) against the step in float64 (tests/_row_geometry.py, whose arithmetic this file calls).  Rows whose scale is within
SKIP_BELOW of the threshold would not be compared: tests/test_capture_cases.py asserts there is none.
"""
import os
import re

import numpy as np

import _kv_model as M
import _row_geometry as G

F = np.float32
R = 4                                   # replays of cases 1, 2 and 5
DIMS = (7, 32, 512)                     # entry-list pipeline with scalar rows and with float4 rows; the sorted-position pipeline
TABLES = 3                              # tables of the batched forms
SEEDS = tuple(range(41, 41 + TABLES * (R + 1)))      # table i: SEEDS[i (R + 1)] the warm-up's batch, then its R replays'
SHAPES = ("tok", "plain", "apply", "unique")
# the captured step: "tok" the training lookup and the apply of the very same ids tensor (bench.py's step); "plain" the
# lookup and an apply that is handed no token; "apply" the apply alone (it inserts the keys itself); "unique" the _unique op
# alone on the batch's distinct keys and their summed gradient rows
CASE1 = [(f, 32, s) for f in G.FAMILIES for s in SHAPES] + \
        [(f, D, s) for f in ("group_adam_v4", "ftrl_v2", "adam") for D in (7, 512) for s in SHAPES]
CASE5 = ("group_adam_v4", "ftrl_v2")

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tfplus_amd", "csrc")


def growth_chunk():
  """Rows of one slab chunk of a table created without capacity_hint, as kv_host.h and kvhip.hip state it."""
  with open(os.path.join(CSRC, "kv_host.h")) as f:
    bits = re.findall(r"\n  int chunk_bits = (\d+);", f.read())
  with open(os.path.join(CSRC, "kvhip.hip")) as f:
    src = f.read()
  assert len(bits) == 1 and "t->chunk_bits = std::max(%s, " % bits[0] in src, bits
  assert "const size_t R = (size_t)1 << t->chunk_bits;" in src
  return 1 << int(bits[0])


# ---- batches -----------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def replay_batches(seeds):
  """-> {"batches": [draw_batch of each seed, the later one redrawn where its keys meet an earlier batch's], "redrawn": how
  often that happened, "n": ids per batch}."""
  key = tuple(int(s) for s in seeds)
  if key not in _BATCHES:
    taken, batches, redrawn = set(), [], 0
    for s in key:
      attempt = 0
      while True:
        b = G.draw_batch(np.random.default_rng([s, attempt]))
        if taken.isdisjoint(b["keys"].tolist()):
          break
        attempt += 1
        redrawn += 1
      taken.update(b["keys"].tolist())
      batches.append(b)
    _BATCHES[key] = {"batches": batches, "redrawn": redrawn, "n": int(batches[0]["ids"].size)}
  return _BATCHES[key]


def table_batches(i):
  """Table i's batches: [the warm-up's, replay 0's, ... replay R - 1's]."""
  return replay_batches(SEEDS)["batches"][i * (R + 1):(i + 1) * (R + 1)]


def has_lookup(shape):
  return shape in ("tok", "plain")


def new_keys(batch, family, lookup):
  """(keys the step inserts into the var, keys it inserts into each slot table), by the ops' rules alone.
  The var: the batch's keys that `pre` did not insert — by the lookup, or by the apply itself (FindOrInsert).
  A slot table gets a row for every key the step updates.  Plain Adam updates every key.  The others leave out a key whose
  frequency is below ENTER when the apply looks: behind the lookup a key's frequency is its hits in `pre` plus its
  occurrences in the batch; without one, a key the apply itself inserts is never left out and a present key has its hits
  in `pre` only."""
  pre = dict(zip(*[a.tolist() for a in np.unique(batch["pre"], return_counts=True)]))
  occ = dict(zip(batch["keys"].tolist(), batch["counts"].tolist()))
  nvar = sum(1 for k in occ if k not in pre)
  if family == "adam":
    return nvar, len(occ)
  if lookup:
    return nvar, sum(1 for k in occ if pre.get(k, 0) + occ[k] >= G.ENTER)
  return nvar, sum(1 for k in occ if k not in pre or pre[k] >= G.ENTER)


def captured_ids(shape, n):
  """Ids the host's bounds take at the capture: (the var's, a slot table's).  Every inserting call takes its whole batch
  length (kvhip.hip ensure_capacity: worst case, every id is new)."""
  return (2 * n if has_lookup(shape) else n), n


def room(shape, n, replays=R):
  """max_new_ids of kv_prepare_capture, (var, slot table): what the replays can insert — at most every id of every replay —
  plus the ids the captured calls themselves take from the host's bounds."""
  cv, cs = captured_ids(shape, n)
  return replays * n + cv, replays * n + cs


def init_rows(keys, seed, init_table):
  """The init rule's rows of `keys`, all at once (_kv_model.Table._init_rule in uint64 arithmetic)."""
  with np.errstate(over="ignore"):
    x = np.asarray(keys, np.int64).astype(np.uint64) ^ np.uint64((int(seed) * 0x9E3779B97F4A7C15) & M.M64)
    x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
  n = np.uint64(init_table.shape[0])
  a, b = (x & np.uint64(0xFFFFFFFF)) % n, (x >> np.uint64(32)) % n
  return ((init_table[a.astype(np.int64)] + init_table[b.astype(np.int64)]) * F(0.5)).astype(F)


# ---- the reference trajectories ---------------------------------------------------------------------------------------------
RADAM_BRANCH = (True, False, True)      # tractable, amsgrad, nesterov: _row_geometry's second step


def _specs(family, D, tables):
  out = []
  for i in range(tables):
    rng = np.random.default_rng([SEEDS[0], D, G.FAMILIES.index(family), i])
    vinit, sinits = G.inits(family, D, rng)
    batches = table_batches(i)
    grads = [G.step_grads(rng, b, D) for b in batches]
    dd = [G._dedup(b["ids"], g) for b, g in zip(batches, grads)]
    out.append({"seed": 7 + i, "vinit": vinit, "sinits": sinits, "batches": batches, "grads": grads, "u": [d[0] for d in dd],
                "s": [d[1] for d in dd]})
  return out


def _side(family, D, sp):
  cls = G._OracleSide if family in G.ORACLE_FAMILIES else G._ModelSide
  side = cls(family, D, sp["seed"], sp["vinit"], sp["sinits"])
  for b in sp["batches"]:                # every batch's `pre` before the capture
    side.lookup(b["pre"])
  return side


def _model_hp(family, D, lookup, specs):
  """The scalars of the four model families, placed by the rows ALL the steps start from (resolve_step does not depend on
  them, and the batches are disjoint)."""
  b1p, b2p = G.beta_pows(0)
  if family == "adam":
    return (0.05, b1p, b2p, 0.9, 0.999, 1e-8)
  xs, ss, gs = [], [], []
  for sp in specs:
    side = _side(family, D, sp)
    for b, u, s in zip(sp["batches"], sp["u"], sp["s"]):
      if lookup:
        side.lookup(b["ids"])
      ctx = M.resolve_step(family, side.tables[0], side.tables[1:], u, s)
      xs.append(ctx["x"]); ss.append(ctx["srows"]); gs.append(ctx["g"])
  x, g = np.concatenate(xs), np.concatenate(gs)
  srows = [np.concatenate([t[j] for t in ss]) for j in range(len(ss[0]))]
  rng = np.random.default_rng([SEEDS[0], D, 99])
  if family == "ftrl_v2":                # l1 = the median |linear'|: about half of the elements are zeroed
    import _ftrl_ref as RF
    lr, _, _, two_l2s, lrp = RF._hp(0.1, 0.0, 1e-2, 1e-2, -0.5)
    return (0.1, float(np.median(np.abs(RF._linear(x, srows[0], srows[1], g, lr, two_l2s, lrp)[1]))), 1e-2, 1e-2, -0.5)
  if family == "group_ftrl_v2":
    hp0 = (0.1, 0.0, 1e-2, 1e-2, -0.5)
    return (0.1, M.lasso_threshold(M.linear_norms(family, x, srows, g, hp0)[0], rng)) + hp0[2:]
  import _radam_ref as RR
  hp0 = (0.1, b1p, b2p, 0.9, 0.999, 1e-7, 0.0, 1e-2, 0.0, 0.4) + RADAM_BRANCH
  hp1 = hp0[:6] + (float(np.median(np.abs(M.linear_norms(family, x, srows, g, hp0)[1]))),) + hp0[7:]
  return hp1[:8] + (M.lasso_threshold(RR.row_norms(x, srows[0], g, *hp1), rng) / float(np.sqrt(D)),) + hp1[9:]


def _oracle_steps(family, D, lookup, sp, hp, l21):
  """One table's steps on the oracle -> (steps, the norms of the keys the steps updated)."""
  side = _side(family, D, sp)
  group = family in G.GROUP_FAMILIES
  nt = len(side.tables)
  init = M.Table(D, sp["vinit"], sp["seed"])
  av, aslots = G.ATOL[family]
  steps, norms = [], []
  for b, grad, u, s in zip(sp["batches"], sp["grads"], sp["u"], sp["s"]):
    keys = b["keys"]
    maps = [side.counters(j)[0] for j in range(nt)]
    out = side.tables[0].gather_or_insert(b["ids"]) if lookup else None
    before = [side.rows(j, keys) for j in range(nt)]
    absent = np.array([m is None for m in side.metas(0, keys)])
    before[0][absent] = np.stack([init.init_row(int(k)) for k in keys[absent]]) if absent.any() else 0   # the apply inserts them
    for j in range(1, nt):               # a slot row the step creates starts from the init rule's row (constant tables)
      before[j][:] = sp["sinits"][j - 1][0]
    gk = s[[int(np.flatnonzero(u == k)[0]) for k in keys]]
    side.apply(u, s, hp)
    new = [side.rows(j, keys) for j in range(nt)]
    metas = [side.metas(j, keys) for j in range(nt)]
    live = np.array([m is not None for m in metas[1]])        # the keys the step updated: they have their slot rows now
    tables = [{"rows32": new[j], "tol": np.where(live[:, None], G.RTOL * np.abs(new[j]) + ([av] + aslots)[j], 0.0),
               "rows64": None, "widen": None, "metas": metas[j], "new": side.counters(j)[0] - maps[j]} for j in range(nt)]
    clear, black, ref_err = np.ones(keys.size, bool), np.zeros(keys.size, bool), 0.0
    if group:
      norm = G._oracle_norms(family, side, keys, D, hp)
      norms.append(norm[live])
      thr = l21 * float(np.sqrt(F(D)))
      with np.errstate(all="ignore"):
        scale = 1.0 - thr / np.maximum(norm, 1e-300)
      clear = ~live | (np.abs(scale) > G.SKIP_BELOW)
      black = np.array([m["blacklist"] for m in metas[0]]) & live
      fn = G.group_adam64 if family.startswith("group_adam") else G.sparse_group_ftrl64
      x64, upd = fn(*[t[live] for t in before], gk[live], *hp)
      bar = G.RTOL / np.maximum(scale[live], G.SKIP_BELOW)[:, None] * np.abs(x64) + av
      ok = clear[live]
      assert np.array_equal(upd[ok], ~black[live][ok]), (family, D)
      err = (np.abs(new[0][live].astype(np.float64) - x64) / bar).max(axis=1)
      ref_err = float(err[ok].max())
      rows64, tol, widen = new[0].astype(np.float64), np.zeros(new[0].shape), np.ones((keys.size, 1))
      rows64[live], tol[live], widen[live] = x64, bar, np.maximum(1.0, 4.0 * err)[:, None]
      tables[0].update(rows64=rows64, tol=tol, widen=widen)
    steps.append({"batch": b, "ids": b["ids"], "grad": grad, "u": u, "s": s, "lookup": out, "tables": tables, "live": live,
                  "clear": clear, "black": black, "ref_err": ref_err, "zeros": None})
  return steps, norms, [side.counters(j) for j in range(nt)]


def _model_steps(family, D, lookup, sp, hp):
  side = _side(family, D, sp)
  group = family in G.GROUP_FAMILIES
  nt = len(side.tables)
  steps = []
  for b, grad, u, s in zip(sp["batches"], sp["grads"], sp["u"], sp["s"]):
    keys = b["keys"]
    pos = {int(k): i for i, k in enumerate(keys.tolist())}
    maps = [side.counters(j)[0] for j in range(nt)]
    out = side.tables[0].gather_or_insert(b["ids"]) if lookup else None
    res = M.apply_step(family, side.tables[0], side.tables[1:], u, s, hp, bar=group)
    li = np.array([pos[k] for k in res["keys"]], np.int64)
    live = np.zeros(keys.size, bool)
    live[li] = True
    clear, black, zeros = np.ones(keys.size, bool), np.zeros(keys.size, bool), None
    if group:
      with np.errstate(all="ignore"):
        scale = 1.0 - 1.0 / res["ratio"]
      clear[li] = np.abs(scale) > G.SKIP_BELOW
      black[li] = ~res["updated"]
    new = [side.rows(j, keys) for j in range(nt)]
    if family == "ftrl_v2":
      zeros = (int((new[0][live] == 0).sum()), int(new[0][live].size))
    tables = [{"rows32": new[j], "tol": side.tables[j].tols(keys), "rows64": None, "widen": None, "metas": side.metas(j, keys),
               "new": side.counters(j)[0] - maps[j]} for j in range(nt)]
    steps.append({"batch": b, "ids": b["ids"], "grad": grad, "u": u, "s": s, "lookup": out, "tables": tables, "live": live,
                  "clear": clear, "black": black, "ref_err": 0.0, "zeros": zeros})
  return steps, [side.counters(j) for j in range(nt)]


_CACHE = {}


def trajectory(family, D, lookup, tables=1):
  """-> {"hp": the scalars of the capture, "exact": the rows are held bit for bit, "tables": [per table {"seed", "vinit",
  "sinits", "pre": every batch's `pre` lookup, "steps": [the warm-up's, then the R replays': {"batch", "ids", "grad", "u", "s",
  "lookup": the rows the step's lookup returns (None: the step has none), "tables": [per table of the set {"rows32", "tol",
  "rows64", "widen" (_row_geometry's second comparison; None: there is none), "metas", "new": keys the step inserted}],
  "live", "clear", "black", "ref_err", "zeros"}], "counters": [per table of the set (map size, size, frequency sum) at the end]}]}.
  Cached: every step shape with (without) a lookup runs the same trajectory."""
  key = (family, int(D), bool(lookup), int(tables))
  if key in _CACHE:
    return _CACHE[key]
  specs = _specs(family, D, tables)
  out = {"exact": family in ("adam", "ftrl_v2"), "tables": []}
  if family in G.ORACLE_FAMILIES:
    l21 = 0.0
    if family in G.GROUP_FAMILIES:       # the norms of every step, with the threshold at zero; then the threshold, once
      norms = [n for sp in specs for n in _oracle_steps(family, D, lookup, sp, G._oracle_hp(family, 0, 0.0), 0.0)[1]]
      l21 = M.lasso_threshold(np.concatenate(norms), np.random.default_rng([SEEDS[0], D, 99])) / float(np.sqrt(F(D)))
    out["hp"] = G._oracle_hp(family, 0, l21)
    runs = [_oracle_steps(family, D, lookup, sp, out["hp"], l21) for sp in specs]
    runs = [(r[0], r[2]) for r in runs]
  else:
    out["hp"] = _model_hp(family, D, lookup, specs)
    runs = [_model_steps(family, D, lookup, sp, out["hp"]) for sp in specs]
  for sp, (steps, counters) in zip(specs, runs):
    out["tables"].append({"seed": sp["seed"], "vinit": sp["vinit"], "sinits": sp["sinits"], "pre": [b["pre"] for b in sp["batches"]],
                          "steps": steps, "counters": counters})
  _CACHE[key] = out
  return out


# ---- case 2: state changed between replays --------------------------------------------------------------------------------
CASE2_FAMILY, CASE2_D = "adam", 32
NEW_DAY = G.DAY + 3


def victims(batch):
  """Keys of `batch` that kv_delete removes just before the batch's replay: every third key its `pre` lookup inserted.  The
  replay finds their entries as tombstones and inserts them again: the init rule's row, the frequency from its occurrences."""
  return np.unique(batch["pre"])[::3]


def early_victims(tables=1):
  """Keys no batch holds, inserted before and deleted just ahead of the capture of variant (b): the free list is then in
  the graph.  More than one replay inserts and fewer than two do: the replays pop the list empty, then take fresh rows."""
  taken = set(k for b in replay_batches(SEEDS)["batches"] for k in b["keys"].tolist())
  keys = [k for k in range(1 << 21, (1 << 21) + 400) if k not in taken]
  nvar = new_keys(table_batches(0)[1], CASE2_FAMILY, True)[0] + victims(table_batches(0)[1]).size
  return np.array(keys[:nvar + nvar // 4], np.int64)


def case2_trajectory(early, new_day=False):
  """The model of variants (a) and (b) (early: (b)), and with new_day of (c) — there without deletes.  The captured step is
  plain Adam's "tok" step.  -> as trajectory()'s one table, each step with "deleted" (the keys removed ahead of it) and
  "counters" (per table, after the step); "early": the keys of early_victims."""
  family, D = CASE2_FAMILY, CASE2_D
  sp = _specs(family, D, 1)[0]
  hp = _model_hp(family, D, True, [sp])
  side = _side(family, D, sp)
  gone = early_victims() if early else np.zeros(0, np.int64)
  side.lookup(gone)
  steps = []
  for k, (b, grad, u, s) in enumerate(zip(sp["batches"], sp["grads"], sp["u"], sp["s"])):
    dele = np.zeros(0, np.int64)
    if k == 1 and early:                 # behind the warm-up, ahead of the capture
      side.tables[0].delete(gone)
    if k >= 2 and not new_day:           # between two replays
      dele = victims(b)
      assert side.tables[0].delete(dele) == dele.size
    keys = b["keys"]
    out = side.tables[0].gather_or_insert(b["ids"])
    M.apply_step(family, side.tables[0], side.tables[1:], u, s, hp)
    steps.append({"batch": b, "ids": b["ids"], "grad": grad, "u": u, "s": s, "lookup": out, "deleted": dele,
                  "tables": [{"rows32": side.rows(j, keys), "metas": side.metas(j, keys)} for j in range(2)],
                  "counters": [side.counters(j) for j in range(2)]})
  return {"hp": hp, "seed": sp["seed"], "vinit": sp["vinit"], "sinits": sp["sinits"], "pre": [b["pre"] for b in sp["batches"]],
          "early": gone, "steps": steps}


# ---- cases 3 and 4: the host's bounds ---------------------------------------------------------------------------------------
def slab_after(rows_ub, extra, rows_cap, chunk):
  """kvhip.hip ensure_capacity's slab rule with an exact bound: whole chunks until rows_ub + extra fits."""
  while rows_ub + extra > rows_cap:
    rows_cap += chunk
  return rows_cap


def bounds_case():
  """Case 3.  One lookup of n distinct ids is captured and replayed `replays` times on fresh ids behind
  kv_prepare_capture(h, replays n): the host's bounds took n, the device inserted replays n — the host lags by `lag`.
  Then `eager` eager calls of n fresh ids each, more than two growth chunks of rows since the capture."""
  chunk = growth_chunk()
  n, replays = 4096, 3
  lag = (replays - 1) * n
  prefill = 4 * lag
  eager = (2 * chunk) // n - replays + 1
  return {"chunk": chunk, "n": n, "replays": replays, "lag": lag, "prefill": prefill, "eager": eager, "dim": 4,
          "prepared": replays * n, "total": prefill + (1 + replays + eager) * n}


def bounds_keys(c):
  """Distinct keys of case 3: (the prefill's, the warm-up's, [each replay's], [each eager call's])."""
  keys = (np.arange(1, c["total"] + 1, dtype=np.int64) * 1000003) ^ 0x5bd1e995
  assert np.unique(keys).size == keys.size
  n, p = c["n"], c["prefill"]
  cuts = [keys[p + i * n: p + (i + 1) * n] for i in range(1 + c["replays"] + c["eager"])]
  return keys[:p], cuts[0], cuts[1:1 + c["replays"]], cuts[1 + c["replays"]:]


def refusal_case():
  """Case 4.  A table of `small` keys; the warm-up, a lookup of m copies of one present key, makes the host grow the slab
  for m new rows (its worst case) and inserts none; one lookup of m distinct fresh keys then fills that room.  Behind
  kv_prepare_capture(h, 0) the captured lookup of the m copies would need m rows more than the slab has."""
  chunk = growth_chunk()
  small, m = 100, chunk
  cap0 = slab_after(1, small, chunk, chunk)                  # (row 0 is nobody's: the bump allocator starts at 1)
  cap1 = slab_after(1 + small, m, cap0, chunk)               # the warm-up
  rows = 1 + small + m                                       # behind the fill
  return {"chunk": chunk, "small": small, "m": m, "dim": 4, "rows_cap": slab_after(1 + small, m, cap1, chunk), "rows": rows,
          "after": 2172}
