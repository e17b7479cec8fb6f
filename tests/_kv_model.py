"""A host model of a KvVariable in NumPy float32, and of one optimizer step of the four families the oracle does not
restate: what a whole random program is carried with, without asking the device for anything.

  Row / Table    key -> (row, frequency word, blacklist, under_threshold) with the reference semantics of the table ops, as
                 oracle/kv_oracle.cc states them (tests/test_kv_model.py holds the two against each other op by op);
  apply_step     the bookkeeping of one step of ftrl_v2 / group_ftrl_v2 / group_radam / adam on unique ids and their summed
                 gradient rows, stated ONCE: the enter-threshold filter, which slot rows are created or hit, when a var is
                 blacklisted or lifted, which under_threshold flags are recomputed.  The row arithmetic is that of
                 tests/_ftrl_ref.py, tests/_radam_ref.py and tests/_adam_ref.py, called on all of a step's rows at once;
  Program        the random-program generator shared by tests/test_kv_model.py (conditions, on the model alone) and
                 tests/test_gpu_fuzz_optimizers.py (the same programs side by side with the GPU tables).

The allowance (programs whose rows depend on a row norm: group FTRL-V2 always, group RAdam with l21 > 0).  The kernel sums
the norm in another order than NumPy, so the var is good to the per-op files' bar (group FTRL-V2: rtol 1e-5, atol 1e-7;
group RAdam: (1e-6 / scale) |x| + 1e-9), and whatever is computed from that var later is off by what the arithmetic carries.
Every Row has `tol`, an absolute per-element allowance, and `acc`, the sum of the relative bars it took.  step_allowance
propagates the allowances of a step's inputs to its outputs to first order and adds the bar to the var; the slot rows get
no bar of their own (their arithmetic is the kernels' operation by operation), only what they carry, plus 2^-22 (four half
ulps) of each term of a sum that cancels, where the same roundings happen at slightly different inputs.
tests/test_kv_model.py holds the propagation against float64: a step at inputs moved by their allowances against the step
at the inputs themselves.  insert,
scatter_update op 0 and blacklisting put exact values: the allowance goes back to zero.  The other scatter ops carry it
(min, max unchanged; add and sub plus one ulp of the result; mul and div scaled by the update, plus that ulp).
"""
import numpy as np

import _ftrl_ref as RF
import _radam_ref as RR

F = np.float32
CUTOFF = F(1e-20)
M64 = (1 << 64) - 1


def _mix64(x):
  """The init rule's picker (oracle/kv_oracle.cc mix64, picker mode 1; the library's pick64)."""
  x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & M64
  x ^= x >> 27; x = (x * 0x94d049bb133111eb) & M64
  x ^= x >> 31
  return x


class Row(object):
  __slots__ = ("row", "freq", "black", "under", "tol", "acc")

  def __init__(self, row, freq, black=False):
    self.row, self.freq, self.black = np.asarray(row, F).copy(), int(freq), bool(black)
    self.under = True
    self.tol, self.acc = 0.0, 0.0
    self.update_under()

  def update_under(self):
    """UpdateUnderThreshold (kv_variable.h:837-861): a blacklisted row is under; else every |element| below the cutoff."""
    self.under = True if self.black else bool(np.all(np.abs(self.row) < CUTOFF))

  def meta(self):
    """The record as kv_get_meta / OracleKv.meta report it."""
    return {"freq": self.freq & 0xFFFF, "day": self.freq >> 16, "blacklist": self.black, "under_threshold": self.under}


_SCATTER = [lambda l, v: v, lambda l, v: l + v, lambda l, v: l - v, lambda l, v: l * v, lambda l, v: l / v,
            lambda l, v: np.where(v < l, v, l), lambda l, v: np.where(l < v, v, l)]       # std::min / std::max


class Table(object):
  """key -> Row.  init_table [R, dim], seed: the init rule 0.5 (T[r1] + T[r2]) (kv_variable.h:889-898)."""

  def __init__(self, dim, init_table, seed=0, day=0, enter_threshold=0):
    self.dim, self.init_table, self.seed, self.day = int(dim), np.asarray(init_table, F), int(seed), int(day)
    self.enter_threshold = min(int(enter_threshold), 65535)
    self.rows = {}
    self._init_rows = {}

  # ---- the pieces -----------------------------------------------------------------------------------------------------
  def init_row(self, key):
    r = self._init_rows.get(key)
    if r is None:
      r = self._init_rows[key] = self._init_rule(key)
    return r

  def _init_rule(self, key):
    h = _mix64(((int(key) & M64) ^ ((self.seed * 0x9E3779B97F4A7C15) & M64)) & M64)
    R = self.init_table.shape[0]
    return ((self.init_table[(h & 0xFFFFFFFF) % R] + self.init_table[(h >> 32) % R]) * F(0.5)).astype(F)

  def hit(self, key, count=1):
    """AddFrequency(count, today) (embedding_value.h:189-193), the count saturated first (utility.h:57-71)."""
    r = self.rows[key]
    r.freq = (self.day << 16) | min((r.freq & 0xFFFF) + min(int(count), 65535), 65535)

  def low_freq(self, r):
    return (r.freq & 0xFFFF) < self.enter_threshold           # kv_variable.h:910-912

  def blacklist(self, key):
    """MarkBlacklist (table_manager.h:335-357): the row is given up and reads as zeros."""
    r = self.rows[int(key)]
    r.black, r.under, r.row = True, True, np.zeros(self.dim, F)
    r.tol, r.acc = 0.0, 0.0

  def set_day(self, day):
    self.day = int(day)

  # ---- the table ops (oracle/kv_oracle.cc kvo_*) --------------------------------------------------------------------------
  def gather_or_insert(self, ids, counts=None):
    """GatherOrInsert (kv_variable.h:263-380), one occurrence after the other: a key found gets AddFrequency(count, today)
    and UpdateUnderThreshold, a blacklisted one reads as zeros; a missing key is inserted with the init rule's row and the
    word today << 16 | count."""
    ids = np.asarray(ids).reshape(-1)
    out = np.zeros((ids.size, self.dim), F)
    for i, k in enumerate(ids.tolist()):
      c = 1 if counts is None else int(counts[i])
      r = self.rows.get(k)
      if r is not None:
        self.hit(k, c)
        r.update_under()
      else:
        r = self.rows[k] = Row(self.init_row(k), (self.day << 16) | min(c, 65535))
      if not r.black:
        out[i] = r.row
    return out

  lookup = gather_or_insert                                   # (the name tests/_adam_ref.py's users know it by)

  def gather_or_zeros(self, keys):
    """GatherOrZeros (kv_variable.h:239-254): missing and blacklisted keys read zeros; nothing is counted."""
    z = np.zeros(self.dim, F)
    rows = [self.rows[k].row if k in self.rows else z for k in np.asarray(keys).reshape(-1).tolist()]
    return np.stack(rows) if rows else np.zeros((0, self.dim), F)

  read = gather_or_zeros

  def scatter_update(self, ids, upd, op=0):
    """ScatterUpdate (kv_variable.h:616-734), op 0 assign, 1 add, 2 sub, 3 mul, 4 div, 5 min, 6 max: a missing key is
    inserted first (init rule, frequency word 1); a blacklisted row is skipped; UpdateUnderThreshold; no frequency."""
    upd = np.asarray(upd, F).reshape(-1, self.dim)
    fn = _SCATTER[int(op)]
    for k, u in zip(np.asarray(ids).reshape(-1).tolist(), upd):
      r = self.rows.get(k)
      if r is None:
        r = self.rows[k] = Row(self.init_row(k), 1)
      if r.black:
        continue
      with np.errstate(all="ignore"):
        r.row = fn(r.row, u).astype(F)
      if op == 0:
        r.tol, r.acc = 0.0, 0.0
      elif op in (1, 2, 3, 4) and np.any(r.tol):            # the same rounding at two slightly different rows: one ulp more
        a = np.abs(u.astype(np.float64))
        t = r.tol * a if op == 3 else r.tol / a if op == 4 else r.tol
        r.tol = t + np.where(t > 0, 2.0 ** -23 * np.abs(r.row.astype(np.float64)), 0.0)
      r.update_under()

  def insert(self, ids, vals):
    """InsertOrUpdate (kv_variable.h:423-485): an existing key's row is overwritten unless blacklisted; a missing key is
    inserted with frequency word 1; UpdateUnderThreshold either way."""
    vals = np.asarray(vals, F).reshape(-1, self.dim)
    for k, v in zip(np.asarray(ids).reshape(-1).tolist(), vals):
      r = self.rows.get(k)
      if r is None:
        self.rows[k] = Row(v, 1)
      else:
        if not r.black:
          r.row = v.copy()
          r.tol, r.acc = 0.0, 0.0
        r.update_under()

  def delete(self, ids):
    """Delete (kv_variable.h:737-755) -> the number of keys that were there."""
    gone = 0
    for k in np.asarray(ids).reshape(-1).tolist():
      if self.rows.pop(k, None) is not None:
        gone += 1
    return gone

  def delete_with_timestamp(self, threshold):
    """DeleteWithTimestamp (kv_variable.h:757-789): day > 0 and today - day >= uint16(threshold) -> the keys, sorted."""
    dl = sorted(k for k, r in self.rows.items() if (r.freq >> 16) > 0 and self.day - (r.freq >> 16) >= (int(threshold) & 0xFFFF))
    for k in dl:
      del self.rows[k]
    return dl

  def get_count(self, keys):
    return np.array([self.rows[k].freq & 0xFFFF if k in self.rows else 0 for k in np.asarray(keys).reshape(-1).tolist()], np.int32)

  def get_timestamp(self, keys):
    return np.array([self.rows[k].freq >> 16 if k in self.rows else self.day for k in np.asarray(keys).reshape(-1).tolist()],
                    np.uint32)

  def size(self):
    """kv_variable.h:139-175: blacklisted keys and keys below the enter threshold do not count."""
    return sum(1 for r in self.rows.values() if not r.black and not self.low_freq(r))

  def sum_freq(self):
    return sum(r.freq & 0xFFFF for r in self.rows.values() if not r.black and not self.low_freq(r))

  def map_size(self):
    return len(self.rows)

  def meta(self, key):
    r = self.rows.get(int(key))
    return None if r is None else r.meta()

  def metas(self, keys):
    return [self.meta(k) for k in np.asarray(keys).reshape(-1).tolist()]

  def tols(self, keys):
    """The allowance of gather_or_zeros(keys), [n, dim] float64."""
    out = np.zeros((np.asarray(keys).size, self.dim))
    for i, k in enumerate(np.asarray(keys).reshape(-1).tolist()):
      r = self.rows.get(k)
      if r is not None:
        out[i] = r.tol
    return out


# ---- one optimizer step -------------------------------------------------------------------------------------------------
FAMILIES = ("ftrl_v2", "group_ftrl_v2", "group_radam", "adam")
FTRL_BAR = (1e-5, 1e-7)          # tests/test_gpu_ftrl_v2.py test_parity_unique_ids, the group op at lr_power -0.5
RADAM_BAR = (1e-6, 1e-9)         # tests/test_gpu_group_radam.py _lasso_tol: RTOL / scale of the value + 1e-9


def slot_dims(family, D):
  return {"ftrl_v2": [D, D], "group_ftrl_v2": [D, D], "group_radam": [5 * D], "adam": [2 * D]}[family]


def linear_norms(family, x, srows, g, hp):
  """Per row, in float64 on the float32 step's linear': what the group op compares with its lasso threshold (it does not
  depend on that threshold), and linear' itself."""
  if family == "group_ftrl_v2":
    lr, _, _, two_l2s, lrp = RF._hp(*hp)
    z1 = RF._linear(x, srows[0], srows[1], g, lr, two_l2s, lrp)[1].astype(F)
    return np.sqrt((z1.astype(np.float64) ** 2).sum(axis=1)), z1
  D = x.shape[1]
  z1 = RR.group_radam(x, srows[0], g, *hp)[1][:, 2 * D:3 * D]
  return RR.row_norms(x, srows[0], g, *hp), z1


def tols_of(rows, d):
  """The allowances of Row objects as [n, d] float64."""
  t = np.zeros((len(rows), d))
  for i, r in enumerate(rows):
    if np.any(r.tol):
      t[i] = r.tol
  return t


def step_allowance(family, x, srows, g, hp, tin, new, upd, norm):
  """The allowances of a group step's outputs from those of its inputs, to first order.
  x, srows, g: the rows the step starts from; tin = [var, slot...] their allowances; new = [var', slot'...]; upd, norm: the
  step's decisions and float64 row norms.  -> ([var', slot'...] allowances, the relative bar each var took).
  Four half ulps (2^-22) of every term of a cancelling sum are added to the sum's allowance."""
  D = x.shape[1]
  x64, g64 = x.astype(np.float64), g.astype(np.float64)
  x1 = np.abs(new[0].astype(np.float64))
  n64 = np.where(norm > 0, norm, 1.0)[:, None]                # (a row of norm 0 is blacklisted: no allowance to give)
  l2norm = lambda t: np.sqrt((t * t).sum(axis=1))[:, None]
  if family == "group_ftrl_v2":
    # gs = g + 2 l2s x; accum_new = accum + gs^2; p = accum^(-lr_power); linear' = linear + gs - (p_new - p_old) / lr x;
    # var' = (l1 - norm) / (y norm) linear', y = p_new / lr + 2 l2; accum' = accum + 2 (g + 2 l2s var')^2
    lr, l1, two_l2, two_l2s, lrp = (float(v) for v in RF._hp(*hp))
    xt, at, zt = tin
    a64, z1 = srows[0].astype(np.float64), new[2].astype(np.float64)
    gs = g64 + two_l2s * x64
    na = a64 + gs * gs
    dpd = lambda v: -lrp * v ** (-lrp - 1.0)                 # d accum^(-lr_power) / d accum
    dgs = two_l2s * xt
    pn, po = na ** -lrp, a64 ** -lrp
    ddp = np.abs(dpd(a64) - dpd(na)) * at + dpd(na) * 2 * np.abs(gs) * dgs
    zt1 = zt + dgs + ddp / lr * np.abs(x64) + np.abs(pn - po) / lr * xt + \
        2.0 ** -22 * (np.abs(srows[1]) + np.abs(z1) + (pn + po) / lr * np.abs(x64) + np.abs(gs))
    y = pn / lr + two_l2
    dy = dpd(na) * (at + 2 * np.abs(gs) * dgs) / lr
    rel = np.full(x.shape[0], FTRL_BAR[0])
    xt1 = np.abs(l1 - n64) / (y * n64) * zt1 + np.abs(z1) * l1 / (n64 * n64 * y) * l2norm(zt1) + x1 * dy / y + \
        FTRL_BAR[0] * x1 + FTRL_BAR[1]
    gs2 = np.abs(g64 + two_l2s * np.where(upd[:, None], new[0], x))
    at1 = at + 4.0 * gs2 * two_l2s * np.where(upd[:, None], xt1, xt) + 2.0 ** -22 * np.abs(new[1])
    return [xt1, at1, zt1], rel
  # group RAdam: linear' = linear + rm - (rv - vhat) x; var' = u scale / (rv + 2 l2), u = clamp(linear') - linear',
  # scale = 1 - thr / |u|; m, v, vhat and vamsgrad never see the var
  xt, st = tin
  thr = float(F(hp[8])) * float(np.sqrt(F(D)))
  l1, l2 = float(F(hp[6])), float(F(hp[7]))
  s1 = new[1].astype(np.float64)
  rv, vh = s1[:, 3 * D:4 * D], srows[0][:, 3 * D:4 * D].astype(np.float64)
  z0, z1 = srows[0][:, 2 * D:3 * D].astype(np.float64), s1[:, 2 * D:3 * D]
  st1 = st.copy()
  moved = (xt > 0) | (st[:, 2 * D:3 * D] > 0)
  st1[:, 2 * D:3 * D] += np.abs(rv - vh) * xt + np.where(moved, 2.0 ** -22 * (np.abs(z0) + np.abs(z1) + np.maximum(rv, vh) * np.abs(x64)), 0.0)
  zt1 = st1[:, 2 * D:3 * D]
  scale = np.where(upd, 1.0 - thr / n64[:, 0], 1.0)
  rel = RADAM_BAR[0] / scale if thr > 0 else np.zeros(x.shape[0])
  u = np.abs(np.clip(z1, -l1, l1) - z1)
  xt1 = (zt1 * scale[:, None] + u * thr / (n64 * n64) * l2norm(zt1)) / (rv + 2.0 * l2) + rel[:, None] * x1 + \
      np.where(zt1 > 0, 2.0 ** -22 * x1, 0.0) + (RADAM_BAR[1] if thr > 0 else 0.0)
  return [xt1, st1], rel


def resolve_step(family, var, slots, uniq_ids, summed_grad):
  """The first half of a step, which does not depend on the op's scalars: the filter, the lifting, the slot rows created or
  hit (apply_step's docstring).  -> the context finish_step takes; ctx["x"], ctx["srows"], ctx["g"] are the rows the step
  starts from (the keys that pass the filter, in the order of uniq_ids)."""
  assert family in FAMILIES
  D = var.dim
  uniq = [int(k) for k in np.asarray(uniq_ids).reshape(-1)]
  g_all = np.asarray(summed_grad, F).reshape(len(uniq), D)
  live, filtered, lifted = [], [], []
  for i, k in enumerate(uniq):
    r = var.rows.get(k)
    if family == "adam":
      s = slots[0].rows.get(k)
      if s is not None:
        slots[0].hit(k)
        s.update_under()
      else:
        slots[0].rows[k] = Row(slots[0].init_row(k), (slots[0].day << 16) | 1)
      if r is None:
        var.rows[k] = Row(var.init_row(k), 1)
    else:
      if r is None:
        var.rows[k] = Row(var.init_row(k), 1)
      elif var.low_freq(r):
        filtered.append(k)
        continue
      elif r.black:
        r.black, r.under, r.row = False, True, np.zeros(D, F)          # RemoveBlacklist (table_manager.h:359-372)
        lifted.append(k)
      for s in slots:
        if k in s.rows:
          s.hit(k)
        else:
          s.rows[k] = Row(s.init_row(k), 1)
    live.append(i)
  keys = [uniq[i] for i in live]
  vr = [var.rows[k] for k in keys]
  sr = [[s.rows[k] for k in keys] for s in slots]
  return {"keys": keys, "filtered": filtered, "lifted": lifted, "vr": vr, "sr": sr, "g": g_all[live],
          "x": np.stack([r.row for r in vr]) if keys else np.zeros((0, D), F),
          "srows": [np.stack([r.row for r in rs]) if keys else np.zeros((0, s.dim), F) for rs, s in zip(sr, slots)]}


def finish_step(family, var, slots, ctx, hp, bar=False):
  """The second half: the row arithmetic with the scalars hp, the rows written, blacklisting, the flags (apply_step)."""
  D = var.dim
  keys, vr, sr, x, srows, g = (ctx[k] for k in ("keys", "vr", "sr", "x", "srows", "g"))
  out = {"keys": keys, "filtered": ctx["filtered"], "lifted": ctx["lifted"], "updated": None, "ratio": None, "hp": hp,
         "below": [], "max_acc": 0.0, "max_rel": 0.0, "allow": None}
  if not keys:
    return out
  under = lambda rows: np.all(np.abs(rows) < CUTOFF, axis=1).tolist()        # UpdateUnderThreshold, a step's rows at once

  if family == "adam":
    import _adam_ref as RA
    x1, m1, v1 = RA.row_math(x, srows[0][:, :D], srows[0][:, D:], g, *hp)
    s1 = np.concatenate([m1, v1], axis=1)
    ux, us = under(x1), under(s1)
    out["below"] = [k for k, r in zip(keys, vr) if var.low_freq(r)]
    for i, (r, s) in enumerate(zip(vr, sr[0])):
      if not s.black:                                          # ScatterUpdate(m_v)
        s.row, s.under = s1[i], us[i]
      if not r.black:                                          # ScatterSub(var)
        r.row, r.under = x1[i], ux[i]
    return out

  if family == "ftrl_v2":
    x1, a1, z1 = RF.ftrl_v2(x, srows[0], srows[1], g, *hp)
    for i, r in enumerate(vr):
      r.row, sr[0][i].row, sr[1][i].row = x1[i], a1[i], z1[i]
    return out

  if family == "group_ftrl_v2":
    x1, a1, z1, upd = RF.group_ftrl_v2(x, srows[0], srows[1], g, *hp)
    new = [x1, a1, z1]
    thr = float(F(hp[1]))
  else:
    x1, s1, upd = RR.group_radam(x, srows[0], g, *hp)
    new = [x1, s1]
    thr = float(F(hp[8])) * float(np.sqrt(F(D)))
  norm = linear_norms(family, x, srows, g, hp)[0]
  out["updated"] = upd
  if thr > 0:
    with np.errstate(all="ignore"):
      out["ratio"] = norm / thr
  if bar:
    tin = [tols_of(vr, D)] + [tols_of(rs, s.dim) for rs, s in zip(sr, slots)]
    tout, rel = step_allowance(family, x, srows, g, hp, tin, new, upd, norm)
    out["allow"] = {"x": x, "srows": srows, "g": g, "tin": tin, "new": new, "tout": tout, "upd": upd}
    if upd.any():     # the var rows' allowance relative to the row (largest element each)
      out["max_rel"] = float((tout[0][upd].max(axis=1) / np.maximum(np.abs(x1[upd]).max(axis=1), 1e-30)).max())
  flags = [under(n) for n in new]
  for i, r in enumerate(vr):
    if upd[i]:
      r.row, r.under = x1[i], flags[0][i]
      if bar:
        r.tol = tout[0][i]
        r.acc += float(rel[i])
        out["max_acc"] = max(out["max_acc"], r.acc)
    else:
      r.black, r.under, r.row, r.tol, r.acc = True, True, np.zeros(D, F), 0.0, 0.0          # MarkBlacklist
    for j in range(len(slots)):
      s = sr[j][i]
      s.row, s.under = new[1 + j][i], flags[1 + j][i]
      if bar:
        s.tol = tout[1 + j][i] if tout[1 + j][i].any() else 0.0
  return out


def apply_step(family, var, slots, uniq_ids, summed_grad, hp, bar=False):
  """One step of `family` on the Table models, in place, on unique ids and their summed gradient rows.

  hp: the op's scalars in its order, or a function (x, slot rows, g) -> those scalars that is shown the rows the step
  starts from: how a program places a lasso threshold.
  bar: carry the rows' allowances through the step (the module docstring).
  -> {"keys": the keys updated, "filtered": ..., "lifted": ..., "updated": per updated key, False where the step blacklisted
      it (None: the family cannot), "ratio": norm / threshold per key in float64 (None: no lasso threshold), "hp": ...,
      "below": the keys plain Adam updated although their frequency is below the threshold, "max_acc": the largest sum
      of relative bars a var row touched now carries, "max_rel": the largest allowance of a var row relative to the row,
      "allow": the step's inputs, outputs and their allowances (bar only)}.

  The group ops and FTRL-V2 (training_ops.cc, FindOrInsertUnsafe kv_variable.h:382-416):
    var    a missing key is inserted with the init rule's row and frequency word 1 and is never filtered; a key whose
           frequency is below the enter threshold is FILTERED: untouched, and it gets no slot rows; a blacklisted key that is
           not filtered is lifted first (a fresh zero row, under_threshold set).  No frequency word of the var's moves.
    slots  a missing row is created from the slot table's init rule with frequency word 1 and no day; an existing one gets
           one hit and today's day.
    flags  ftrl_v2 recomputes none (a row created now has the flag of its init row; a lifted var keeps under_threshold);
           the group ops blacklist the var where the norm does not pass, else recompute its flag from the new row, and
           recompute every slot row's flag from the row they wrote.
  Plain Adam is the reference's chain gather_or_insert(m_v) -> scatter_update(m_v) -> scatter_sub(var) (tests/_adam_ref.py):
    no filter; the slot row is found (one hit, today, flag recomputed) or inserted with the word today << 16 | 1; a missing
    var key is inserted with word 1; a blacklisted row of either table reads as zeros and is neither written nor lifted;
    flags from the rows written.
  """
  ctx = resolve_step(family, var, slots, uniq_ids, summed_grad)
  if callable(hp):
    hp = hp(ctx["x"], ctx["srows"], ctx["g"])
  return finish_step(family, var, slots, ctx, hp, bar)


# ---- the random programs --------------------------------------------------------------------------------------------------
DAY0 = 20000
DIMS = [4, 8, 20, 32, 64, 100, 5, 6]          # 5, 6: the sorted-position fallback kernels; 100: 16 lanes x 2
FORMS = ("plain", "tok", "unique", "counted", "batched")
OPS = ("lookup", "lookup_counts", "apply", "scatter", "insert", "delete", "expire", "query")
OP_P = [.15, .1, .3, .1, .05, .15, .05, .1]
RADAM_BRANCHES = {"plain": (False, False), "tractable": (True, False), "amsgrad": (True, True)}
MARGIN = 1.005                                # no key's norm / threshold within [1 / MARGIN, MARGIN]
# the seeds tests/test_gpu_fuzz_optimizers.py runs in each of its two modes, per family (seed % 3 == 1: the lasso programs of
# the two group families, half of their seeds; seed % 4 == 3: int32 keys, on lasso and exact programs alike); tests/test_kv_model.py asserts the generator's conditions on exactly these
SEEDS = {"ftrl_v2": [1, 3, 4, 6, 7, 12], "group_ftrl_v2": [0, 3, 7, 10, 22, 23], "group_radam": [0, 1, 3, 4, 5, 19],
         "adam": [0, 1, 2, 3, 4, 7]}
GQ = 2.0 ** -12                               # the counted form's gradients are multiples of this: any order sums them exactly


def dedup_sum(ids, grad):
  """TF-core's de-duplication: (unique ids in first-occurrence order, their gradient rows added one by one in occurrence
  order) — oracle/kv_oracle.cc kvo_dedup_segment_sum."""
  ids = np.asarray(ids).reshape(-1)
  grad = np.asarray(grad, F).reshape(ids.size, -1)
  pos, uniq = {}, []
  sums = np.zeros_like(grad)
  for i, k in enumerate(ids.tolist()):
    p = pos.get(k)
    if p is None:
      p = pos[k] = len(uniq); uniq.append(k)
    sums[p] += grad[i]                                        # (from zero, as unsorted_segment_sum does)
  return np.array(uniq, np.int64), sums[:len(uniq)].copy()


def lasso_threshold(norms, rng):
  """A threshold in the widest gap between adjacent norms (as tests/test_gpu_group_radam.py _pick_regularizers: between the
  10th and the 90th percentile when a gap of 2 % is found there, else anywhere); with one norm, half or twice it.  None:
  no positive norm."""
  n = np.unique(norms[norms > 0])
  if n.size == 0:
    return None
  if n.size == 1:
    return float(n[0]) * (0.5 if rng.integers(0, 2) else 2.0)
  gap = n[1:] / n[:-1]
  lo, hi = n.size // 10, n.size - n.size // 10
  k = int(np.argmax(gap))
  if hi - lo >= 2:
    kc = lo + int(np.argmax(gap[lo:hi - 1]))
    if gap[kc] >= 1.02:
      k = kc
  return float(np.sqrt(n[k] * n[k + 1]))


class TableSet(object):
  """One var and its slot tables."""

  def __init__(self, family, D, thr, vinit, sinits, seed):
    self.var = Table(D, vinit, seed, DAY0, thr)
    self.slots = [Table(d, t, seed, DAY0, 0) for d, t in zip(slot_dims(family, D), sinits)]
    self.vinit, self.sinits, self.seed = vinit, sinits, seed
    self.orphans = [set() for _ in self.slots]               # keys whose slot row was deleted while the var kept its own
    self.was_black = set()                                   # keys a group step blacklisted (and nothing removed since)

  @property
  def tables(self):
    return [self.var] + self.slots


class Program(object):
  """A 40-step random program of one family on two table sets A and B, carried on the models.  steps() yields, after the
  models have taken each step, what the step was and what it returns: the GPU test replays it and compares.  Deterministic
  in (family, seed, occ).  self.stats collects what the generator conditions are asserted on."""

  STEPS = 40

  def __init__(self, family, seed, occ, on_allow=None):
    self.family, self.seed, self.occ = family, int(seed), bool(occ)
    self.on_allow = on_allow                                 # called with every group step's inputs, outputs and allowances
    rng = self.rng = np.random.default_rng([FAMILIES.index(family), self.seed, int(self.occ), 2024])
    self.int32 = self.seed % 4 == 3
    self.D = D = int(rng.choice(DIMS))
    self.thr = int(rng.choice([0, 0, 2]))
    self.keyspace = int(rng.choice([50, 400, 5000]))
    self.lasso = family in ("group_ftrl_v2", "group_radam") and self.seed % 3 == 1
    self.exact = family in ("ftrl_v2", "adam") or (family == "group_radam" and not self.lasso)
    self.branch = str(rng.choice(sorted(RADAM_BRANCHES)))
    self.nesterov = bool(rng.integers(0, 2))
    self.sets = []
    for i in range(2):
      if family == "adam":
        vinit = rng.uniform(-0.5, 0.5, (32, D)).astype(F)
        sinits = [np.zeros((4, 2 * D), F)]
      else:       # rows of two magnitudes (tests/test_gpu_group_radam.py _var_init): the lasso norms fall into groups
        vinit = rng.uniform(0.5, 1.0, (32, D)) * 0.05
        vinit[::2] *= 1e-3
        vinit = vinit.astype(F)
        sinits = [np.zeros((4, 5 * D), F)] if family == "group_radam" else [np.full((4, D), 0.1, F), np.zeros((4, D), F)]
      self.sets.append(TableSet(family, D, self.thr, vinit, sinits, 10 * self.seed + i + 1))
    self.day = DAY0
    self.b1p, self.b2p = F(0.9), F(0.999)
    # the batched and the counted ops exist for dims that are multiples of 4 (the others are refused as unimplemented)
    self.forms = FORMS if D % 4 == 0 else FORMS[:3]
    self.universe = np.arange(-self.keyspace - 5, self.keyspace + 5, dtype=np.int64)
    self.stats = {"ops": set(), "forms": set(), "lasso_steps": 0, "branches": set(), "worst_margin": np.inf, "max_acc": 0.0, "max_rel": 0.0,
                  "black_lookup": 0, "black_delete": 0, "black_expire": 0, "black_lift": 0, "blacklisted": 0,
                  "orphan_apply": 0, "filtered_apply": 0, "applies": 0}

  # ---- hyperparameters -------------------------------------------------------------------------------------------------
  def _hp_fn(self, live_rows):
    """-> the scalars of this apply, one set for A and B (the batched form takes one): thresholds from the rows of both."""
    fam, rng = self.family, self.rng
    if fam == "ftrl_v2":
      return (0.1, 2e-3, 1e-2, 1e-2, -0.5)
    if fam == "adam":
      return (0.05, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-8)
    x = np.concatenate([t[0] for t in live_rows])
    srows = [np.concatenate([t[1][j] for t in live_rows]) for j in range(len(live_rows[0][1]))]
    g = np.concatenate([t[2] for t in live_rows])
    if fam == "group_ftrl_v2":
      hp0 = (0.1, 0.0, 1e-2, 1e-2, -0.5)
      if not self.lasso or not x.shape[0]:
        return hp0
      thr = lasso_threshold(linear_norms(fam, x, srows, g, hp0)[0], rng)
      return hp0 if thr is None else (0.1, thr) + hp0[2:]
    tract, ams = RADAM_BRANCHES[self.branch]
    hp0 = (0.1, float(self.b1p), float(self.b2p), 0.9, 0.999, 1e-7, 0.0, 1e-2, 0.0, 0.4, tract, ams, self.nesterov)
    if not x.shape[0]:
      return hp0
    # l1 = the median |linear'|: about half the elements clamped, and a row with every element clamped has norm 0 and is
    # blacklisted whatever l21 is — the blacklist / lifting cycle with no rounding involved
    l1 = float(np.median(np.abs(linear_norms(fam, x, srows, g, hp0)[1])))
    hp1 = hp0[:6] + (l1,) + hp0[7:]
    if not self.lasso:
      return hp1
    thr = lasso_threshold(RR.row_norms(x, srows[0], g, *hp1), rng)
    return hp1 if thr is None else hp1[:8] + (thr / float(np.sqrt(self.D)),) + hp1[9:]

  # ---- one apply on both sets --------------------------------------------------------------------------------------------
  def _apply(self, form):
    rng, D, st = self.rng, self.D, self.stats
    per = []
    for ts in self.sets:
      n = int(rng.choice([1, 7, 300, 3000]))
      ids = rng.integers(-self.keyspace, self.keyspace, n).astype(np.int64)
      g = (rng.normal(0, 1, (n, D)) * rng.choice([1e-1, 1e-3], (n, 1))).astype(F)
      if form == "counted":
        g = (np.round(g / F(GQ)) * F(GQ) + F(0)).astype(F)                 # (+ 0: no negative zeros)
      u, s = dedup_sum(ids, g)
      per.append({"ids": ids, "grad": g, "u": u, "s": s, "variant": int(rng.integers(0, 2))})
      if form == "tok":                                      # the training lookup whose token the apply comes with
        per[-1]["tok_rows"] = ts.var.gather_or_insert(ids if self.occ else u)
        per[-1]["tok_tol"] = ts.var.tols(ids if self.occ else u)
    # both sets' steps are resolved first: the scalars (one set for A and B: the batched form takes one) are placed by the
    # rows both start from
    ctxs = [resolve_step(self.family, ts.var, ts.slots, p["u"], p["s"]) for ts, p in zip(self.sets, per)]
    hp = self._hp_fn([(c["x"], c["srows"], c["g"]) for c in ctxs])
    for ts, p, ctx in zip(self.sets, per, ctxs):
      before_orphans = [set(o) for o in ts.orphans]
      res = finish_step(self.family, ts.var, ts.slots, ctx, hp, bar=not self.exact)
      if self.on_allow is not None and res["allow"] is not None:
        self.on_allow(self.family, hp, res["allow"])
      st["applies"] += 1
      st["filtered_apply"] += len(res["filtered"]) + len(res["below"])      # (plain Adam has no filter: the key is updated)
      st["black_lift"] += len(res["lifted"])
      for k in res["lifted"]:
        ts.was_black.discard(k)
      for j, o in enumerate(before_orphans):
        hit = o.intersection(res["keys"])
        st["orphan_apply"] += len(hit)
        ts.orphans[j] -= hit
      if res["updated"] is not None:
        bl = [k for k, u_ in zip(res["keys"], res["updated"]) if not u_]
        st["blacklisted"] += len(bl)
        ts.was_black.update(bl)
      if res["ratio"] is not None and len(res["keys"]):
        st["lasso_steps"] += 1
        r = res["ratio"]
        st["branches"].update(bool(b) for b in res["updated"])
        pos = r[r > 0]
        if pos.size:
          st["worst_margin"] = min(st["worst_margin"], float(np.exp(np.abs(np.log(pos)).min())))
      st["max_acc"] = max(st["max_acc"], res["max_acc"])
      st["max_rel"] = max(st["max_rel"], res["max_rel"])
    if self.family != "ftrl_v2":
      self.b1p, self.b2p = F(self.b1p * F(0.9)), F(self.b2p * F(0.999))
    return {"form": form, "hp": hp, "sets": per}

  def _touch_black(self, ts, ids, what):
    n = len(ts.was_black.intersection(int(k) for k in ids if int(k) in ts.var.rows and ts.var.rows[int(k)].black))
    self.stats[what] += n

  # ---- the program -------------------------------------------------------------------------------------------------------
  def steps(self):
    rng, D = self.rng, self.D
    for step in range(self.STEPS):
      op = str(rng.choice(OPS, p=OP_P))
      self.stats["ops"].add(op)
      out = {"step": step, "op": op, "sets": []}
      if op == "apply":
        form = str(rng.choice(self.forms))
        self.stats["forms"].add(form)
        # a burst of applies with nothing in between but the tok form's own lookup: the later ones find the slot mirrors the
        # first one left (kv_key_update.h key_update); every other op ends the mirror epoch
        out["form"], out["reps"] = form, [self._apply(form) for _ in range(int(rng.choice([1, 2, 3])))]
      elif op == "expire":
        self.day += int(rng.integers(1, 5))
        thr_days = int(rng.integers(2, 8))
        out["day"], out["thr_days"] = self.day, thr_days
        for ts in self.sets:
          for t in ts.tables:
            t.set_day(self.day)
          black = {k for k in ts.was_black if k in ts.var.rows and ts.var.rows[k].black}
          gone = ts.var.delete_with_timestamp(thr_days)
          self.stats["black_expire"] += len(black.intersection(gone))
          ts.was_black.difference_update(gone)
          for o in ts.orphans:
            o.difference_update(gone)
          out["sets"].append({"gone": gone})
      else:
        for ts in self.sets:
          n = int(rng.choice([1, 7, 300, 3000]))
          ids = rng.integers(-self.keyspace, self.keyspace, n).astype(np.int64)
          a = {"ids": ids}
          if op == "lookup":
            self._touch_black(ts, ids, "black_lookup")
            a["rows"], a["tol"] = ts.var.gather_or_insert(ids), ts.var.tols(ids)
          elif op == "lookup_counts":
            a["counts"] = rng.integers(1, 40000, n).astype(np.int32)
            self._touch_black(ts, ids, "black_lookup")
            a["rows"], a["tol"] = ts.var.gather_or_insert(ids, a["counts"]), ts.var.tols(ids)
          elif op == "scatter":
            a["ids"] = np.unique(ids)
            a["upd"] = rng.uniform(0.5, 2.0, (a["ids"].size, D)).astype(F)
            a["which"] = int(rng.integers(0, 7))
            ts.var.scatter_update(a["ids"], a["upd"], a["which"])
          elif op == "insert":
            a["ids"] = np.unique(ids)
            a["vals"] = rng.standard_normal((a["ids"].size, D)).astype(F)
            ts.var.insert(a["ids"], a["vals"])
          elif op == "delete":       # a random non-empty subset of {var, slot0, slot1}: a var may keep a hint to a slot row that is gone
            nt = len(ts.tables)
            mask = int(rng.integers(1, 1 << nt))
            a["tables"] = [j for j in range(nt) if mask >> j & 1]
            if 0 in a["tables"]:
              self._touch_black(ts, np.unique(ids), "black_delete")
              ts.was_black.difference_update(ids.tolist())
            for j, s in enumerate(ts.slots):
              if j + 1 in a["tables"] and 0 not in a["tables"]:
                ts.orphans[j].update(k for k in set(ids.tolist()) if k in s.rows and k in ts.var.rows)
              elif 0 in a["tables"]:
                ts.orphans[j].difference_update(ids.tolist())
            a["gone"] = [ts.tables[j].delete(ids) for j in a["tables"]]
          else:                      # query: read-only, var (the fused serving lookup) or a slot table
            a["table"] = int(rng.integers(0, len(ts.tables)))
            a["rows"], a["tol"] = ts.tables[a["table"]].gather_or_zeros(ids), ts.tables[a["table"]].tols(ids)
          out["sets"].append(a)
      last = step == self.STEPS - 1
      out["check"] = [self.universe if (last or self.keyspace <= 400) else
                      rng.integers(-self.keyspace - 5, self.keyspace + 5, 200).astype(np.int64) for _ in self.sets]
      yield out
