"""NumPy float32 restatement of ONE plain-Adam step (kvhip.h kv_apply_adam) on a dict-of-rows table model: the definition
the GPU tests compare against.

The reference has no op for the step: its AdamOptimizer composes it (tfplus python/training/adam.py:93-163) from TF-core's
de-duplication and three generic table ops.  What is restated here is that chain:

  unique ids in order of first occurrence, a repeated id's gradient rows added one by one in occurrence order;
  GatherOrInsert on the slot table m_v (kv_variable.h:263-380), count 1 per distinct id;
  m = beta1 m + g (1 - beta1);  v = beta2 v + (g g) (1 - beta2);  ScatterUpdate(m_v, [m | v]) (:616-734);
  ScatterSub(var, (lr_t m) / (epsilon + sqrt(v))),  lr_t = (lr sqrt(1 - beta2_power)) / (1 - beta1_power).

Every operation is one IEEE float32 rounding, like the kernels built with -ffp-contract=off.  lr_t, 1 - beta1 and
1 - beta2 are computed once in float32, as the host does.

Bookkeeping (the chain's, not the group optimizers'):
  slot table  row found, or inserted with the init rule and frequency word day << 16 | 1; an existing row's word gets one hit
              and the day; a blacklisted row reads as zeros and is left unwritten; flags from the row written;
  var table   row found, or inserted with the init rule and frequency word 1; an existing row's word is untouched; no
              enter-threshold filter; a blacklisted row is neither written nor un-blacklisted; flags from the row written.
"""
import numpy as np

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
  __slots__ = ("row", "freq", "black", "under")

  def __init__(self, row, freq, black=False):
    self.row, self.freq, self.black = np.asarray(row, F).copy(), int(freq), bool(black)
    self.under = True
    self.update_under()

  def update_under(self):
    """UpdateUnderThreshold (kv_variable.h:837-861): a blacklisted row is under; else every |element| below the cutoff."""
    self.under = True if self.black else bool(np.all(np.abs(self.row) < CUTOFF))

  def meta(self):
    """The record as kv_get_meta / OracleKv.meta report it."""
    return {"freq": self.freq & 0xFFFF, "day": self.freq >> 16, "blacklist": self.black, "under_threshold": self.under}


class Table(object):
  """key -> Row.  init_table [R, dim], seed: the init rule 0.5 (T[r1] + T[r2]) (kv_variable.h:889-898)."""

  def __init__(self, dim, init_table, seed=0, day=0, enter_threshold=0):
    self.dim, self.init_table, self.seed, self.day = int(dim), np.asarray(init_table, F), int(seed), int(day)
    self.enter_threshold = int(enter_threshold)          # carried for the tests' set-up: the step never reads it
    self.rows = {}

  def init_row(self, key):
    h = _mix64(((int(key) & M64) ^ ((self.seed * 0x9E3779B97F4A7C15) & M64)) & M64)
    R = self.init_table.shape[0]
    return ((self.init_table[(h & 0xFFFFFFFF) % R] + self.init_table[(h >> 32) % R]) * F(0.5)).astype(F)

  def hit(self, key, count=1):
    """AddFrequency(count, today) (embedding_value.h:189-193)."""
    r = self.rows[key]
    r.freq = (self.day << 16) | min((r.freq & 0xFFFF) + count, 65535)

  def lookup(self, keys):
    """What a training lookup of distinct keys leaves (GatherOrInsert, one hit each): the tests' set-up."""
    for k in (int(k) for k in keys):
      if k in self.rows:
        self.hit(k)
        self.rows[k].update_under()
      else:
        self.rows[k] = Row(self.init_row(k), (self.day << 16) | 1)

  def blacklist(self, key):
    """MarkBlacklist (table_manager.h:335-357): the row is given up and reads as zeros."""
    r = self.rows[int(key)]
    r.black, r.under, r.row = True, True, np.zeros(self.dim, F)

  def read(self, keys):
    return np.stack([self.rows[int(k)].row if int(k) in self.rows else np.zeros(self.dim, F) for k in keys])

  def metas(self, keys):
    return [self.rows[int(k)].meta() if int(k) in self.rows else None for k in keys]


def host_scalars(lr, beta1_power, beta2_power, beta1, beta2):
  """-> (lr_t, 1 - beta1, 1 - beta2) as kv_apply_adam computes them (fp32, in this order)."""
  lr_t = F(F(lr) * np.sqrt(F(1) - F(beta2_power))) / F(F(1) - F(beta1_power))
  return F(lr_t), F(F(1) - F(beta1)), F(F(1) - F(beta2))


def dedup_sum(ids, grad):
  """-> (unique ids in first-occurrence order, their gradient rows added one by one in occurrence order)."""
  ids = np.asarray(ids).reshape(-1)
  grad = np.asarray(grad, F).reshape(ids.size, -1)
  pos, uniq, sums = {}, [], []
  for i, k in enumerate(int(k) for k in ids):
    if k in pos:
      sums[pos[k]] = (sums[pos[k]] + grad[i]).astype(F)
    else:
      pos[k] = len(uniq); uniq.append(k); sums.append(grad[i].copy())
  return np.array(uniq, np.int64), np.stack(sums) if sums else np.zeros((0, grad.shape[1]), F)


def row_math(x, m, v, g, lr, beta1_power, beta2_power, beta1, beta2, epsilon):
  """The arithmetic on arrays of rows -> (var, m, v), one float32 rounding per operation."""
  x, m, v, g = (np.asarray(t, F) for t in (x, m, v, g))
  lr_t, omb1, omb2 = host_scalars(lr, beta1_power, beta2_power, beta1, beta2)
  b1, b2, eps = F(beta1), F(beta2), F(epsilon)
  m1 = b1 * m + g * omb1
  v1 = b2 * v + (g * g) * omb2
  x1 = x - (lr_t * m1) / (eps + np.sqrt(v1))
  return x1.astype(F), m1.astype(F), v1.astype(F)


def adam_step(var, slot, ids, grad, lr, beta1_power, beta2_power, beta1, beta2, epsilon):
  """One step on the two Table models, in place.  -> the unique ids in first-occurrence order."""
  D = var.dim
  assert slot.dim == 2 * D
  uniq, sums = dedup_sum(ids, grad)
  for k, g in zip((int(k) for k in uniq), sums):
    # GatherOrInsert(m_v): find_func / insert_func
    if k in slot.rows:
      slot.hit(k)
      slot.rows[k].update_under()
    else:
      slot.rows[k] = Row(slot.init_row(k), (slot.day << 16) | 1)
    s = slot.rows[k]
    mv = np.zeros(2 * D, F) if s.black else s.row
    # ScatterSub's insert comes before the op (kv_variable.h:713-730): the row the arithmetic starts from
    if k not in var.rows:
      var.rows[k] = Row(var.init_row(k), 1)
    r = var.rows[k]
    x1, m1, v1 = row_math(r.row[None], mv[None, :D], mv[None, D:], g[None], lr, beta1_power, beta2_power, beta1, beta2, epsilon)
    if not s.black:                                      # ScatterUpdate(m_v)
      s.row = np.concatenate([m1[0], v1[0]])
      s.update_under()
    if not r.black:                                      # ScatterSub(var)
      r.row = x1[0]
      r.update_under()
  return uniq
