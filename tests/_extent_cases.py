"""The inputs and the closed forms of tests/test_gpu_buffer_extents.py (tests/test_buffer_extents_cases.py checks this file
on the CPU: the forms against the oracle, the sums' exactness, no value equal to the sentinel of tests/_guarded.py).

Every expected value is computed here in numpy from the inputs alone, with no second GPU run:
  rows         a key held by kv_insert reads _size_cases.key_row(key, D): integers in [-4095, 4096], every element a function
               of key and element index; the init table's rows are all init_row(D), so a key a training lookup inserts reads
               0.5 (c + c) = c; a blacklisted key reads zeros
  Population   the four kinds of key a prepared table holds: present, absent, blacklisted (imported on the blacklist), and —
               on a table with enter_threshold = ENTER — under the threshold (inserted by ONE training lookup)
  sums         segment lengths <= 64, |element| <= 4096, weights powers of two in [1/2, 4]: every partial sum is an integer
               multiple of 1/2 below 2^24, exact in float32 in any order, and a product plus an add is the fused multiply-add
  mean, sqrtn  one IEEE division (sqrtf first) in float32, as numpy takes it
  Adagrad      summed gradients in {-4, 0, 4}, accumulator rows 48, lr = 1/2: 48 + 16 = 64, 1 / sqrt(64) = 1/8 — the float32
               step and _size_cases.adagrad_ref in float64 are the same number, x -+ 1/4 or x
"""
import numpy as np

import _hash_keys
import _size_cases as S
from _guarded import SENT_BYTE, SENT_F32
from _row_geometry import DIMS, REFUSED, TILE, draw_batch  # noqa: F401  (re-exported for the tests)

F = np.float32
SEED = 20251021
DAY = 20000
ENTER = 2
NKEYS = 704                              # keys per part: a unique list of TILE + 1 ids fits in three parts
NS = (1, 65, TILE - 1, TILE + 1)         # one id, one row past a wave, one row on either side of a tile
SMALL_DIMS = (4, 100)                    # the ops that write no rows
WIDE_DIMS = (257, 1028)                  # outside the fused range: lookups, insert, assign, export / import
ROW_DIMS = tuple(DIMS)
MAX_SEG = 64
PRESENT, ABSENT, BLACK, UNDER = 0, 1, 2, 3
ACC0, LR = 48.0, 0.5
NP_KEY = {"int64": np.int64, "int32": np.int32, "uint64": np.int64}      # uint64 keys travel as their int64 pattern


def init_row(D):
  """c: never zero, exact, another value in (nearly) every element"""
  e = np.arange(D)
  return ((e * 37) % 101 - 50 + 0.25).astype(F)


def init_table(D, value=None):
  return np.tile(init_row(D) if value is None else np.full(D, value, F), (4, 1))


def key_rows(keys, D):
  import torch
  return S.key_row(torch.from_numpy(np.asarray(keys).astype(np.int64)), D).numpy()


class Population:
  """parts[PRESENT | ABSENT | BLACK | UNDER]: NKEYS distinct keys each, as int64 patterns"""

  def __init__(self, key_dtype="int64", seed=0):
    rng = np.random.default_rng([SEED, seed, sorted(NP_KEY).index(key_dtype)])
    if key_dtype == "int32":
      k = S.draw_keys(rng, 4 * NKEYS, bits=31)
    elif key_dtype == "uint64":          # the top bit set: negative as int64
      k = (S.draw_keys(rng, 4 * NKEYS, bits=62).astype(np.uint64) | np.uint64(1 << 63)).view(np.int64)
    else:
      k = S.draw_keys(rng, 4 * NKEYS, bits=40)
      k[::5] = -k[::5]
    self.key_dtype = key_dtype
    self.parts = k.reshape(4, NKEYS)
    order = np.argsort(k)
    self._sorted, self._part = k[order], (np.arange(4 * NKEYS) // NKEYS)[order]

  def part_of(self, ids):
    ids = np.asarray(ids).astype(np.int64)
    at = np.searchsorted(self._sorted, ids)
    assert np.array_equal(self._sorted[at], ids)
    return self._part[at]

  def ids(self, a):
    return np.ascontiguousarray(np.asarray(a).astype(NP_KEY[self.key_dtype]))

  def draw(self, n, rng, parts=(PRESENT, ABSENT, BLACK, UNDER), unique=False):
    """n ids from `parts`, the first one present; repeated ids unless unique"""
    pool = np.concatenate([self.parts[p] for p in parts])
    if unique:
      assert n <= pool.size
      out = rng.permutation(pool)[:n]
    else:
      out = pool[rng.integers(0, pool.size, n)]
    if PRESENT in parts and n:
      first = self.parts[PRESENT][0]
      if unique and first in out:
        out[np.flatnonzero(out == first)[0]] = out[0]
      out[0] = first
    return self.ids(out)

  def rows(self, ids, D, absent, under):
    """absent / under: "zeros" or "init" — what those parts read"""
    part = self.part_of(ids)
    out = key_rows(ids, D)
    c = init_row(D)
    out[part == BLACK] = 0
    for p, what in ((ABSENT, absent), (UNDER, under)):
      out[part == p] = c if what == "init" else 0
    return out

  def rows_read(self, ids, D):
    """kv_gather_or_zeros on the prepared table"""
    return self.rows(ids, D, "zeros", "init")

  def rows_lookup(self, ids, D):
    """a training lookup on the prepared table"""
    return self.rows(ids, D, "init", "init")

  # frequency, day and flags on the prepared table (present keys: inserted, then looked up once on DAY)
  def counts(self, ids):
    return np.array([2, 0, 1, 1], np.int32)[self.part_of(ids)]

  def days(self, ids):
    return np.array([DAY, DAY, 0, DAY], np.uint32)[self.part_of(ids)]      # absent: today

  def freq_words(self, ids):
    return np.array([(DAY << 16) | 2, 0, 1, (DAY << 16) | 1], np.uint32)[self.part_of(ids)]

  def flags(self, ids):
    return np.array([0x80, 0, 0x83, 0x80], np.uint8)[self.part_of(ids)]


FLAG_BITS = 0x83                          # what kvhip.h defines of a flags byte: blacklist, under_threshold, present


# ---- segments --------------------------------------------------------------------------------------------------------------
def draw_segments(n, rng, max_len=8):
  """(segment ids [n] ascending, num_segments): lengths 1..max_len, the first, the last and one inner segment empty"""
  lens = []
  while sum(lens) < n:
    lens.append(int(rng.integers(1, max_len + 1)))
  if lens:
    lens[-1] -= sum(lens) - n
  lens = [0] + lens[:len(lens) // 2] + [0] + lens[len(lens) // 2:] + [0]
  return np.repeat(np.arange(len(lens)), lens).astype(np.int64), len(lens)


def draw_weights(n, rng):
  return np.array([0.5, 1, 2, 4], F)[rng.integers(0, 4, n)]


def seg_stats(seg, w, nseg):
  """(length, float32 sum of w, float32 sum of w^2) per segment; w None: ones"""
  w = np.ones(seg.size, F) if w is None else w
  ln = np.bincount(seg, minlength=nseg)[:nseg]
  ws = np.bincount(seg, weights=w.astype(np.float64), minlength=nseg)[:nseg]
  w2 = np.bincount(seg, weights=w.astype(np.float64) ** 2, minlength=nseg)[:nseg]
  assert np.array_equal(ws.astype(F), ws) and np.array_equal(w2.astype(F), w2)
  return ln, ws.astype(F), w2.astype(F)


def _den(ws, w2, combiner):
  return ws if combiner == 1 else np.sqrt(w2)


def combine(rows, seg, w, nseg, combiner):
  """embedding_lookup_sparse: out [nseg, D]; an empty segment is a zero row, weighted mean / sqrtn 0/0"""
  ln, ws, w2 = seg_stats(seg, w, nseg)
  acc = np.zeros((nseg, rows.shape[1]), np.float64)
  np.add.at(acc, seg, rows.astype(np.float64) * (1.0 if w is None else w.astype(np.float64)[:, None]))
  out = acc.astype(F)
  assert np.array_equal(out, acc) and np.abs(acc).max(initial=0) < 2 ** 24
  if combiner:
    div = (ln > 0) | (w is not None)
    with np.errstate(invalid="ignore", divide="ignore"):
      out[div] = out[div] / _den(ws, w2, combiner)[div, None]
  return out


def expand(seg_grad, seg, w, nseg, combiner):
  """the backward: values[j] = scale_j * seg_grad[seg[j]], the scale one IEEE division, each element one multiply"""
  ln, ws, w2 = seg_stats(seg, w, nseg)
  wj = np.ones(seg.size, F) if w is None else w
  scale = wj if combiner == 0 else wj / _den(ws, w2, combiner)[seg]
  return (scale[:, None] * seg_grad[seg]).astype(F)


def int_rows(n, D, rng, values=(-3, -2, -1, 1, 2, 3)):
  return np.array(values, F)[rng.integers(0, len(values), (n, D))]


def segment_sum(data, seg, nseg):
  """tf.unsorted_segment_sum: ids outside [0, nseg) are dropped"""
  ok = (seg >= 0) & (seg < nseg)
  acc = np.zeros((nseg, data.shape[1]), np.float64)
  np.add.at(acc, seg[ok], data[ok].astype(np.float64))
  assert np.abs(acc).max(initial=0) < 2 ** 24
  return acc.astype(F)


def dedup(ids, rows):
  """{id: summed row}, and {id: occurrences}"""
  u, inv, cnt = np.unique(np.asarray(ids).astype(np.int64), return_inverse=True, return_counts=True)
  s = segment_sum(rows, inv, u.size) if rows is not None else None
  return u, s, cnt


# ---- owners ----------------------------------------------------------------------------------------------------------------
def owners(ids, world, rule):
  ids = np.asarray(ids).astype(np.int64)
  if rule == 0:
    return ((_hash_keys.hashes(ids) >> np.uint64(32)) % np.uint64(world)).astype(np.int64)
  return np.mod(ids, world)


# ---- the Adagrad step ------------------------------------------------------------------------------------------------------
def apply_batch(pop, n, rng, parts, unique):
  """(ids [n], grad [n, *] as a function of D): unique ids, or some of them listed twice; a key's summed gradient is -4, 0 or 4
  in every element"""
  if unique or n < 4:
    ids, twice = pop.draw(n, rng, parts, unique=True), 0
  else:
    twice = n // 4
    once = pop.draw(n - twice, rng, parts, unique=True)
    ids = np.concatenate([once, once[:twice]])
    rng.shuffle(ids)
  def grad(D):
    g = np.array([-4, 0, 4], F)[rng.integers(0, 3, (n, D))]
    u, inv, cnt = np.unique(ids.astype(np.int64), return_inverse=True, return_counts=True)
    rep = cnt[inv] == 2
    g[rep] = np.array([-2, 2], F)[rng.integers(0, 2, (int(rep.sum()), D))]
    return g
  return ids, grad


def adagrad_step(x, gsum, skip):
  """(x', acc') in float32 from _size_cases.adagrad_ref; rows of `skip` keep x and have no accumulator row (read as zeros)"""
  acc = np.full_like(x, ACC0)
  x2, acc2 = S.adagrad_ref(x, acc, gsum, LR)
  x2f, acc2f = x2.astype(F), acc2.astype(F)
  assert np.array_equal(x2f, x2) and np.array_equal(acc2f, acc2)
  # the float32 sequence of the op itself, x - (lr g) (1 / sqrt(acc')), gives the same number
  with np.errstate(invalid="ignore"):
    mine = x - (F(LR) * gsum) * (F(1) / np.sqrt(acc2f))
  assert np.array_equal(mine.astype(F), x2f)
  x2f[skip], acc2f[skip] = x[skip], 0
  return x2f, acc2f


def holds_sentinel(a):
  """whether an expected array holds the sentinel of its type in any element"""
  a = np.ascontiguousarray(a)
  if a.dtype == np.float32:
    return bool((a.view(np.uint32) == SENT_F32).any())
  return bool((a.view(np.uint8).reshape(a.size, a.dtype.itemsize) == SENT_BYTE).all(axis=1).any())
