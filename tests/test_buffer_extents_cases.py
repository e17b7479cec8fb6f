"""tests/_extent_cases.py on the CPU: the closed forms tests/test_gpu_buffer_extents.py compares against are what the oracle
computes for the same sequence of ops, the sums they rest on are exact, and nothing a test expects equals a sentinel of
tests/_guarded.py (an expected sentinel would read as "not written")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _extent_cases as X  # noqa: E402
from _extent_cases import ABSENT, BLACK, PRESENT, UNDER, F  # noqa: E402
from oracle import kv_oracle as ko  # noqa: E402


def _prepared(pop, D, enter=X.ENTER):
  """the sequence test_gpu_buffer_extents.py runs to prepare a table, on the oracle"""
  o = ko.OracleKv(D, enter, X.init_table(D), day=X.DAY, picker=1, seed=1)
  b, p, u = pop.parts[BLACK], pop.parts[PRESENT], pop.parts[UNDER]
  o.import_(b, X.key_rows(b, D), blacklist=b)
  o.insert(p, X.key_rows(p, D))
  o.gather_or_insert(p)
  o.gather_or_insert(u)
  return o


def _same(got, want):
  """bit for bit; a NaN for a NaN (0/0 has no defined sign)"""
  assert got.dtype == want.dtype and got.shape == want.shape
  if got.dtype != np.float32:
    assert np.array_equal(got, want)
    return
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("key_dtype", ["int64", "int32", "uint64"])
def test_population(key_dtype):
  pop = X.Population(key_dtype)
  k = pop.parts.reshape(-1)
  assert np.unique(k).size == 4 * X.NKEYS
  if key_dtype == "int32":
    assert k.min() > 0 and k.max() < 2 ** 31
  if key_dtype == "uint64":
    assert (k < 0).all()                                   # the top bit
  for D in X.SMALL_DIMS:
    rows = X.key_rows(k, D)
    assert np.unique(rows, axis=0).shape[0] == k.size      # a row names its key
    assert np.abs(rows).max() <= 4096 and (rows != 0).any(axis=1).all()
    assert not X.holds_sentinel(rows)
  assert not X.holds_sentinel(pop.ids(k))
  rng = np.random.default_rng(1)
  for n in X.NS:
    ids = pop.draw(n, rng)
    assert ids.size == n and ids.dtype == X.NP_KEY[key_dtype] and pop.part_of(ids)[0] == PRESENT
    u = pop.draw(n, rng, (PRESENT, ABSENT, UNDER), unique=True)
    assert np.unique(u).size == n and pop.part_of(u)[0] == PRESENT and BLACK not in pop.part_of(u)
  ids = pop.draw(X.TILE + 1, rng)
  assert set(pop.part_of(ids)) == {0, 1, 2, 3} and np.unique(ids).size < ids.size


def test_init_row():
  for D in X.ROW_DIMS + X.WIDE_DIMS:
    c = X.init_row(D)
    assert (c != 0).all() and np.array_equal((c + c) * F(0.5), c) and not X.holds_sentinel(c)
    assert np.array_equal(X.init_table(D)[3], c)


@pytest.mark.parametrize("D", [4, 7, 100])
def test_rows_against_the_oracle(D):
  pop = X.Population("int64")
  o = _prepared(pop, D)
  rng = np.random.default_rng(D)
  ids = pop.draw(X.TILE + 1, rng)
  _same(o.gather_or_zeros(ids), pop.rows_read(ids, D))
  _same(o.get_count(ids), pop.counts(ids))
  _same(o.get_timestamp(ids), pop.days(ids))
  for k in (pop.parts[p][0] for p in (PRESENT, BLACK, UNDER)):
    m = o.meta(int(k))
    word = (m["day"] << 16) | m["freq"]
    flag = 0x80 | (1 if m["blacklist"] else 0) | (2 if m["under_threshold"] else 0)
    assert (word, flag) == (int(pop.freq_words([k])[0]), int(pop.flags([k])[0]))
  for arr in (pop.counts(ids), pop.days(ids), pop.freq_words(ids), pop.flags(ids)):
    assert not X.holds_sentinel(arr)
  # the export lists of the prepared table
  keys, values, black, fkeys, fvals = o.export(first_n=6)[:5]
  assert set(keys.tolist()) == set(pop.parts[PRESENT].tolist())             # under-threshold keys: frequency 1 < ENTER
  assert set(black.tolist()) == set(pop.parts[BLACK].tolist())
  assert set(fkeys.tolist()) == set(pop.parts[[PRESENT, BLACK, UNDER]].reshape(-1).tolist())
  _same(np.asarray(fvals, np.uint32), pop.freq_words(fkeys))
  keys2 = o.export(first_n=2)[0]
  assert set(keys2.tolist()) == set(pop.parts[[PRESENT, UNDER]].reshape(-1).tolist())
  # ... and the training lookup, which changes it
  _same(o.gather_or_insert(ids), pop.rows_lookup(ids, D))


@pytest.mark.parametrize("D", [4, 7])
@pytest.mark.parametrize("unique", [False, True])
def test_adagrad_step_against_the_oracle(D, unique):
  pop = X.Population("int64")
  ov = _prepared(pop, D)
  oa = ko.OracleKv(D, 0, X.init_table(D, X.ACC0), day=X.DAY, picker=1, seed=1)
  rng = np.random.default_rng([D, unique])
  parts = (PRESENT, ABSENT, BLACK, UNDER)
  ids, grad = X.apply_batch(pop, X.TILE + 1, rng, parts, unique)
  g = grad(D)
  assert ids.size == X.TILE + 1 and (np.unique(ids).size < ids.size) != unique
  x0 = ov.gather_or_insert(ids)                      # the step's lookup: absent keys enter with frequency 1 < ENTER
  _same(x0, pop.rows_lookup(ids, D))
  u, s, cnt = X.dedup(ids, g)
  assert cnt.max() <= 2 and set(np.unique(s).tolist()) <= {-4.0, 0.0, 4.0}
  assert ko.apply_adagrad(ov, oa, X.LR, s, u) in (0, None)
  xu = pop.rows_lookup(u, D)
  xu[pop.part_of(u) == BLACK] = 0                    # frequency 2 after the lookup: the blacklist is lifted, a zero row
  # (an absent key listed twice was counted twice by the lookup: it is over the threshold)
  want_x, want_a = X.adagrad_step(xu, s, (pop.part_of(u) == ABSENT) & (cnt == 1))
  _same(ov.gather_or_zeros(u), want_x)
  _same(oa.gather_or_zeros(u), want_a)
  assert not X.holds_sentinel(want_x) and not X.holds_sentinel(want_a)


def test_segments_and_sums_are_exact():
  rng = np.random.default_rng(3)
  for n in X.NS + (0,):
    seg, nseg = X.draw_segments(n, rng)
    assert seg.size == n and nseg >= 3 and (np.diff(seg) >= 0).all()
    ln = np.bincount(seg, minlength=nseg)
    assert ln[0] == 0 and ln[-1] == 0 and ln.max(initial=0) <= X.MAX_SEG and (n == 0 or (ln[1:-1] == 0).any())
    w = X.draw_weights(n, rng)
    rows = X.int_rows(n, 5, rng, values=(-4095, -7, 1, 4096))
    for combiner in (0, 1, 2):
      for wts in (None, w):
        out = X.combine(rows, seg, wts, nseg, combiner)          # asserts exactness itself
        empty = ln == 0
        if wts is not None and combiner:
          assert np.isnan(out[empty]).all()
        else:
          assert (out[empty] == 0).all()
        assert np.isfinite(out[~empty]).all() and not X.holds_sentinel(out)
        if n:
          sg = X.int_rows(nseg, 5, rng)
          assert not X.holds_sentinel(X.expand(sg, seg, wts, nseg, combiner))
  # a sum written out by hand
  rows = np.array([[1, 2], [3, 4], [5, 6]], F)
  seg = np.array([1, 1, 2])
  w = np.array([0.5, 2, 4], F)
  _same(X.combine(rows, seg, w, 4, 1), np.array([[np.nan] * 2, [6.5 / 2.5, 9 / 2.5], [5, 6], [np.nan] * 2], F))
  _same(X.combine(rows, seg, None, 4, 2)[1], (np.array([4, 6], F) / np.sqrt(F(2))))
  _same(X.expand(rows[:2].repeat(2, 0), seg, w, 4, 1)[0], F(0.5) / F(2.5) * np.array([1, 2], F))
  # unsorted segment sums: out-of-range ids are dropped, unnamed segments are zero rows
  for n in X.NS:
    nseg = max(4, n // 3)
    seg = rng.integers(-2, nseg + 2, n)
    assert np.bincount(seg[(seg >= 0) & (seg < nseg)], minlength=nseg).max() <= X.MAX_SEG
    X.segment_sum(X.int_rows(n, 3, rng), seg, nseg)


def test_owner_rules():
  ids = np.array([-7, -1, 0, 5, 1 << 40], np.int64)
  assert X.owners(ids, 4, 1).tolist() == [1, 3, 0, 1, 0]
  import _hash_keys
  assert X.owners(ids, 3, 0).tolist() == [(_hash_keys.hash_of(int(k)) >> 32) % 3 for k in ids]
