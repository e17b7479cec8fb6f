"""tests/_size_cases.py on the CPU: the restated limits equal what the sources state, straddle_ids meets its classes for
every (chunk, tail) the GPU module uses, key_row is injective and never zero on every key set the GPU module uses, the
integer gradients sum exactly, adagrad_ref agrees with the oracle's Adagrad, and the oracle serves the longest
oracle-backed case in the time a GPU test can afford."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _size_cases as S  # noqa: E402

from oracle import kv_oracle as ko  # noqa: E402

torch = pytest.importorskip("torch")


def test_limits_match_the_sources():
  src = S.source_limits()
  assert src == {"FUSED_MAX_N": S.FUSED_MAX_N, "OTHER_DIM_MAX_N": S.OTHER_DIM_MAX_N, "LOOKUP_MAX_N": S.LOOKUP_MAX_N,
                 "SCATTER_CHUNK": S.SCATTER_CHUNK, "FOLD_CHUNK": S.SCATTER_CHUNK, "TILE": S.TILE}
  assert (S.FUSED_MAX_N, S.OTHER_DIM_MAX_N, S.SCATTER_CHUNK, S.LOOKUP_MAX_N, S.TILE) == (1 << 23, 1 << 21, 1 << 21, 1 << 30, 2048)
  # the dims on either side of the entry-list kernels, as kvhip.hip and kv_row_geom.h state them
  import _row_geometry as G
  assert G.class_of("entry", 256) is not None
  assert G.class_of("entry", S.NONFUSED_DIM) is None and G.class_of("entry", S.NONFUSED_DIM4) is None
  # 257: lookups, insert, export and import serve it (kvhip.h), the optimizer ops do not; 260 is the next dim they do
  assert S.NONFUSED_DIM == 257 and not G.dim_supported(S.NONFUSED_DIM) and S.NONFUSED_DIM in G.REFUSED
  assert G.dim_supported(S.NONFUSED_DIM4) and not any(G.dim_supported(D) for D in (258, 259))
  assert G.class_of("entry", 4) is not None and G.dim_supported(S.WIDE_DIM) and G.class_of("entry", S.WIDE_DIM) is None
  # the wide shape: the last two tiles wholly beyond element 2^31, bytes beyond 2^32 on the way
  assert (S.WIDE_N - 2 * S.TILE) * S.WIDE_DIM >= 1 << 31 and S.WIDE_N <= S.OTHER_DIM_MAX_N + S.WIDE_TAIL
  assert S.WIDE_N % S.TILE == 0


@pytest.fixture(scope="module", params=sorted(S.STRADDLES))
def straddle(request):
  return request.param, S.straddle_case(request.param)


def test_straddle_ids_meet_their_classes(straddle):
  name, s = straddle
  chunk, tail, bits = S.STRADDLES[name]
  ids = s["ids"]
  assert ids.dtype == np.int64 and ids.size == chunk + tail and ids.min() >= 1 and ids.max() < 1 << bits
  first, last = ids[:chunk], ids[chunk:]
  u1, u2 = np.unique(first), np.unique(last)
  assert np.union1d(u1, u2).size <= S.MAX_KEYS
  only1, both, only2 = np.setdiff1d(u1, u2), np.intersect1d(u1, u2), np.setdiff1d(u2, u1)
  assert np.array_equal(only1, np.sort(s["a"])) and s["a"].size >= 1000                      # (a)
  assert np.array_equal(both, np.sort(np.append(s["b"], s["d"])))                            # (b): d is one of them
  assert np.array_equal(only2, np.sort(s["c"])) and s["c"].size >= 1                         # (c)
  if tail > 1000:
    assert s["b"].size >= 1000 and s["c"].size >= 1000
  before, after = int((first == s["d"]).sum()), int((last == s["d"]).sum())                  # (d)
  assert before == S.FREQ_MAX - 1 < S.FREQ_MAX and after == 2 and before + after > S.FREQ_MAX
  assert s["e"] == (ids[chunk - 1], ids[chunk]) and s["e"][0] != s["e"][1]                    # (e)
  assert s["e"][0] in s["a"] and s["e"][1] in s["c"]            # neither occurs on the other side
  cnt = np.unique(ids, return_counts=True)[1]
  assert (cnt > S.FREQ_MAX).sum() >= 2 and (cnt < 100).sum() >= 1000     # keys that saturate inside one pass, and cold ones
  assert 3 * int(cnt.max()) < 1 << 24                            # |g| <= 3: every per-key sum is exact in fp32
  ck, names = S.class_keys(s)
  assert ck.dtype == np.int64 and ck.size == names.size == s["a"].size + s["b"].size + s["c"].size + 3
  assert np.array_equal(np.unique(ck), np.unique(ids))            # every key of the batch is read
  assert ck[-3] == s["d"] and list(names[-3:]) == ["d", "e[0]", "e[1]"] and names[0] == "a"


def test_integer_rows_sum_exactly():
  gen = torch.Generator().manual_seed(S.SEED)
  g = S.draw_int_rows(70000, 4, gen, "cpu")
  assert g.dtype == torch.float32 and set(g.unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
  fwd = torch.zeros(4)
  for blk in g.split(1000):                                      # another grouping, same fp32 sum
    fwd = fwd + blk.sum(0)
  assert torch.equal(fwd, g.double().sum(0).float()) and torch.equal(g.flip(0).cumsum(0)[-1], fwd)
  m = S.draw_int_rows(1000, 4, gen, "cpu", values=(1.0, 2.0, 0.5))
  assert set(m.unique().tolist()) == {0.5, 1.0, 2.0}


def _rows_injective(keys, D):
  rows = S.key_row(keys, D)
  assert rows.dtype == torch.float32 and rows.shape == (keys.numel(), D)
  assert torch.equal(rows, rows.round()) and rows.abs().max() <= 4096
  assert bool((rows != 0).any(1).all())                          # a zero-filled miss never passes
  dig = (rows[:, :4] + 4095).to(torch.int64)
  packed = dig[:, 0] | dig[:, 1] << 13 | dig[:, 2] << 26 | dig[:, 3] << 39
  assert torch.unique(packed).numel() == torch.unique(keys).numel() == keys.numel()
  return rows


def test_key_row_is_injective_on_every_key_set(straddle):
  name, s = straddle
  keys = torch.from_numpy(np.unique(s["ids"]))
  _rows_injective(keys, 4)


def test_key_row_on_the_distinct_and_wide_key_sets():
  rows = _rows_injective(S.distinct_keys(S.FUSED_MAX_N), 4)      # sections A.4 to A.7 use leading parts of these, B all
  assert torch.equal(rows[:5000], S.key_row(S.distinct_keys(5000), 4))
  _rows_injective(S.distinct_keys(S.WIDE_N), 4)                  # section C's distinct keys: elements 0..3 of the wide rows
  wide = _rows_injective(S.distinct_keys(S.WIDE_KEYS + S.WIDE_TAIL)[-300:], S.WIDE_DIM)
  assert torch.equal(wide[:, :8], S.key_row(S.distinct_keys(S.WIDE_KEYS + S.WIDE_TAIL)[-300:], 8))   # a prefix at every D
  assert torch.unique(wide[0]).numel() > 1000                    # a wide row is no repeat of four values
  chunked = S.key_row(S.distinct_keys(S.ROW_CHUNK + 5), 4)       # the chunked fill leaves no seam
  assert torch.equal(chunked[-5:], S.key_row(S.distinct_keys(5, start=S.ROW_CHUNK + 1), 4))
  into = torch.full((7, 4), 9.0)
  assert S.key_row(S.distinct_keys(7), 4, out=into) is into and torch.equal(into, rows[:7])


def test_adagrad_ref_agrees_with_the_oracle():
  """1e-6 relative on every element.  The fp32 step s = lr g / sqrt(acc') carries about 3 x 2^-24 |s| of rounding, the
  subtraction 2^-24 |x'|: relative to x' that is within 1e-6 wherever |s| < 4 |x'|.  Rows start at 1 <= |x| < 2 and
  |s| <= lr 3 / sqrt(0.1 + 9) < 0.05, so no element cancels — as in the GPU cases, whose rows are integers and |s| < 0.05."""
  rng = np.random.default_rng(S.SEED)
  D, n, lr = 8, 1000, 0.05
  ov = ko.OracleKv(D, 0, np.zeros((4, D), np.float32), day=20000, picker=1, seed=3)
  oa = ko.OracleKv(D, 0, np.full((4, D), 0.1, np.float32), day=20000, picker=1, seed=3)
  keys = S.draw_keys(rng, n)
  x0 = (rng.uniform(1, 2, (n, D)) * rng.choice([-1.0, 1.0], (n, D))).astype(np.float32)
  ov.insert(keys, x0)
  g = rng.integers(-3, 4, (n, D)).astype(np.float32)
  ko.apply_adagrad(ov, oa, lr, g, keys)
  x1, a1 = S.adagrad_ref(x0, np.full((n, D), np.float32(0.1)), g, lr)
  np.testing.assert_allclose(ov.gather_or_zeros(keys), x1, rtol=1e-6, atol=0)
  np.testing.assert_allclose(oa.gather_or_zeros(keys), a1, rtol=1e-6, atol=0)
  tx, ta = S.adagrad_ref(torch.from_numpy(x0), torch.full((n, D), 0.1), torch.from_numpy(g), lr)
  assert np.array_equal(tx.numpy(), x1) and np.array_equal(ta.numpy(), a1)      # the torch form: the same float64 step


def test_the_oracle_serves_the_longest_case_in_time():
  """the longest oracle-backed case (2 x 2^23 ids, dim 4, under 300 k keys): lookup, frequencies, de-duplication and
  the Adagrad step over its keys, each well inside what one GPU case may spend on its reference"""
  s = S.straddle_case("fused-x2")
  ids = s["ids"]
  table = np.arange(64 * 4, dtype=np.float32).reshape(64, 4)
  ov = ko.OracleKv(4, 0, table, day=20000, picker=1, seed=1)
  t0 = time.perf_counter()
  rows = ov.gather_or_insert(ids)
  t1 = time.perf_counter()
  cnt = ov.get_count(S.class_keys(s)[0])
  half = ids[:S.FUSED_MAX_N]
  u, sm, _ = ko.dedup_segment_sum(half, np.ones((half.size, 4), np.float32))
  t2 = time.perf_counter()
  print("oracle: lookup of %d ids %.2f s, dedup of %d ids %.2f s" % (ids.size, t1 - t0, half.size, t2 - t1))
  assert rows.shape == (ids.size, 4) and cnt.max() == S.FREQ_MAX and u.size <= S.MAX_KEYS
  # measured 1.8 s and 0.3 s; a GPU case can afford a few seconds.  A loaded host only warns; ten times that fails
  if t1 - t0 > 6.0 or t2 - t1 > 3.0:
    import warnings
    warnings.warn("the oracle took %.1f s + %.1f s on the longest size case (budget 6 s + 3 s)" % (t1 - t0, t2 - t1))
  assert t1 - t0 < 60.0 and t2 - t1 < 30.0
