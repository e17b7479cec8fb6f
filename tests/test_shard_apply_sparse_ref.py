"""tests/_shard_apply_sparse_ref.py held to its own claims, without a GPU, for the seeds and dims the GPU test uses: the batches
have the shape the kernels' paths need, the "exact" inputs really are exact (every product, and a float32 sum in three
different orders, equals the float64 sum), the per-id terms are the expansion's rows, and the bound is the stated one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _row_geometry as G  # noqa: E402
import _shard_apply_sparse_ref as A  # noqa: E402
import _sparse_grad_ref as R  # noqa: E402

DIMS = (4, 8, 12, 32, 64, 100, 256)


@pytest.mark.parametrize("seed", A.SEEDS)
def test_batches_cover_the_paths(seed):
  ids = A.draw_ids(seed)
  assert ids.size == A.N == 2 * G.TILE + 37
  keys, counts = np.unique(ids, return_counts=True)
  assert (counts == 1).sum() >= 50 and counts.max() >= 300                     # singles and a hot key
  tiles = [set(ids[t * G.TILE:(t + 1) * G.TILE].tolist()) for t in range(3)]
  assert len(tiles[0] & tiles[1]) > 20 and len(tiles[1] & tiles[2]) > 5        # repeats straddle both tile boundaries
  in_tile = [np.unique(ids[t * G.TILE:(t + 1) * G.TILE], return_counts=True)[1] for t in range(2)]
  assert all((c >= 2).sum() > 20 for c in in_tile)                             # tile sums in both full tiles
  assert (ids > (1 << 32)).any() and (ids < 0).any()


@pytest.mark.parametrize("D", DIMS)
def test_layout_has_the_segments_the_issue_names(D):
  seg, nseg = A.layout(D, np.random.default_rng(D))
  lens = np.bincount(seg, minlength=nseg)
  assert seg.size == A.N and np.all(np.diff(seg) >= 0)
  assert lens[0] == 0 and lens[4] == 0 and lens[-1] == 0 and lens[nseg - 4] == 0   # empty: first, middle, last, trailing
  big = int(np.argmax(lens))
  first = int(np.flatnonzero(seg == big)[0])
  assert lens[big] == 2100 and first < G.TILE < first + 2100                   # one segment across a tile boundary
  assert lens[A.ZERO_SUM_SEGMENT] == 4 * A.lanes(D) + 3


@pytest.mark.parametrize("D", (4, 100))
@pytest.mark.parametrize("seed", A.SEEDS)
def test_exact_inputs_are_exact_in_every_order(seed, D):
  ids, seg, nseg, w, sg = A.exact_inputs(seed, D)
  rng = np.random.default_rng(seed)
  for weights in (None, w):
    terms = A.per_id_terms(ids, sg, seg, weights, nseg, "sum")
    ww = np.ones(A.N) if weights is None else weights.astype(np.float64)
    prod64 = sg.astype(np.float64)[seg] * ww[:, None]
    flat = np.concatenate([np.asarray(terms[k]) for k in dict.fromkeys(ids.tolist())])
    order = np.concatenate([np.flatnonzero(ids == k) for k in dict.fromkeys(ids.tolist())])
    assert np.array_equal(flat.astype(np.float64), prod64[order])              # every product is exact
    s64 = A.sums64(terms)
    for k, t in terms.items():
      m = len(t)
      for o in (list(range(m)), list(range(m))[::-1], rng.permutation(m).tolist()):
        assert np.array_equal(A.sum32(t, o).astype(np.float64), s64[k]), (k, m)


@pytest.mark.parametrize("combiner", R.COMBINERS)
def test_terms_are_the_expansions_rows_and_the_bound_is_the_stated_one(combiner):
  ids, seg, nseg, w, sg = A.general_inputs(A.SEEDS[0], 8)
  values = R.lookup_sparse_grad(sg, seg, w, nseg, combiner)
  terms = A.per_id_terms(ids, sg, seg, w, nseg, combiner)
  assert sum(len(t) for t in terms.values()) == A.N
  for k in (int(ids[0]), int(ids[-1]), int(ids[G.TILE])):
    at = np.flatnonzero(ids == k)
    assert R.same_bits(np.asarray(terms[k]), values[at], nan_ok=True)
  b, s64 = A.bounds(terms), A.sums64(terms)
  nan_ids = 0
  for k, t in terms.items():
    m = len(t)
    a = np.asarray(t, np.float64)
    if not np.isfinite(a).all():
      nan_ids += 1
      continue
    if m == 1:
      assert not b[k].any() and np.array_equal(s64[k], a[0])
      continue
    assert np.allclose(b[k], m * 2.0 ** -24 * np.abs(a).sum(0), rtol=1e-12, atol=0)
    # a float32 sum in position order and in reverse: both inside the bound
    for o in (list(range(m)), list(range(m))[::-1]):
      assert np.all(np.abs(A.sum32(t, o).astype(np.float64) - s64[k]) <= b[k])
  assert (nan_ids > 0) == (combiner == "mean")                                 # the zero-sum segment: 0 / 0 under mean only


def test_out_of_range_segment_ids_are_clamped_as_the_op_clamps_them():
  ids = np.array([5, 5, 7, 9])
  sg = np.arange(6, dtype=np.float32).reshape(3, 2)
  terms = A.per_id_terms(ids, sg, np.array([-4, 0, 2, 70000]), None, 3, "sum")
  assert np.array_equal(np.asarray(terms[5]), sg[[0, 0]]) and np.array_equal(terms[7][0], sg[2]) and np.array_equal(terms[9][0], sg[2])
