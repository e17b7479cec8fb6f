"""The yardstick of the fused sharded sparse apply (kvhip.h kv_shard_apply_route_sparse), on the CPU: which terms the record
of a distinct id receives, what they sum to, and how far any float32 order of adding them can be from that.

  term_j = fl(scale_j * seg_grad[s_j, :])          tests/_sparse_grad_ref.lookup_sparse_grad: the row the expansion writes
  record(id) = the sum of term_j over the id's positions j, in the pre-sum's order

Bound.  The terms are rounded products — data, as far as the sum is concerned.  m float32 additions-in-some-order of m numbers
t_1 .. t_m differ from their exact sum by at most gamma_(m-1) sum|t_i|, gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy
and Stability of Numerical Algorithms, section 4.2: any summation order); gamma_(m-1) <= m u as long as m (m - 1) u <= 1, i.e.
m <= 4096 (asserted).  So every element lies within m 2^-24 sum|term| of the float64 sum; an id that occurs once within 0.
No measured figure is involved.

Exact inputs.  Segment gradients that are integers in [-8, 8] times _row_geometry.GQ, the combiner `sum`, weights None or
drawn from {0.5, 1, 2}: every product is an integer times GQ / 2 below 2^5, every partial sum of up to 4096 of them an integer
times GQ / 2 below 2^17 — all exact in float32, so every order of the additions gives the same bits, the float64 sum's.

The batches of tests/test_gpu_shard_apply_sparse.py are drawn here, so that tests/test_shard_apply_sparse_ref.py can hold
these conditions on the CPU for the very seeds the GPU test uses."""
import numpy as np

import _row_geometry as G
import _sparse_grad_ref as R

F = np.float32
TILE = G.TILE
N = 2 * TILE + 37
SEEDS = (11, 12, 13)             # rank r of a case draws with SEEDS[r]
U = 2.0 ** -24
ZERO_SUM_SEGMENT = 6


def lanes(D):
  """lanes per row of the row-copy kernels (row_lanes): the segment lengths below straddle it"""
  return G._pow2ceil(max(1, D // 4))


def draw_ids(seed):
  """[N] int64: _row_geometry.draw_batch's multiplicity plan (singles, in-tile repeats, cold and hot keys, a 300- and a
  500-fold key) in the first tile and a bit, padded to N with further occurrences of its keys — so that repeats straddle both
  tile boundaries and a key has a tile sum in more than one tile."""
  rng = np.random.default_rng(seed)
  b = G.draw_batch(rng)
  ids = b["ids"].astype(np.int64)
  assert TILE < ids.size < N
  rep = b["keys"][b["counts"] >= 2].astype(np.int64)
  pad = rep[rng.integers(0, rep.size, N - ids.size)]
  return np.concatenate([ids, pad])


def layout(D, rng, n=N):
  """(segment ids [n] ascending, num_segments): tests/test_gpu_shard_lookup_sparse._layout's lengths — 0 (first, middle, last,
  trailing), 1, L - 1, L, L + 1, 4 L + 3, one of 2 100 positions across the first tile boundary, the rest 1 .. 8; segment
  ZERO_SUM_SEGMENT (4 L + 3 positions) is the one whose weights sum to zero."""
  L = lanes(D)
  lens = [0, 1, L - 1, L, 0, L + 1, 4 * L + 3]
  while sum(lens) < 1000:
    lens.append(int(rng.integers(1, 9)))
  lens.append(2100)
  assert sum(lens[:-1]) < TILE < sum(lens) and sum(lens) < n
  while sum(lens) < n:
    lens.append(min(n - sum(lens), int(rng.integers(1, 9))))
  lens.append(0)
  nseg = len(lens) + 3
  seg = np.repeat(np.arange(len(lens)), lens)
  assert seg.size == n and lens[ZERO_SUM_SEGMENT] >= 2
  return seg.astype(np.int64), nseg


def general_inputs(seed, D):
  """(ids, seg, nseg, weights, seg_grad): full-mantissa segment gradients, weights of one sign except the zero-sum segment
  (weights 1.5, -1.5, the rest 0: mean and sqrtn divide by zero there — 0 / 0 and x / 0 as IEEE gives them)"""
  ids = draw_ids(seed)
  rng = np.random.default_rng(1000 + seed * 7 + D)
  seg, nseg = layout(D, rng)
  w = rng.uniform(0.1, 2.0, N).astype(F)
  at = np.flatnonzero(seg == ZERO_SUM_SEGMENT)
  w[at] = 0.0
  w[at[0]], w[at[1]] = 1.5, -1.5
  seg_grad = (rng.standard_normal((nseg, D)) * 1e-2).astype(F)
  return ids, seg, nseg, w, seg_grad


def exact_inputs(seed, D):
  """(ids, seg, nseg, weights, seg_grad) for the combiner `sum`: see the module docstring"""
  ids = draw_ids(seed)
  rng = np.random.default_rng(2000 + seed * 7 + D)
  seg, nseg = layout(D, rng)
  w = np.array([0.5, 1.0, 2.0], F)[rng.integers(0, 3, N)]
  seg_grad = (rng.integers(-8, 9, (nseg, D)) * G.GQ).astype(F)
  return ids, seg, nseg, w, seg_grad


def per_id_terms(ids, seg_grad, seg, weights, nseg, combiner):
  """{id: [term_j for the id's positions j, in position order]}, each term a float32 row — bit for bit the values row of
  kv_lookup_sparse_grad (segment ids clamped into [0, nseg) as the op clamps them)"""
  seg = np.clip(np.asarray(seg).astype(np.int64), 0, nseg - 1)
  values = R.lookup_sparse_grad(seg_grad, seg, weights, nseg, combiner)
  out = {}
  for j, k in enumerate(np.asarray(ids).tolist()):
    out.setdefault(int(k), []).append(values[j])
  return out


def sums64(terms):
  """{id: float64 sum of its terms}"""
  with np.errstate(invalid="ignore"):                             # (inf - inf where a scale is x / 0)
    return {k: np.sum(np.asarray(t, np.float64), axis=0) for k, t in terms.items()}


def bounds(terms):
  """{id: per element, m 2^-24 sum|term| for its m terms (0 for an id that occurs once)}"""
  out = {}
  for k, t in terms.items():
    m = len(t)
    assert m * (m - 1) * U <= 1.0
    with np.errstate(invalid="ignore"):                           # (0 * inf for an id that occurs once in a zero-sum segment)
      out[k] = (m * U if m > 1 else 0.0) * np.sum(np.abs(np.asarray(t, np.float64)), axis=0)
  return out


def sum32(rows, order):
  """float32 sum of the rows in the given order, one addition at a time from the first row"""
  acc = np.asarray(rows[order[0]], F).copy()
  for i in order[1:]:
    acc = (acc + np.asarray(rows[i], F)).astype(F)
  return acc
