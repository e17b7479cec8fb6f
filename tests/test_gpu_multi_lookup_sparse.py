"""kv_multi_lookup_sparse / kv_multi_lookup_sparse_grad: the sparse lookup and its backward over many tables, one launch
per stage.  Table i must get exactly what the single-table op gives a same-seed twin: output bits, key set, frequency
words and flags (forward, cold and warm), values bits (backward)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
DAY = 20000
NS = [0, 37, 2048 + 37, 5000]          # no ids, inside a tile, across a tile boundary, several tiles
WEIGHTED = [True, False, True, False]
COUNT_OCC = [False, True, False, True]


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _tables(ops, D, count=4, thr=3):
  hs = []
  for k in range(count):
    h = ops.kv_variable([D], enter_threshold=thr)
    ops.kv_set_clock_days(h, DAY)
    ops.kv_set_seed(h, 11 + k)
    ops.init_kv_variable_v2(h, np.random.default_rng(100 + k).standard_normal((32, D)).astype(np.float32))
    hs.append(h)
  return hs


def _batches(seed):
  """per table: ids (many repeats: frequencies pass the threshold of 3 for some keys only), ascending ragged segment ids
  with empty segments, weights or None, num_segments"""
  rng = np.random.default_rng(seed)
  out = []
  for n, weighted in zip(NS, WEIGHTED):
    nseg = max(3, n // 3)
    seg = np.sort(rng.integers(0, nseg - 1, n))                      # the last segment (at least) stays empty
    ids = rng.integers(-400, 400, n) * 7919
    w = rng.uniform(0.25, 2.0, n).astype(np.float32) if weighted else None
    out.append((ids, seg, w, nseg))
  return out


def _bits(t):
  return t.contiguous().view(torch.int32)


def _same_state(ops, a, b, ids):
  assert ops.kv_variable_size_v2(a) == ops.kv_variable_size_v2(b)
  assert ops.kv_variable_frequency(a) == ops.kv_variable_frequency(b)
  if len(ids):
    assert ops.kv_get_meta(a, ids) == ops.kv_get_meta(b, ids)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 20, 6])        # 6: the single-table path looped inside the call
@pytest.mark.parametrize("combiner,seg_dtype", [("mean", np.int64), ("sqrtn", np.int32), ("sum", np.int64)])
def test_batched_forward_equals_the_single_op_on_twins(ops, D, combiner, seg_dtype):
  batched, single = _tables(ops, D), _tables(ops, D)
  for call in range(2):                           # every key new, then a warm call with partly new keys
    bt = _batches(call)
    got = ops.kv_multi_lookup_sparse(batched, [b[0] for b in bt], [b[1].astype(seg_dtype) for b in bt], [b[2] for b in bt],
                                     [b[3] for b in bt], combiner, COUNT_OCC)
    for k, (ids, seg, w, nseg) in enumerate(bt):
      want = ops.kv_variable_lookup_sparse(single[k], ids, seg.astype(seg_dtype), w, nseg, combiner, COUNT_OCC[k])
      assert tuple(got[k].shape) == (nseg, D)
      assert torch.equal(_bits(got[k]), _bits(want)), (call, k)
      _same_state(ops, batched[k], single[k], ids)
    assert float(got[0].abs().sum()) == 0.0       # no ids: zero rows
  k, v = ops.read_kv_variable_op_v2(batched[3])   # the rows themselves (keys past the threshold), whatever row ids they got
  k2, v2 = ops.read_kv_variable_op_v2(single[3])
  o, o2 = torch.argsort(k), torch.argsort(k2)
  assert k.numel() > 0 and torch.equal(k[o], k2[o2]) and torch.equal(_bits(v[o]), _bits(v2[o2]))


@pytest.mark.gpu
def test_batched_forward_without_weights_and_counts(ops):
  """weights = None and count_occurrences = None as a whole"""
  batched, single = _tables(ops, 32, thr=0), _tables(ops, 32, thr=0)
  bt = _batches(5)
  got = ops.kv_multi_lookup_sparse(batched, [b[0] for b in bt], [b[1] for b in bt], None, [b[3] for b in bt], "mean")
  for k, (ids, seg, _, nseg) in enumerate(bt):
    want = ops.kv_variable_lookup_sparse(single[k], ids, seg, None, nseg, "mean", False)
    assert torch.equal(_bits(got[k]), _bits(want))
    _same_state(ops, batched[k], single[k], ids)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 20, 6])
@pytest.mark.parametrize("combiner,seg_dtype", [("mean", np.int32), ("sqrtn", np.int64), ("sum", np.int32)])
def test_batched_backward_equals_the_single_op(ops, D, combiner, seg_dtype):
  hs = _tables(ops, D)
  bt = _batches(9)
  rng = np.random.default_rng(D)
  grads = [rng.standard_normal((b[3], D)).astype(np.float32) for b in bt]
  got = ops.kv_multi_lookup_sparse_grad(hs, grads, [b[1].astype(seg_dtype) for b in bt], [b[2] for b in bt],
                                        [b[3] for b in bt], combiner)
  for k, (ids, seg, w, nseg) in enumerate(bt):
    want = ops.kv_variable_lookup_sparse_grad(hs[k], grads[k], seg.astype(seg_dtype), w, nseg, combiner)
    assert tuple(got[k].shape) == (NS[k], D)
    assert torch.equal(_bits(got[k]), _bits(want)), k
  assert all(ops.kv_variable_size_v2(h) == 0 for h in hs)            # the tables only lend their workspaces


@pytest.mark.gpu
def test_batched_ops_refuse_what_the_other_batched_ops_refuse(ops):
  from tfplus_amd import _lib
  a, b = _tables(ops, 32, count=2)
  other = _tables(ops, 16, count=1)[0]
  ids, seg = np.arange(8), np.repeat(np.arange(4), 2)
  fwd = lambda hs: ops.kv_multi_lookup_sparse(hs, [ids] * 2, [seg] * 2, None, [4, 4], "sum")
  bwd = lambda hs: ops.kv_multi_lookup_sparse_grad(hs, [np.zeros((4, h.dim), np.float32) for h in hs], [seg] * 2, None,
                                                   [4, 4], "sum")
  for f in (fwd, bwd):
    with pytest.raises(_lib.InvalidArgumentError, match="listed twice"):
      f([a, a])
    with pytest.raises(_lib.InvalidArgumentError, match="dim"):
      f([a, other])
  occ = _tables(ops, 32, count=1)[0]
  ops.kv_set_deterministic(occ, ops.KV_ORDER_OCCURRENCE)
  for f in (fwd, bwd):
    with pytest.raises(_lib.UnimplementedError):
      f([a, occ])
  with pytest.raises(ValueError):
    ops.kv_multi_lookup_sparse([a, b], [ids] * 2, [seg] * 2, None, [4, 4], "max")
  with pytest.raises(_lib.InvalidArgumentError):
    ops.kv_multi_lookup_sparse([a, b], [ids] * 2, [seg[:3], seg], None, [4, 4], "sum")
  with pytest.raises(_lib.InvalidArgumentError):
    ops.kv_multi_lookup_sparse([a, b], [ids], [seg] * 2, None, [4, 4], "sum")
  assert ops.kv_variable_size_v2(a) == 0 and ops.kv_variable_size_v2(b) == 0    # nothing ran
  assert [tuple(t.shape) for t in fwd([a, b])] == [(4, 32)] * 2
