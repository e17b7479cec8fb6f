"""kv_lookup_sparse_grad, the native backward of the fused sparse lookup, bit for bit against the float32 restatement
tests/_sparse_grad_ref.py (which tests/test_sparse_grad_ref.py holds against torch autograd on the CPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sparse_grad_ref as R  # noqa: E402

N = 5000


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _table(ops, D, init=True):
  h = ops.kv_variable([D])
  if init:
    ops.init_kv_variable_v2(h, np.random.default_rng(D).standard_normal((16, D)).astype(np.float32))
  return h


def _ragged():
  """5000 positions: empty segments first, in the middle and last; lengths 1, 5, 7 and 600; the segment of length 5 has
  weights that sum to exactly 0."""
  rng = np.random.default_rng(7)
  lens = [0, 0, 1, 5, 7, 600, 0]
  while sum(lens) < N:
    lens.append(int(min(rng.integers(0, 10), N - sum(lens))))
  lens += [0, 0]
  lens = np.array(lens)
  seg = np.repeat(np.arange(lens.size), lens)
  w = rng.uniform(0.25, 2.0, N).astype(np.float32)
  w[1:6] = [1.0, -1.0, 2.0, -2.0, 0.0]
  return seg, w, lens.size


def _more_segments_than_positions():
  rng = np.random.default_rng(8)
  return np.sort(rng.integers(0, 7000, N)), rng.uniform(0.25, 2.0, N).astype(np.float32), 7000


def _one_segment():
  return np.zeros(N, np.int64), np.random.default_rng(9).uniform(0.25, 2.0, N).astype(np.float32), 1


SHAPES = {"ragged": (_ragged, np.int64), "sparse": (_more_segments_than_positions, np.int32), "one": (_one_segment, np.int64)}
_cache = {}


def _shape(name):
  if name not in _cache:
    seg, w, nseg = SHAPES[name][0]()
    _cache[name] = (seg, w, nseg, {})
  return _cache[name]


def _scale(name, weighted, combiner):
  """the restatement's scales of a shape: computed once, shared by every dim"""
  seg, w, nseg, sc = _shape(name)
  if (weighted, combiner) not in sc:
    sc[(weighted, combiner)] = R.scales(seg, w if weighted else None, nseg, combiner)
  return sc[(weighted, combiner)]


def _seg_grad(seg, nseg, D, seed):
  g = np.random.default_rng(seed).standard_normal((nseg, D)).astype(np.float32)
  empty = np.ones(nseg, bool)
  empty[seg] = False
  g[empty] = np.nan                                   # rows of empty segments are never read: no NaN may come out
  return g


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 20, 32, 256, 6])
@pytest.mark.parametrize("combiner", R.COMBINERS)
@pytest.mark.parametrize("weighted", [False, True])
def test_grad_is_bit_equal_to_the_restatement(ops, D, combiner, weighted):
  h = _table(ops, D)
  for name, (_, seg_dtype) in SHAPES.items():
    seg, w, nseg, _ = _shape(name)
    w = w if weighted else None
    g = _seg_grad(seg, nseg, D, D + nseg)
    got = ops.kv_variable_lookup_sparse_grad(h, g, seg.astype(seg_dtype), w, nseg, combiner)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, D)
    want = R.lookup_sparse_grad(g, seg, w, nseg, combiner, scale=_scale(name, weighted, combiner))
    zero_den = weighted and combiner == "mean" and name == "ragged"
    assert np.isnan(want).any() == zero_den           # NaN only from the zero denominator, never from an empty segment's row
    assert R.same_bits(got.cpu().numpy(), want, nan_ok=zero_den), (name, D, combiner, weighted)


@pytest.mark.gpu
@pytest.mark.parametrize("seg_dtype", [np.int32, np.int64])
def test_grad_both_segment_dtypes_same_input(ops, seg_dtype):
  seg, w, nseg, _ = _shape("ragged")
  h = _table(ops, 20)
  g = _seg_grad(seg, nseg, 20, 1)
  got = ops.kv_variable_lookup_sparse_grad(h, g, seg.astype(seg_dtype), w, nseg, "sqrtn").cpu().numpy()
  assert R.same_bits(got, R.lookup_sparse_grad(g, seg, w, nseg, "sqrtn", scale=_scale("ragged", True, "sqrtn")))


@pytest.mark.gpu
def test_grad_without_positions_or_segments(ops):
  h = _table(ops, 8)
  out = ops.kv_variable_lookup_sparse_grad(h, np.zeros((5, 8), np.float32), np.zeros(0, np.int64), None, 5, "mean")
  assert tuple(out.shape) == (0, 8)
  from tfplus_amd import _lib
  one = torch.zeros(8, device="cuda")
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = ctypes.c_void_p(one.data_ptr())
  assert _lib.lib().kv_lookup_sparse_grad(h.ptr, p, p, _lib.KV_DT_INT64, None, 0, 5, 1, p, st) == _lib.KV_OK
  assert _lib.lib().kv_lookup_sparse_grad(h.ptr, None, None, _lib.KV_DT_INT64, None, 3, 0, 1, None, st) == _lib.KV_OK   # no-op
  torch.cuda.synchronize()
  assert float(one.abs().sum()) == 0.0


@pytest.mark.gpu
def test_grad_argument_errors(ops):
  from tfplus_amd import _lib
  h = _table(ops, 8)
  g = np.zeros((2, 8), np.float32)
  with pytest.raises(ValueError):
    ops.kv_variable_lookup_sparse_grad(h, g, [0, 1], None, 2, "max")
  with pytest.raises(_lib.InvalidArgumentError):
    ops.kv_variable_lookup_sparse_grad(h, g, [0, 1], [1.0], 2, "sum")               # weights of another length
  with pytest.raises(_lib.InvalidArgumentError):
    ops.kv_variable_lookup_sparse_grad(h, g, [0, 1], None, 3, "sum")                # seg_grad has not num_segments rows
  # the C entry point's own checks (all made before anything is read or queued)
  buf = torch.zeros(64, device="cuda")
  p, st = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  f = _lib.lib().kv_lookup_sparse_grad
  i64 = _lib.KV_DT_INT64
  assert f(None, p, p, i64, None, 2, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT        # null handle
  assert f(h.ptr, p, p, i64, None, 2, 2, 3, p, st) == _lib.KV_INVALID_ARGUMENT       # combiner
  assert f(h.ptr, p, p, _lib.KV_DT_FLOAT, None, 2, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT   # segment dtype
  assert f(h.ptr, p, p, i64, None, -1, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT
  assert f(h.ptr, p, p, i64, None, (1 << 23) + 1, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT    # the per-call limit of kv_lookup_sparse
  assert f(h.ptr, p, p, i64, None, 2, -1, 1, p, st) == _lib.KV_INVALID_ARGUMENT
  assert f(h.ptr, None, p, i64, None, 2, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT    # null pointers
  assert f(h.ptr, p, None, i64, None, 2, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT
  assert f(h.ptr, p, p, i64, None, 2, 2, 1, None, st) == _lib.KV_INVALID_ARGUMENT
  assert f(_table(ops, 6).ptr, p, p, i64, None, (1 << 21) + 1, 2, 1, p, st) == _lib.KV_INVALID_ARGUMENT   # ... of the other dims
  with pytest.raises(_lib.FailedPreconditionError):
    ops.kv_variable_lookup_sparse_grad(_table(ops, 8, init=False), g, [0, 1], None, 2, "sum")
  torch.cuda.synchronize()
  assert float(buf.abs().sum()) == 0.0


@pytest.mark.gpu
def test_grad_leaves_the_table_alone(ops):
  h = _table(ops, 32)
  ids = np.arange(100, 400)
  ops.kv_variable_gather_or_insert_v2(h, np.concatenate([ids, ids[:50]]))
  rows = ops.kv_variable_gather_or_zeros_v2(h, ids)
  before = (ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h), ops.kv_get_meta(h, [100, 399, 7]))
  seg, w, nseg, _ = _shape("ragged")
  ops.kv_variable_lookup_sparse_grad(h, _seg_grad(seg, nseg, 32, 2), seg, w, nseg, "mean")
  assert (ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h), ops.kv_get_meta(h, [100, 399, 7])) == before
  assert before[2][0]["freq"] == 2 and before[2][2] is None          # (a key that is there, and one that is not)
  assert torch.equal(ops.kv_variable_gather_or_zeros_v2(h, ids), rows)


@pytest.mark.gpu
def test_grad_replays_in_a_graph(ops):
  """One call outside the capture (the workspace grows there), then the captured call replayed on new gradients."""
  seg, w, nseg, _ = _shape("ragged")
  D = 32
  h = _table(ops, D)
  dev = torch.device("cuda", 0)
  segt, wt = torch.from_numpy(seg).to(dev), torch.from_numpy(w).to(dev)
  g = torch.from_numpy(_seg_grad(seg, nseg, D, 3)).to(dev)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ops.kv_variable_lookup_sparse_grad(h, g, segt, wt, nseg, "sqrtn")
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    out = ops.kv_variable_lookup_sparse_grad(h, g, segt, wt, nseg, "sqrtn")
  sc = _scale("ragged", True, "sqrtn")
  for rep in range(2):
    new = _seg_grad(seg, nseg, D, 10 + rep)
    g.copy_(torch.from_numpy(new).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu().numpy(), R.lookup_sparse_grad(new, seg, w, nseg, "sqrtn", scale=sc))
