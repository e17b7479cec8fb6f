"""The de-duplicated path without a host round trip (include/kvhip.h kv_dedup_segment_sum_dev + kv_apply_unique_counted;
csrc/kv_uapply.h k_uapply_counted): the count of distinct ids stays on the device and the unique apply reads it there.
The chain lookup -> kv_dedup_segment_sum(sync=False) -> apply(unique_count=...) against the synchronous chain on a twin
(bit for bit) and against the oracle (1e-6); the count's edges around a wave's ids; int64 ids on an int32-key table; a count
outside 0 .. n_max (reported, nothing applied, never clamped); a broken uniqueness promise; what the op refuses; and that
neither call waits for the stream.
"""
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import kv_oracle as ko  # noqa: E402  (checker only)
from test_gpu_parity import _np, _beta_pows, _assert_same_table, RTOL, DAY  # noqa: E402
from test_gpu_unique_apply import _oracle, _tables, _same_bits  # noqa: E402
import test_gpu_group_radam as gr  # noqa: E402

N_MAX = 3000


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _count(c):
  return torch.tensor([c], dtype=torch.int64, device="cuda")


def _step(ops, name, hs, grad, ids, t, **how):
  """one optimizer step of `name` at step t; how: unique_indices=True or unique_count=<device tensor>"""
  b1p, b2p = _beta_pows(t)
  if name == "adam4":
    ops.kv_variable_group_sparse_apply_adam_v4(hs[0], hs[1], grad, ids, 0.05, b1p, b2p, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, **how)
  elif name == "adagrad":
    ops.kv_variable_sparse_apply_adagrad(hs[0], hs[1], 0.05, grad, ids, **how)
  elif name == "ftrl":
    ops.kv_variable_sparse_group_sparse_apply_ftrl_v2(hs[0], hs[1], hs[2], grad, ids, 0.05, 0.0, 0.0, 0.0, 0.0, -0.5, **how)
  else:
    ops.kv_variable_group_sparse_apply_rectified_adam(hs[0], hs[1], grad, ids, *gr._hp(t, tractable=True, amsgrad=True), **how)


def _twice_at_most(rng, universe=6000, distinct=2000, n=N_MAX):
  """n positions over `distinct` ids, none more than twice: a + b == b + a, so every order of summing gives the same bits"""
  u = rng.choice(universe, distinct, replace=False).astype(np.int64) - 500      # negative keys too
  ids = np.concatenate([u, u[:n - distinct]])
  rng.shuffle(ids)
  return ids


def _sync_chain(ops, name, hs, grad, ids, t):
  u, s, _ = ops.kv_dedup_segment_sum(hs[0], ids, grad)
  _step(ops, name, hs, s, u, t, unique_indices=True)


def _counted_chain(ops, name, hs, grad, ids, t):
  u, s, _, nu = ops.kv_dedup_segment_sum(hs[0], ids, grad, sync=False)
  assert u.numel() == ids.size and tuple(s.shape) == (ids.size, hs[0].dim) and nu.dtype == torch.int64 and nu.is_cuda
  _step(ops, name, hs, s, u, t, unique_count=nu)
  return nu


# ---- 1. chain equals chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 16, 32, 64, 128, 256])              # one per k_uapply geometry
@pytest.mark.parametrize("name", ["adam4", "adagrad", "ftrl", "radam"])
def test_counted_chain_equals_synchronous_chain_and_oracle(ops, name, D):
  rng = np.random.default_rng(900 + D)
  if name == "radam":
    init = gr._var_init(rng, D)
    hc, hs, os_ = gr._pair(ops, D, rng, init=init), gr._pair(ops, D, rng, init=init), None
  else:
    hc, hs, os_ = _tables(ops, name, D)
  seen = []
  for t in range(3):
    ids = _twice_at_most(rng)
    seen.append(ids)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(np.float32)
    # a training lookup in front, like a step; without one the op inserts the keys it meets first (the restatement that
    # checks group RectifiedAdam starts from rows that exist: a lookup in front of every step there)
    if t == 1 or name == "radam":
      for h in (hc[0], hs[0]):
        ops.kv_variable_gather_or_insert_v2(h, ids)
      if os_:
        os_[0].gather_or_insert(ids)
    uo, so, _ = ko.dedup_segment_sum(ids, grad)
    if name == "radam":                                   # the restatement, from the state the step starts from
      ex, metas, _ = gr._expect(ops, hs, uo, so, gr._hp(t, tractable=True, amsgrad=True))
    _sync_chain(ops, name, hs, grad, ids, t)
    nu = _counted_chain(ops, name, hc, grad, ids, t)
    assert int(nu.item()) == uo.size
    allk = np.concatenate(seen)
    for a, b in zip(hc, hs):
      _same_bits(ops, a, b, allk)
    if name == "radam":
      gr._check(ops, hc, uo, ex, metas)
    else:
      _oracle(name, os_, so, uo, lr=0.05, b1p=_beta_pows(t)[0], b2p=_beta_pows(t)[1])
      for h, o in zip(hc, os_):
        _assert_same_table(ops, h, o, allk, rtol=RTOL, atol=1e-7)


# ---- 2. the count's edges ---------------------------------------------------------------------------------------------------
def _edge_batch(D, seed=7):
  """N_MAX unique ids — half of them known to the table beforehand (`known`), half new — and their gradient rows"""
  rng = np.random.default_rng(seed)
  ids = rng.permutation(N_MAX * 2)[:N_MAX].astype(np.int64) * 3 - 1000
  known = ids[::2].copy()
  grad = rng.normal(0, 1e-2, (N_MAX, D)).astype(np.float32)
  return ids, known, grad


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1700, N_MAX])
@pytest.mark.parametrize("D", [4, 128])                                      # D = 4: 64 ids per wave and step
def test_count_edges_tail_is_never_touched(ops, D, count):
  hc, hp, _ = _tables(ops, "adam4", D)
  ids, known, grad = _edge_batch(D)
  for h in (hc[0], hp[0]):
    ops.kv_variable_gather_or_insert_v2(h, known)
  tail_keys = (1 << 40) + np.arange(N_MAX - count, dtype=np.int64)           # keys the table does not hold
  ids_c, grad_c = ids.copy(), grad.copy()
  ids_c[count:] = tail_keys
  grad_c[count:] = np.nan
  _step(ops, "adam4", hc, grad_c, ids_c, 0, unique_count=_count(count))
  _step(ops, "adam4", hp, grad[:count], ids[:count], 0, unique_indices=True)
  torch.cuda.synchronize()
  for a, b in zip(hc, hp):
    _same_bits(ops, a, b, np.concatenate([ids, known]))
  assert ops.kv_variable_size_v2(hc[0]) == known.size + int((~np.isin(ids[:count], known)).sum())
  if tail_keys.size:
    for h in hc:
      assert ops.kv_get_meta(h, tail_keys) == [None] * tail_keys.size
  assert np.isfinite(_np(ops.kv_variable_gather_or_zeros_v2(hc[0], ids))).all()


# ---- 3. int64 ids on an int32-key table ------------------------------------------------------------------------------------
def test_int32_key_table_takes_the_dedups_int64_ids(ops):
  D = 16
  rng = np.random.default_rng(21)
  init = rng.standard_normal((64, D)).astype(np.float32)
  twins = []
  for _ in range(2):
    hs = []
    for dim, tab in ((D, init), (D, np.full((16, D), 0.1, np.float32))):
      h = ops.kv_variable([dim], key_dtype=torch.int32)
      ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, 1); ops.init_kv_variable_v2(h, tab)
      hs.append(h)
    twins.append(hs)
  hc, hp = twins
  for t in range(2):
    ids = _twice_at_most(rng)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(np.float32)
    u, s, _, nu = ops.kv_dedup_segment_sum(hc[0], ids, grad, sync=False)
    assert u.dtype == torch.int64 and hc[0].key_dtype == torch.int32
    ops.kv_variable_sparse_apply_adagrad(hc[0], hc[1], 0.05, s, u, unique_count=nu)
    _sync_chain(ops, "adagrad", hp, grad, ids, t)
    for a, b in zip(hc, hp):
      _same_bits(ops, a, b, ids)
  # ... and int32 ids with KV_DT_INT32
  ids = np.arange(500, dtype=np.int32) * 5
  grad = rng.normal(0, 1e-2, (ids.size, D)).astype(np.float32)
  ops.kv_variable_sparse_apply_adagrad(hc[0], hc[1], 0.05, grad, torch.from_numpy(ids).cuda(), unique_count=_count(ids.size))
  ops.kv_variable_sparse_apply_adagrad(hp[0], hp[1], 0.05, grad, ids, unique_indices=True)
  for a, b in zip(hc, hp):
    _same_bits(ops, a, b, ids)


# ---- 4. a count outside 0 .. n_max ---------------------------------------------------------------------------------------------
def _snapshot(ops, hs, keys):
  return [(_np(ops.kv_variable_gather_or_zeros_v2(h, keys)).tobytes(), ops.kv_get_meta(h, keys), ops.kv_variable_size_v2(h),
           ops.kv_variable_frequency(h)) for h in hs]


@pytest.mark.parametrize("bad", [N_MAX + 1, -1])
def test_a_count_out_of_range_applies_nothing_and_is_reported(ops, bad):
  from tfplus_amd import _lib
  D = 32
  hc, _, _ = _tables(ops, "adam4", D)
  ids, known, grad = _edge_batch(D)
  ops.kv_variable_gather_or_insert_v2(hc[0], known)
  _step(ops, "adam4", hc, grad[::2], known, 0, unique_indices=True)          # slot rows exist too
  before = _snapshot(ops, hc, ids)
  _step(ops, "adam4", hc, grad, ids, 1, unique_count=_count(bad))           # queued: the device finds the count
  torch.cuda.synchronize()
  with pytest.raises(_lib.InvalidArgumentError, match="kv_apply_unique_counted"):
    ops.kv_variable_size_v2(hc[0])
  assert _snapshot(ops, hc, ids) == before                                   # the call after the report succeeds: nothing moved
  _step(ops, "adam4", hc, grad, ids, 1, unique_count=_count(N_MAX))         # and the table serves again
  torch.cuda.synchronize()
  assert ops.kv_variable_size_v2(hc[0]) == N_MAX


# ---- 5. the promise is still guarded -----------------------------------------------------------------------------------------------
def test_a_broken_promise_inside_the_count_is_reported(ops):
  from tfplus_amd import _lib
  D = 32
  hc, _, _ = _tables(ops, "adam4", D)
  ids, known, grad = _edge_batch(D)
  ops.kv_variable_gather_or_insert_v2(hc[0], known)
  ids = ids.copy()
  ids[1500] = ids[20]                                                        # both inside the count
  _step(ops, "adam4", hc, grad, ids, 0, unique_count=_count(1700))
  torch.cuda.synchronize()
  with pytest.raises(_lib.InvalidArgumentError, match="NOT unique"):       # error code 4
    ops.kv_variable_size_v2(hc[0])
  ids[1500] = ids[2000]                                                      # the same id twice, once beyond the count: no duplicate
  _step(ops, "adam4", hc, grad, ids, 1, unique_count=_count(1700))
  torch.cuda.synchronize()
  ops.kv_variable_size_v2(hc[0])


# ---- 6. what the op refuses -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 260])
def test_dims_off_the_one_launch_kernel_are_refused(ops, D):
  from tfplus_amd import _lib
  hc, _, _ = _tables(ops, "adagrad", D)
  ids = np.arange(200, dtype=np.int64) * 3
  grad = np.random.default_rng(5).normal(0, 1e-2, (ids.size, D)).astype(np.float32)
  ops.kv_variable_gather_or_insert_v2(hc[0], ids[:100])
  before = _snapshot(ops, hc, ids)
  with pytest.raises(_lib.UnimplementedError, match="kv_apply_unique_counted"):
    _step(ops, "adagrad", hc, grad, ids, 0, unique_count=_count(ids.size))
  torch.cuda.synchronize()
  assert _snapshot(ops, hc, ids) == before
  _step(ops, "adagrad", hc, grad, ids, 0, unique_indices=True)              # the exact form serves the dim (batch pipeline)


def test_refused_under_stream_capture_and_the_capture_survives(ops):
  from tfplus_amd import _lib
  D = 32
  hc, _, _ = _tables(ops, "adam4", D, cap=1 << 16)
  ids_np, known, grad_np = _edge_batch(D)
  ids, grad, cnt = torch.from_numpy(ids_np).cuda(), torch.from_numpy(grad_np).cuda(), _count(1700)
  _step(ops, "adam4", hc, grad, ids, 0, unique_count=cnt)                   # warmed: the same call outside a capture
  torch.cuda.synchronize()
  before = _snapshot(ops, hc, ids_np)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=side):                                     # refused before anything is queued
    with pytest.raises(_lib.UnimplementedError, match="stream capture"):
      _step(ops, "adam4", hc, grad, ids, 1, unique_count=cnt)
  torch.cuda.synchronize()                                                   # the capture ended validly
  assert _snapshot(ops, hc, ids_np) == before
  _step(ops, "adam4", hc, grad, ids, 1, unique_count=cnt)
  torch.cuda.synchronize()
  assert ops.kv_variable_size_v2(hc[0]) == 1700


# ---- 7. no host wait ---------------------------------------------------------------------------------------------------------------
def test_dedup_and_counted_apply_do_not_wait_for_the_stream(ops):
  if not hasattr(torch.cuda, "_sleep"):
    pytest.skip("torch.cuda._sleep is not available in this torch: the stream cannot be held busy")
  D = 32
  rng = np.random.default_rng(31)
  hc, hp, _ = _tables(ops, "adam4", D, cap=1 << 18)                          # ample capacity: no count refresh
  batches = []
  for _ in range(2):
    ids = _twice_at_most(rng)
    batches.append((torch.from_numpy(ids).cuda(), torch.from_numpy(rng.normal(0, 1e-2, (ids.size, D)).astype(np.float32)).cuda(), ids))
  ids, grad, ids_np = batches[0]
  _counted_chain(ops, "adam4", hc, grad, ids_np, 0)                          # warms the workspace, pairs var and slot
  _sync_chain(ops, "adam4", hp, grad, ids_np, 0)
  torch.cuda.synchronize()
  # cycles per millisecond of the spin kernel, measured, then some tens of ms of it
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record(); torch.cuda._sleep(2_000_000); ev[1].record(); ev[1].synchronize()
  per_ms = 2_000_000 / max(ev[0].elapsed_time(ev[1]), 1e-3)
  ids, grad, ids_np = batches[1]
  stream = torch.cuda.current_stream()
  torch.cuda.synchronize()
  torch.cuda._sleep(int(60 * per_ms))
  t0 = time.perf_counter()
  u, s, _, nu = ops.kv_dedup_segment_sum(hc[0], ids, grad, sync=False)
  _step(ops, "adam4", hc, s, u, 1, unique_count=nu)
  host_ms = (time.perf_counter() - t0) * 1e3
  busy = not stream.query()
  stream.synchronize()
  assert busy, "the two calls returned only after the stream had drained (%.1f ms on the host)" % host_ms
  _sync_chain(ops, "adam4", hp, grad, ids_np, 1)
  for a, b in zip(hc, hp):
    _same_bits(ops, a, b, np.concatenate([batches[0][2], ids_np]))
