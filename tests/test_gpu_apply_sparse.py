"""kv_apply_sparse / kv_multi_apply_sparse (include/kvhip.h): the optimizer apply straight from the segment gradients of the
sparse lookup against the composition it replaces — kv_lookup_sparse_grad, then the plain named op on (ids, values) — on twin
tables: bit for bit in deterministic mode, within the plain apply's own bars in the default mode."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _reorder  # noqa: E402
import _row_geometry as G  # noqa: E402
import _shard_apply_sparse_ref as A  # noqa: E402
import _sparse_grad_ref as R  # noqa: E402
from _radam_ref import HP as RADAM_HP  # noqa: E402
from tfplus_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
BATCH = G.draw_batch(np.random.default_rng(G.OPT_SEED))           # 2 172 ids: hot keys, cold keys of 1 .. 16 sources, tile sums
ADAM0 = (1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8)
FAM = {"group_adam_v4": ("group_adam", (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 1e-3, 1e-2, 2e-2, 4)),      # stem, scalars (_lib.OPT_FAMILIES)
       "group_adam_v3": ("group_adam", (0.05, 0.9, 0.999, 0.9, 0.999, 1e-8, 5e-5, 1e-2, 1e-3, 3)),
       "adagrad": ("adagrad", (0.05, True)), "sparse_group_ftrl": ("sparse_group_ftrl", (0.1, 1e-3, 1e-2, 1e-3, 1e-2, -0.5)),
       "ftrl_v2": ("ftrl_v2", (0.1, 1e-3, 1e-2, 1e-2, -0.5)), "group_ftrl_v2": ("group_ftrl_v2", (0.1, 1e-3, 1e-2, 1e-2, -0.5)),
       "group_radam": ("group_rectified_adam", (0.1, 0.9, 0.999, 0.9, 0.999, 1e-7, 1e-3, 1e-2, 1e-3, 0.4, True, False, False)),
       "adam": ("adam", (0.05,) + ADAM0[1:]), "plain_adam_v4": ("group_adam", ADAM0 + (0.0, 0.0, 0.0, 4)),
       "radam": ("rectified_adam", RADAM_HP),
       "group_amsgrad": ("group_amsgrad", (0.05, 0.9, 0.999, 0.9, 0.999, 1e-7, 1e-3, 0.01, 1e-3)),
       "group_adabelief": ("group_adabelief", (0.05, 0.9, 0.999, 0.9, 0.999, 1e-7, 1e-3, 0.01, 1e-3))}
CLASS_DIMS = sorted({min(d for d in range(4, 257, 4) if G.class_of("entry", d) == G.class_of("entry", D)) for D in range(4, 257, 4)})
DET_CASES = [(f, 32, "mean", np.int64, True) for f in G.ALL_FAMILIES] + \
            [(f, D, "mean", np.int64, True) for f in ("group_adam_v4", "adagrad", "adam") for D in CLASS_DIMS] + \
            [("adagrad", 32, c, t, w) for c in R.COMBINERS for t in (np.int32, np.int64) for w in (False, True)]


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _twin(ops, family, D, det, enter=G.ENTER, also=None):
  """[var, slot tables...] built identically every time; half of the batch's keys looked up before (half of those twice)"""
  vinit, sinits = G.inits(family.replace("plain_adam", "group_adam"), D, np.random.default_rng([7, D]))
  tabs = [ops.kv_variable([t.shape[1]], enter_threshold=enter if j == 0 else 0) for j, t in enumerate([vinit] + sinits)]
  for h, t in zip(tabs, [vinit] + sinits):
    ops.kv_set_clock_days(h, G.DAY)
    ops.kv_set_seed(h, 1)
    ops.init_kv_variable_v2(h, t)
  ops.kv_set_deterministic(tabs[0], det)
  for ids in (BATCH["pre"], also):
    if ids is not None:
      ops.kv_variable_gather_or_insert_v2(tabs[0], ids)
  return tabs


def _state(ops, tabs, keys=BATCH["keys"]):
  """everything the tables hold, in key order: rows (bits), blacklist, frequency words, sizes, flags"""
  out = []
  for h in tabs:
    k, v, bl, fk, fv = (t.cpu().numpy() for t in ops.kv_variable_export(h))
    o, of = np.argsort(k), np.argsort(fk)
    out += [k[o], v[o].view(np.uint32), np.sort(bl), fk[of], fv[of], np.array(ops.kv_variable_size_v2(h)),
            np.array([repr(m) for m in ops.kv_get_meta(h, keys)])]
  return out


def _same(a, b):
  return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _segments(rng, n):
  """ascending segment ids of n positions: lengths 0 (first, inside, trailing), 1 .. 70"""
  lens = [0]
  while sum(lens) < n:
    lens.append(min(n - sum(lens), int(rng.choice([0, 1, 1, 2, 5, 17, 64, 70]))))
  return np.repeat(np.arange(len(lens) + 2), lens + [0, 0]), len(lens) + 2


def _step(ops, family, tabs, fused, ids, sg, seg, w, nseg, combiner):
  stem, sc = FAM[family]
  if fused:
    return ops.kv_variable_apply_sparse(stem, tabs, sc, sg, ids, seg, w, nseg, combiner)
  vals = sg if seg is None else ops.kv_variable_lookup_sparse_grad(tabs[0], sg, seg, w, nseg, combiner)   # (seg None: plain values)
  ops._apply(stem, tabs, vals, ids, sc, False)


@pytest.mark.parametrize("family,D,combiner,seg_dtype,weighted", DET_CASES)
def test_deterministic_mode_is_the_composition_bit_for_bit(ops, family, D, combiner, seg_dtype, weighted):
  rng = np.random.default_rng([3, D])
  ids = BATCH["ids"]
  seg, nseg = _segments(rng, ids.size)
  w = rng.uniform(0.5, 1.5, ids.size).astype(F) if weighted else None
  twins = [_twin(ops, family, D, 1) for _ in range(2)]
  before = _state(ops, twins[0])
  for step in range(2):     # the second step meets existing rows, keys that were under the threshold, blacklisted rows
    sg = (rng.standard_normal((nseg, D)) * 3e-2).astype(F)
    for fused, tabs in zip((True, False), twins):
      _step(ops, family, tabs, fused, ids, sg, seg.astype(seg_dtype), w, nseg, combiner)
    after = _state(ops, twins[0])
    assert _same(after, _state(ops, twins[1])) and not _same(before, after)
    before = after


@pytest.mark.parametrize("family,D,exact", [("adagrad", 8, True), ("adagrad", 100, True), ("group_adam_v4", 32, True),
                                            ("adagrad", 32, False), ("adagrad", 132, False), ("plain_adam_v4", 32, False),
                                            ("plain_adam_v4", 132, False)])
def test_default_mode_against_the_oracle(ops, family, D, exact):
  """The 512-thread blocks.  exact: gradients every order sums exactly (_shard_apply_sparse_ref) — the deterministic twin's
  bits, and Adagrad's rows are the oracle's step on the float64 sums.  Else full-mantissa gradients, the oracle fed the
  EXPANDED gradients: Adagrad at the plain apply's bar (_row_geometry RTOL / ATOL), GroupAdam V4 without regularizers on
  fresh slots inside tests/_reorder.py's bound — every key: the multiset of terms is the plain apply's."""
  from oracle import kv_oracle as ko
  ids, seg, nseg, w, sg = (A.exact_inputs if exact else A.general_inputs)(A.SEEDS[0 if exact else 1], D)
  enter = 0 if family == "plain_adam_v4" else G.ENTER
  twins = [_twin(ops, family, D, det, enter=enter, also=ids) for det in ((0, 1) if exact else (0,))]
  keys = np.unique(ids)
  x0 = ops.kv_variable_gather_or_zeros_v2(twins[0][0], keys).cpu().numpy()
  for tabs in twins:
    _step(ops, family, tabs, True, ids, sg, seg, w, nseg, "sum")
  got = ops.kv_variable_gather_or_zeros_v2(twins[0][0], keys).cpu().numpy()
  assert not exact or _same(_state(ops, twins[0], keys), _state(ops, twins[1], keys))
  expanded = R.lookup_sparse_grad(sg, seg, w, nseg, "sum")
  if family == "adagrad":
    vinit, sinits = G.inits(family, D, np.random.default_rng([7, D]))
    ov, oa = ko.OracleKv(D, G.ENTER, vinit, day=G.DAY, picker=1, seed=1), ko.OracleKv(D, 0, sinits[0], day=G.DAY, picker=1, seed=1)
    for x in (BATCH["pre"], ids):
      ov.gather_or_insert(x)
    terms = A.per_id_terms(ids, sg, seg, w, nseg, "sum")
    s64, bnd, lr = A.sums64(terms), A.bounds(terms), FAM[family][1][0]
    u, s = (keys, np.stack([s64[int(k)] for k in keys]).astype(F)) if exact else ko.dedup_segment_sum(ids, expanded)[:2]
    ko.apply_adagrad(ov, oa, lr, s, u, True)
    # two float32 orders of one key's terms lie within 2 b of each other (b = _shard_apply_sparse_ref.bounds), and the step
    # x - lr g / sqrt(acc + g^2) moves by at most lr / sqrt(acc) per unit of g, acc >= the accumulator's initial value
    slack = 0.0 if exact else 2 * lr / np.sqrt(float(sinits[0][0, 0])) * np.stack([bnd[int(k)] for k in keys])
    ref = ov.gather_or_zeros(keys).astype(np.float64)
    assert np.all(np.abs(got - ref) <= G.RTOL * np.abs(ref) + G.ATOL[family][0] + slack)
  elif not exact:
    zero = np.zeros_like(x0)
    assert np.array_equal(_reorder.adam_reorder_check(x0, zero, zero, zero, ids, expanded, got, _reorder.adam_hp(*ADAM0[:3])), keys)


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("family", ["group_adam_v4", "sparse_group_ftrl"])
def test_batched_form_equals_the_single_table_calls(ops, family, empty):
  """two sparse tables of different lengths (one empty on request) and one that passes plain values"""
  D, rng = 32, np.random.default_rng(21)
  ins = []
  for ids, plain in ((BATCH["ids"], False), (G.draw_batch(np.random.default_rng(12))["ids"][:0 if empty else 700], False), (BATCH["ids"], True)):
    seg, nseg = _segments(rng, ids.size)
    ins.append((ids, (rng.standard_normal((ids.size if plain else nseg, D)) * 3e-2).astype(F), None if plain else seg,
                rng.uniform(0.5, 1.5, ids.size).astype(F), nseg))
  multi, single = ([_twin(ops, family, D, 1) for _ in ins] for _ in range(2))
  ops.kv_multi_apply_sparse(FAM[family][0], tuple(zip(*multi)), FAM[family][1], *[[i[j] for i in ins] for j in (1, 0, 2, 3, 4)], "mean")
  for tabs, (ids, sg, seg, w, nseg) in zip(single, ins):
    if ids.size:
      _step(ops, family, tabs, seg is not None, ids, sg, seg, w, nseg, "mean")
  assert all(_same(_state(ops, a), _state(ops, b)) for a, b in zip(multi, single))


def test_refusals_leave_the_tables_as_they_were(ops):
  n, nseg = 300, 100
  ids, seg = torch.arange(n, device="cuda") % 50, torch.arange(n, device="cuda") // 3
  hp = ops._hp_array(ADAM0)

  def call(tabs, sg, comb=1, dt=L.KV_DT_INT64, n=n, nseg=nseg, hp=hp, seg=seg):
    return L.lib().kv_apply_sparse(tabs[0].ptr, 7, tabs[1].ptr, None, hp, ops._p(sg), ops._p(ids), ops._p(seg), dt, None, n, nseg,
                                   comb, ops._stream(tabs[0]))

  tabs = _twin(ops, "adam", 32, 0)
  before, sg, m0 = _state(ops, tabs), torch.randn(nseg, 32, device="cuda"), ops.kv_variable_shape_v2(tabs[0])[0]
  for kw in (dict(sg=None), dict(comb=3), dict(dt=L.KV_DT_FLOAT), dict(nseg=0), dict(hp=ops._hp_array((0.0,) + ADAM0[1:])), dict(seg=None)):
    assert call(tabs, **dict(dict(sg=sg), **kw)) == L.KV_INVALID_ARGUMENT, kw
  assert call(tabs, sg, n=0) == L.KV_OK and _same(before, _state(ops, tabs))
  for D, mode in ((6, 0), (260, 0), (32, 2)):     # off the entry-list kernels: the dim, or occurrence-order mode
    off = _twin(ops, "adam", D, mode)
    b = _state(ops, off)
    assert call(off, torch.randn(nseg, D, device="cuda")) == L.KV_UNIMPLEMENTED and _same(b, _state(ops, off)), (D, mode)
  # a captured call that would have to grow the position records: refused with nothing queued, the capture stays valid
  torch.cuda.synchronize()
  s0, g0 = torch.cuda.Stream(), torch.cuda.CUDAGraph()
  s0.wait_stream(torch.cuda.current_stream())
  with torch.cuda.graph(g0, stream=s0):
    with pytest.raises(L.FailedPreconditionError, match="have to grow"):
      ops.kv_variable_apply_sparse("adam", tabs, FAM["adam"][1], sg, ids, seg, None, nseg, "mean")
  torch.cuda.synchronize()
  assert _same(before, _state(ops, tabs))
  ops.kv_variable_apply_sparse("adam", tabs, FAM["adam"][1], sg, ids, seg, None, nseg, "mean")      # outside: the buffers grow
  assert ops.kv_variable_shape_v2(tabs[0])[0] > m0


@pytest.mark.parametrize("which", ["group_adam", "adagrad", "pop", "occurrence", "occurrence_behind_the_handle"])
def test_python_training_step_with_fused_backward(ops, which):
  """embedding_lookup_sparse[_multi](fused_backward=True) over two features + one optimizer step, deterministic mode: the tables
  of the default backward, bit for bit — also where the second table is in occurrence-order mode (set through the Python op,
  or behind it: the op's refusal) and its step expands; a consumer that pops the gradients gets the default IndexedSlices"""
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import embedding_ops, kv_variable_ops, variable_scope
  kv_variable_ops.set_training(True)
  D, rng, feats, state = 16, np.random.default_rng(31), [], []
  for n in (900, 1300):
    seg, _ = _segments(rng, n)
    ind = np.stack([seg, np.zeros_like(seg)], 1)
    feats.append((embedding_ops.SparseTensor(ind, rng.integers(-150, 150, seg.size), [seg[-1] + 1, 8]),
                  embedding_ops.SparseTensor(ind, rng.uniform(0.5, 1.5, seg.size).astype(F), [seg[-1] + 1, 8])))
  for fused in (True, False):
    vs = [variable_scope.get_kv_variable("as/%s/%d/f%d" % (which, fused, f), embedding_dim=D,
                                         initializer=variable_scope.random_normal_initializer(seed=f)) for f in range(2)]
    opt = training.AdagradOptimizer(0.1) if which == "adagrad" else training.GroupAdamOptimizer(0.01)
    for v in vs:
      ops.kv_set_deterministic(v.handle, 1)
    if which == "occurrence":
      ops.kv_set_deterministic(vs[1].handle, 2)
    elif which.startswith("occurrence"):
      L.check(L.lib().kv_set_deterministic(vs[1].handle.ptr, 2))
    if which.startswith("occurrence"):   # (the batched lookup refuses an occurrence-order table: feature by feature)
      outs = [embedding_ops.embedding_lookup_sparse(v, a, b, combiner="mean", fused_backward=fused) for v, (a, b) in zip(vs, feats)]
    else:
      outs = embedding_ops.embedding_lookup_sparse_multi(vs, [a for a, _ in feats], [b for _, b in feats], combiner="mean",
                                                         fused_backward=fused)
    loss = sum(torch.nansum(o * torch.from_numpy(np.random.default_rng(40 + f).standard_normal(tuple(o.shape)).astype(F)).to(o.device))
               for f, o in enumerate(outs))
    if which == "pop":
      loss.backward()
      state.append([x.cpu().numpy().view(np.int32 if x.dtype == torch.float32 else np.int64) for v in vs for x in v.pop_gradients()[:2]])
      continue
    gv = opt.compute_gradients(loss, vs)
    assert all(isinstance(g, kv_variable_ops.DeferredSparseGrad) == fused for g, _ in gv)
    opt.apply_gradients(gv)
    state.append(sum((_state(ops, [v.handle, opt.get_slot(v, opt.get_slot_names()[0]).handle], keys=np.arange(-150, 150)) for v in vs), []))
  assert _same(*state)
