"""Every kernel dispatch class against the oracle: the row-geometry matrix.

Each kernel family picks its instantiation from the embedding dim (tests/_row_geometry.py class_of restates the seven
dispatch tables; tests/test_row_geometry.py holds the restatement against the sources).  This module runs every class of
every table at its smallest dim, its largest dim and a dim that leaves a lane or a k vector partly masked (DIMS), on one
batch that reaches every branch of the apply kernels (draw_batch: cold keys of 1..16 occurrences, hot keys of one and of
several chunks, a key in both tiles), and compares with oracle.kv_oracle and tests/_kv_model.py — never with another GPU
path.

  a. row movement    training lookups (plain, with counts), gather_or_zeros, the batched gather over three dims, insert,
                     export -> import -> export after kv_reserve has rehashed the table, scatter_update with every
                     operation: bit for bit (DIV: unique ids, rtol 1e-6);
  b. sparse lookups  kv_lookup_sparse (three combiners, with and without weights), its backward, kv_lookup_sparse_zeros:
                     the bounds of tests/_sparse_zeros_ref.py, the bits of tests/_sparse_grad_ref.py;
  c. optimizers      eight families x every dim x every apply form the library offers for the dim (plain, with the lookup's
                     token, unique; counted for the multiples of 4 up to 256; batched over two tables for every multiple of
                     4), three steps with the state carried, regularizers on so that some rows blacklist (or zero) and
                     some do not.  One reference trajectory per (family, dim) serves all forms (_row_geometry.trajectory);
  d. occurrence order  kv_set_deterministic(h, 2): the sorted pipeline with k_occ_sum at one dim per NC class and its edges;
                     the sums bit for bit;
  e. refused dims    which ops refuse a dim outside the fused kernels' range with KV_UNIMPLEMENTED and nothing changed,
                     and which serve it and match the oracle (SERVED / REFUSING below; include/kvhip.h kv_create).

Classes no test had run before this module (the suite's dims were 1, 5, 6, 7, 8, 12, 16, 20, 32, 64, 100, 128, 256, 260):
  sorted apply      scalar rows (1,16,1), (1,32,1), (1,64,1), (1,64,2), (1,64,4) — dims 9..255 that are no multiple of 4 —
                    and (1,2,1), (1,4,1) at dims 2, 3; float4 (4,64,4) at 516..1024; (4,64,2) with a full row (512); every
                    k_apply_fin launch from dim 576 up, where the block's LDS passes 64 KB and the launcher asks for it;
  entry-list apply  (4,8,2) and (4,64,1) with masked vectors (dims 36, 60 and 132, 252), next to row copies that use
                    another lane count for the same dim (36: 16 lanes in k_ltile, 8 x 2 in k_papply);
  group optimizers  every family with its regularizers on at every class (before: GroupAdam at dim 32, SparseGroupFtrl at 1,
                    16, 32, group FTRL-V2 and group RAdam at one masked dim, nothing above 256);
  gather            k_gather VQ = 128, 256 (dims 512, 1024), the generic body above 260;
  occurrence order  k_occ_sum<8> and <16> (dims 260..1024);
  sparse zeros      the whole-wave body (VQ = 0) up to its limit of dim 1024.
Two arithmetic-only edits of the group norm in opt_core (kv_device.h, shared by the three apply kernels) show where the
matrix bites.  With the last k vector left out of the sum this module failed 317 cases, at exactly the dims whose last k
vector holds row elements (36, 60, 64, 65, 68, 124, 127, 128, 254, 255, 260, 508, 512, 1020, 1024); the rest of the suite
noticed at dim 64 alone (16 cases).  With 1.0 added for every masked lane it failed 536 cases, at every dim of DIMS that is
not its class's full width (3, 5, 7, 9, 12, ... 576, 1020); the rest of the suite noticed at dims 7 and 12 (19 cases).

Bars: ids, flags, frequency words, counters exact; rows rtol 1e-6 with the atol of the family's own test file; a var that
went through a group norm (1e-6 / scale) |x| + atol per row, rows whose scale is within 1e-4 of the threshold skipped (at
least 99 % of the keys are compared: asserted here and, on the reference alone, in tests/test_row_geometry.py).  A var
element outside that bar must be within max(bar, 4 x ref_err x bar) of the same step in float64, ref_err being the float32
reference's own distance from the float64 step ON THAT ROW in units of the row's bar (largest element), measured on the CPU.
What ref_err measures is mostly not the order of the norm's sum — it does not grow with the dim — but the step's own
float32 roundings (linear', the clamp's difference, scale, the division), which at scale near 1 are a few ulps against a
bar of 1e-6: GroupAdam's is past 1 from dim 4 up.  The kernel makes the same roundings as the reference, so the first,
unwidened comparison is the one that normally holds.

GroupAdam (both versions) between two steps: linear' = linear + alpha m - coef var reads the var the step before left, which
is within its bar of the reference's, not on it, and with coef = (sqrt(v') - sqrt(v)) / lr (version 3) that difference comes
back in linear' larger than linear''s own bar: compared with the reference's trajectory as it stands, group_adam_v3 at dim 127
has, at the third step, one element of one key at 2.33e-10 from the reference's against a bar of 1.87e-10 (1.25 x), dim 572
three elements of one key.  The bars are per step from the same state (tests/test_gpu_occurrence_order.py REG_RTOL says so
of its own), so after a step has been checked its rows are set to the reference's bits (_align: ASSIGN, exact) and the
next step starts where the reference's does.  No bar is widened for it; frequency words, blacklist and flags are never
touched and stay carried on the device.

ref_err, the largest over a case's rows and its three steps, per dim (tests/test_row_geometry.py prints it with -s):

  dim    group_adam_v4  group_adam_v3  sparse_group_ftrl  group_ftrl_v2  group_radam
     1      0.505          0.348           0.405           0.0218         0.607
     2       0.55          0.441           0.634           0.0124         0.136
     3      0.466          0.866           0.842           0.0155         0.116
     4       1.03           1.03           0.426           0.0145         0.124
     5       1.11           1.38           0.715           0.0154         0.596
     7       1.55            1.5           0.899           0.0172         0.172
     8       1.36           2.16           0.857           0.0177          0.16
     9        1.2            1.9           0.295           0.0168         0.167
    12       1.28           1.09           0.745           0.0215         0.221
    15       1.61           2.15           0.631           0.0176         0.197
    16       1.32           2.18           0.746           0.0189         0.151
    17        1.4           2.15           0.434            0.017         0.184
    20       1.42           1.81           0.667           0.0208         0.178
    31       2.04           1.66           0.795           0.0206         0.236
    32        1.3           2.57            0.37           0.0118         0.183
    33       1.97            2.2           0.395           0.0193         0.212
    36       1.96           1.77           0.771           0.0157         0.413
    60       1.39           2.89           0.829           0.0174         0.172
    63       6.25           2.64            0.48           0.0155         0.208
    64       2.72           2.99           0.786           0.0163         0.226
    65       3.86           1.43            1.02             0.02         0.164
    68       1.77           1.87           0.945           0.0219          1.88
   124       2.33           2.19           0.701           0.0198          2.85
   127       2.77           2.83           0.839           0.0191         0.208
   128       3.18           2.08           0.989           0.0146         0.305
   129        3.9           3.24               1           0.0179         0.476
   132       2.15            1.7            1.27           0.0167         0.216
   252       5.99           2.71           0.676           0.0204         0.223
   254       3.93           3.65            1.06           0.0227         0.195
   255       2.69            3.2           0.602           0.0195         0.196
   256        3.5           3.29           0.816           0.0228         0.182
   260       3.77            2.9           0.985           0.0218          0.21
   508       2.83           3.43            1.23           0.0238         0.239
   512       3.86           2.79            1.13           0.0243             3
   516       6.42           2.97            1.02           0.0227          0.39
   572       2.67           2.44            1.06           0.0205         0.282
   576       2.97           2.59           0.887           0.0233         0.311
  1020       3.21           3.65            1.26           0.0195         0.464
  1024       3.04           4.19            1.52           0.0184         0.262
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _row_geometry as G  # noqa: E402
import _sparse_grad_ref as GR  # noqa: E402
import _sparse_zeros_ref as ZR  # noqa: E402
from oracle import kv_oracle as ko  # noqa: E402  (checker only)

F = np.float32
DAY = G.DAY


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _np(t):
  return t.detach().cpu().numpy()


def _table(ops, D, init, thr=0, seed=0, kd=np.int64, cap=64):
  h = ops.kv_variable([D], enter_threshold=thr, capacity_hint=cap, key_dtype=torch.int32 if np.dtype(kd) == np.int32 else torch.int64)
  ops.kv_set_clock_days(h, DAY)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, init)
  return h


def _pair(ops, D, thr=0, seed=0, kd=np.int64, cap=64):
  init = np.random.default_rng([D, seed]).standard_normal((32, D)).astype(F)
  return _table(ops, D, init, thr, seed, kd, cap), ko.OracleKv(D, thr, init, day=DAY, picker=1, seed=seed)


def _same_table(ops, h, o, keys):
  """rows, frequency words and flags of `keys`, and the table-wide counters: equal."""
  keys = np.unique(np.asarray(keys)).astype(np.int64)
  np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_zeros_v2(h, keys)), o.gather_or_zeros(keys))
  for k, m in zip(keys, ops.kv_get_meta(h, keys)):
    assert m == o.meta(int(k)), (int(k), m, o.meta(int(k)))
  assert (ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)) == \
      (o.map_size(), o.size(), o.sum_freq())


# one int32 dim per class of the row copies and of the sorted apply's scalar rows
INT32_DIMS = [1, 3, 7, 15, 31, 63, 127, 255, 4, 8, 12, 20, 36, 68, 132, 260, 516, 1024]
MOVE = [(D, np.int64) for D in G.DIMS] + [(D, np.int32) for D in INT32_DIMS]


def _sorted_export(ops, h):
  k, v, bl, fk, fv = (_np(t) for t in ops.kv_variable_export(h, first_n=6))
  o, fo = np.argsort(k), np.argsort(fk)
  return k[o], v[o], np.sort(bl), fk[fo], fv[fo].view(np.uint32)


def _same_export(ex, o):
  """ex (_sorted_export) holds what the oracle table exports: keys, rows, blacklist, frequency keys and words."""
  ok_, ov_, obl, ofk, ofv = o.export(first_n=6)
  oo, fo = np.argsort(ok_), np.argsort(ofk)
  for got, want in zip(ex, (ok_[oo], ov_[oo], np.sort(obl), ofk[fo], ofv[fo])):
    np.testing.assert_array_equal(got, want)


def _import_pair(ops, D, ex, thr, seed):
  """A fresh GPU table and a fresh oracle table, both filled by importing the export `ex`."""
  init = np.zeros((1, D), F)
  h2 = _table(ops, D, init, thr=thr, seed=seed)
  o2 = ko.OracleKv(D, thr, init, day=DAY, picker=1, seed=seed)
  ops.kv_variable_import(h2, ex[0], ex[1], ex[2], ex[3], ex[4], first_n=6)
  o2.import_(ex[0], ex[1], ex[2], ex[3], ex[4], first_n=6)
  return h2, o2


# ---- a. row movement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kd", MOVE, ids=["%d-%s" % (D, np.dtype(kd).name) for D, kd in MOVE])
def test_row_movement(ops, D, kd):
  assert D in G.DIMS
  rng = np.random.default_rng([D, 1])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[D % len(G.SEEDS)]), kd)
  ids, keys = b["ids"], b["keys"]
  h, o = _pair(ops, D, thr=G.ENTER, seed=3, kd=kd)
  misses = (keys[:20].astype(np.int64) + 7).astype(kd)
  probe = np.concatenate([ids, misses])

  def lookups():
    np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_v2(h, ids)), o.gather_or_insert(ids))
    counts = rng.integers(1, 40000, ids.size).astype(np.int32)
    np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_with_counts(h, ids, counts)), o.gather_or_insert(ids, counts))
    np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_zeros_v2(h, probe)), o.gather_or_zeros(probe))
    _same_table(ops, h, o, probe)

  np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_v2(h, b["pre"])), o.gather_or_insert(b["pre"]))
  lookups()
  # insert: existing rows overwritten, new keys created
  ins = np.concatenate([keys[::3], misses[:10]])
  vals = rng.standard_normal((ins.size, D)).astype(F)
  ops.kv_variable_insert_v2(h, ins, vals)
  o.insert(ins, vals)
  _same_table(ops, h, o, probe)
  ops.kv_reserve(h, 1 << 16)                           # a second slab chunk and a rehash
  _same_table(ops, h, o, probe)
  if np.dtype(kd) == np.int64:                         # (the library imports int64 keys only)
    ex = _sorted_export(ops, h)
    _same_export(ex, o)
    # ... into a fresh table and out again: keys, rows, blacklist as exported; the frequency list as the reference's own
    # round trip leaves it (a key below the enter threshold is exported with its frequency word but without its row, so the
    # import does not bring it back)
    h2, o2 = _import_pair(ops, D, ex, G.ENTER, 3)
    ex2 = _sorted_export(ops, h2)
    for got, want in zip(ex2[:3], ex[:3]):
      np.testing.assert_array_equal(got, want)
    _same_export(ex2, o2)
    _same_table(ops, h2, o2, probe)
  lookups()


TRIPLES = [G.DIMS[i:i + 3] for i in range(0, len(G.DIMS), 3)]


@pytest.mark.parametrize("dims", TRIPLES, ids=["-".join(map(str, t)) for t in TRIPLES])
def test_batched_gather_over_three_dims(ops, dims):
  b = G.draw_batch(np.random.default_rng(G.SEEDS[1]))
  pairs = [_pair(ops, D, seed=5 + i) for i, D in enumerate(dims)]
  idl = []
  for i, (h, o) in enumerate(pairs):
    mine = b["keys"][i::2]                               # every table holds another part of the keys
    np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_v2(h, mine)), o.gather_or_insert(mine))
    idl.append(np.roll(b["ids"], 17 * i)[: b["ids"].size - 100 * i])
  outs = ops.batch_kv_variable_gather_or_zeros_v2([h for h, _ in pairs], idl)
  for (h, o), i, got in zip(pairs, idl, outs):
    np.testing.assert_array_equal(_np(got), o.gather_or_zeros(i))


@pytest.mark.parametrize("D", G.DIMS)
def test_scatter_update_every_operation(ops, D):
  """On the batch with its repeats.  ADD, SUB: rows and updates on one binary grid, so every order of a repeated id's
  updates gives the same bits; MUL: factors of +-1 for repeated ids; MIN, MAX: order-free; ASSIGN: a repeated id's updates
  are equal rows.  DIV on unique ids."""
  rng = np.random.default_rng([D, 2])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[2]))
  ids, keys = b["ids"], b["keys"]
  h, o = _pair(ops, D, seed=9)
  grid = (rng.integers(-64, 65, (keys.size, D)) * G.GQ).astype(F)
  ops.kv_variable_insert_v2(h, keys[::2], grid[::2])      # half of the keys exist (on the grid); the others are created
  o.insert(keys[::2], grid[::2])
  pos = {int(k): i for i, k in enumerate(keys.tolist())}
  row_of = np.array([pos[int(k)] for k in ids.tolist()])
  repeated = (b["counts"] > 1)[row_of]
  fns = [ops.kv_variable_scatter_update_v2, ops.kv_variable_scatter_add_v2, ops.kv_variable_scatter_sub_v2,
         ops.kv_variable_scatter_mul_v2, ops.kv_variable_scatter_div_v2, ops.kv_variable_scatter_min_v2,
         ops.kv_variable_scatter_max_v2]
  for op in (5, 6, 1, 2, 3, 0, 4):
    if op in (1, 2):
      # new keys start from the init rule's full-mantissa row: put every row on the grid first
      ops.kv_variable_scatter_update_v2(h, keys, grid)
      o.scatter_update(keys, grid, 0)
      upd = (rng.integers(-8, 9, (ids.size, D)) * G.GQ).astype(F)
    elif op == 3:
      upd = rng.uniform(0.5, 2.0, (ids.size, D)).astype(F)
      upd[repeated] = rng.choice([-1.0, 1.0], (int(repeated.sum()), D)).astype(F)
    elif op == 0:
      upd = rng.standard_normal((keys.size, D)).astype(F)[row_of]
    else:
      upd = rng.uniform(0.5, 2.0, (ids.size, D)).astype(F)
    if op == 4:
      u_ids, u_upd = keys, upd[: keys.size]
      fns[op](h, u_ids, u_upd)
      o.scatter_update(u_ids, u_upd, op)
      np.testing.assert_allclose(_np(ops.kv_variable_gather_or_zeros_v2(h, keys)), o.gather_or_zeros(keys), rtol=1e-6)
      continue
    fns[op](h, ids, upd)
    o.scatter_update(ids, upd, op)
    _same_table(ops, h, o, keys)


# ---- b. sparse lookups ------------------------------------------------------------------------------------------------------
def _segments(rng, cand):
  """About 200 segments: empty ones in front, in the middle and behind, one longer than a wave, one of misses only."""
  lens = rng.integers(0, 8, 200)
  lens[:3] = 0
  lens[100] = 0
  lens[7] = 70
  lens[9] = 5
  seg = np.repeat(np.arange(lens.size), lens)
  ids = rng.choice(cand, seg.size)
  ids[seg == 9] = cand[-5:]                                # the misses
  w = rng.uniform(0.1, 2.0, seg.size).astype(F)
  return ids, seg, w, int(lens.size + 4)


@pytest.mark.parametrize("D", G.DIMS)
def test_sparse_lookups(ops, D):
  rng = np.random.default_rng([D, 3])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[0]))
  h, o = _pair(ops, D, seed=11)
  known = b["keys"][:100]
  np.testing.assert_array_equal(_np(ops.kv_variable_gather_or_insert_v2(h, known)), o.gather_or_insert(known))
  absent = (b["keys"][:5].astype(np.int64) + 3)
  ids, seg, w, nseg = _segments(rng, np.concatenate([known, absent]))
  empty = np.setdiff1d(np.arange(nseg), seg)
  seg_grad = rng.standard_normal((nseg, D)).astype(F)
  for combiner in GR.COMBINERS:
    for weights in (None, w):
      what = "D %d %s %s" % (D, combiner, "weighted" if weights is not None else "plain")
      # the read-only lookup first: the misses read zeros
      got = ops.kv_variable_lookup_sparse_zeros(h, ids, seg, weights, nseg, combiner)
      want, tol = ZR.combine(o.gather_or_zeros(ids), seg, weights, nseg, combiner)
      ZR.check(_np(got), want, tol, what + " zeros")
      if weights is not None and combiner != "sum":
        assert bool(torch.isnan(got[empty]).all())
      else:
        assert float(got[empty].abs().sum()) == 0.0
      # the backward: defined bit for bit
      gg = ops.kv_variable_lookup_sparse_grad(h, seg_grad, seg, weights, nseg, combiner)
      assert GR.same_bits(_np(gg), GR.lookup_sparse_grad(seg_grad, seg, weights, nseg, combiner), nan_ok=True), what + " grad"
  # the training lookup inserts the misses (one hit per distinct key and call)
  for combiner in GR.COMBINERS:
    for weights in (None, w):
      got = ops.kv_variable_lookup_sparse(h, ids, seg, weights, nseg, combiner, count_occurrences=False)
      uniq, inv = np.unique(ids, return_inverse=True)
      rows = o.gather_or_insert(uniq)[inv]
      want, tol = ZR.combine(rows, seg, weights, nseg, combiner)
      ZR.check(_np(got), want, tol, "D %d %s training" % (D, combiner))
      assert (ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)) == (o.size(), o.sum_freq())
  _same_table(ops, h, o, np.concatenate([known, absent]))


# ---- c. optimizers ----------------------------------------------------------------------------------------------------------
def _single(ops, family):
  return {"group_adam_v4": ops.kv_variable_group_sparse_apply_adam_v4, "group_adam_v3": ops.kv_variable_group_sparse_apply_adam_v3,
          "sparse_group_ftrl": ops.kv_variable_sparse_group_sparse_apply_ftrl_v2, "ftrl_v2": ops.kv_variable_sparse_apply_ftrl_v2,
          "group_ftrl_v2": ops.kv_variable_group_sparse_apply_ftrl_v2,
          "group_radam": ops.kv_variable_group_sparse_apply_rectified_adam, "adam": ops.kv_variable_sparse_apply_adam}[family]


def _apply(ops, family, hs, grad, ids, hp, **kw):
  """One step of `family` on the tables hs = (var, slots...) through its single-table op."""
  if family == "adagrad":
    return ops.kv_variable_sparse_apply_adagrad(hs[0], hs[1], hp[0], grad, ids, update_slots=hp[1], **kw)
  if family.startswith("group_adam"):
    hp = hp[:9]
  return _single(ops, family)(*hs, grad, ids, *hp, **kw)


def _apply_multi(ops, family, sets, grads, idl, hp):
  roles = [[hs[j] for hs in sets] for j in range(len(sets[0]))]
  if family == "adagrad":
    return ops.kv_multi_sparse_apply_adagrad(roles[0], roles[1], hp[0], grads, idl, update_slots=hp[1])
  if family.startswith("group_adam"):
    return ops.kv_multi_group_sparse_apply_adam(*roles, grads, idl, *hp[:9], version=hp[9])
  fn = {"sparse_group_ftrl": ops.kv_multi_sparse_group_sparse_apply_ftrl, "ftrl_v2": ops.kv_multi_sparse_apply_ftrl_v2,
        "group_ftrl_v2": ops.kv_multi_group_sparse_apply_ftrl_v2, "group_radam": ops.kv_multi_group_sparse_apply_rectified_adam,
        "adam": ops.kv_multi_sparse_apply_adam}[family]
  return fn(*roles, grads, idl, *hp)


def _forms(D):
  f = ["plain", "tok", "unique"]
  if D % 4 == 0 and D <= 256:
    f.append("counted")
  if D % 4 == 0:
    f.append("multi")
  return f


def _check_step(ops, hs, tr, t, tag):
  st, keys = tr["steps"][t], tr["batch"]["keys"]
  clear = st["clear"]
  assert clear.mean() >= 0.99, tag                          # the cap of the skip
  for j, (h, tb) in enumerate(zip(hs, st["tables"])):
    got = _np(ops.kv_variable_gather_or_zeros_v2(h, keys)).astype(np.float64)
    tol = tb["tol"]
    if j == 0:
      ok = np.abs(got - tb["rows32"]) <= tol                # the project's bar against the float32 reference, or
      ok |= np.abs(got - tb["rows"]) <= st["widen"] * tol   # max(bar, 4 x the reference's own error) against float64, per row
    else:
      ok = np.abs(got - tb["rows"]) <= tol
    bad = ~ok & clear[:, None]
    assert not bad.any(), (tag, "table %d" % j, np.argwhere(bad)[:5], got[bad][:5], tb["rows"][bad][:5], tol[bad][:5])
    gm = ops.kv_get_meta(h, keys)
    diff = [(int(k), a, e) for k, a, e, c in zip(keys, gm, tb["metas"], clear) if c and a != e]
    assert not diff, (tag, "table %d" % j, diff[:5])
    assert ops.kv_variable_shape_v2(h)[0] == tb["counters"][0], (tag, j)      # the keys of the map: whatever a skipped row did
    if clear.all():                                         # (size and frequency sum leave blacklisted keys out)
      assert (ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)) == tb["counters"][1:], (tag, j)


def _align(ops, hs, tr, t):
  """GroupAdam between two steps: the rows just found within their bars of the reference's are set to the reference's own
  bits (scatter_update ASSIGN: no frequency word moves, a blacklisted row is left alone, the flags come from the same rows
  as the reference's).  The next step then starts from the reference's state, as the bars assume."""
  st, keys = tr["steps"][t], tr["batch"]["keys"]
  for h, tb in zip(hs, st["tables"]):
    there = st["clear"] & np.array([m is not None for m in tb["metas"]])
    ops.kv_variable_scatter_update_v2(h, keys[there], tb["rows32"][there].astype(F))


OPT_CASES = [(f, D, form) for f in G.FAMILIES for D in G.DIMS for form in _forms(D)]


@pytest.mark.parametrize("family,D,form", OPT_CASES, ids=["%s-%d-%s" % c for c in OPT_CASES])
def test_optimizer_step(ops, family, D, form):
  tr = G.trajectory(family, D)
  b = tr["batch"]
  sdims = G.slot_dims(family, D)
  sets = []
  for _ in range(2 if form == "multi" else 1):             # the batched form: two tables with the same history
    hs = [_table(ops, D, tr["vinit"], thr=G.ENTER, seed=G.OPT_SEED)] + \
         [_table(ops, d, init, seed=G.OPT_SEED) for d, init in zip(sdims, tr["sinits"])]
    ops.kv_variable_gather_or_insert_v2(hs[0], b["pre"])
    sets.append(hs)
  for t, st in enumerate(tr["steps"]):
    ids, grad, hp = st["ids"], st["grad"], st["hp"]
    tag = "%s D=%d %s step %d" % (family, D, form, t)
    if form == "multi":
      for hs in sets:
        ops.kv_variable_gather_or_insert_v2(hs[0], ids)
      _apply_multi(ops, family, sets, [grad] * 2, [ids] * 2, hp)
    else:
      hs = sets[0]
      if form == "tok":                                    # the training lookup of a device tensor, then the very same object
        dev_ids = torch.from_numpy(ids).cuda()
        ops.kv_variable_gather_or_insert_v2(hs[0], dev_ids)
        _apply(ops, family, hs, torch.from_numpy(grad).cuda(), dev_ids, hp)
      else:
        ops.kv_variable_gather_or_insert_v2(hs[0], ids)
        if form == "plain":
          _apply(ops, family, hs, grad, ids, hp)
        elif form == "unique":
          _apply(ops, family, hs, st["s"], st["u"], hp, unique_indices=True)
        else:                                              # counted: the unique count stays on the device
          uu, ss, _, nu = ops.kv_dedup_segment_sum(hs[0], ids, grad, sync=False)
          _apply(ops, family, hs, ss, uu, hp, unique_count=nu)
    if family in G.GROUP_FAMILIES:
      nb = int(st["black"].sum())
      assert 0 < nb < int(st["live"].sum()), tag            # both branches, by the reference alone
    if st["zeros"] is not None:
      assert 0 < st["zeros"][0] < st["zeros"][1], tag
    for hs in sets:
      _check_step(ops, hs, tr, t, tag)
      if family.startswith("group_adam") and t + 1 < G.STEPS:
        _align(ops, hs, tr, t)


# ---- d. occurrence order ----------------------------------------------------------------------------------------------------
OCC_DIMS = [64, 68, 128, 256, 260, 512, 516, 1024, 7, 63, 255]


@pytest.mark.parametrize("family", ["adam", "group_ftrl_v2"])
@pytest.mark.parametrize("D", OCC_DIMS)
def test_occurrence_order(ops, D, family):
  """kv_set_deterministic(h, 2): every dim takes the sorted pipeline, a hot key's chain is k_occ_sum's.  Gradients with full
  mantissas: the sums must be TF-core's occurrence-order sums bit for bit, and with them the step the model's."""
  import _kv_model as M
  assert D in G.DIMS
  rng = np.random.default_rng([D, 4])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[1]))
  ids, keys = b["ids"], b["keys"]
  vinit, sinits = G.inits(family, D, rng)
  sdims = G.slot_dims(family, D)
  hs = [_table(ops, D, vinit, thr=G.ENTER, seed=4)] + [_table(ops, d, i, seed=4) for d, i in zip(sdims, sinits)]
  var = M.Table(D, vinit, 4, DAY, G.ENTER)
  slots = [M.Table(d, i, 4, DAY, 0) for d, i in zip(sdims, sinits)]
  ops.kv_set_deterministic(hs[0], ops.KV_ORDER_OCCURRENCE)
  for t in range(2):
    grad = (rng.standard_normal((ids.size, D)) * 3e-2).astype(F)
    got = _np(ops.kv_variable_gather_or_insert_v2(hs[0], ids))
    want = var.gather_or_insert(ids)
    tol0 = var.tols(ids)
    assert (np.abs(got.astype(np.float64) - want) <= tol0).all()
    u, s, _ = ko.dedup_segment_sum(ids, grad)
    gu, gs, _ = ops.kv_dedup_segment_sum(hs[0], ids, grad)
    o1, o2 = np.argsort(_np(gu)), np.argsort(u)
    assert np.array_equal(_np(gu)[o1], u[o2])
    assert np.array_equal(_np(gs)[o1].view(np.uint32), s[o2].view(np.uint32)), "D %d: the sums differ from the occurrence-order sums" % D
    b1p, b2p = G.beta_pows(t)
    if family == "adam":
      hp = (0.05, b1p, b2p, 0.9, 0.999, 1e-8)
    else:
      hp = lambda x, srows, g: (0.1, M.lasso_threshold(M.linear_norms(family, x, srows, g, (0.1, 0.0, 1e-2, 1e-2, -0.5))[0], rng),
                                1e-2, 1e-2, -0.5)
    res = M.apply_step(family, var, slots, u, s, hp, bar=family != "adam")
    _apply(ops, family, hs, grad, ids, res["hp"])
    for j, (h, m) in enumerate(zip(hs, [var] + slots)):
      got = _np(ops.kv_variable_gather_or_zeros_v2(h, keys))
      want = m.gather_or_zeros(keys)
      if family == "adam":                                  # the same sums, the same operations: the same bits
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, t, j)
      else:
        assert (np.abs(got.astype(np.float64) - want) <= m.tols(keys)).all(), (D, t, j)
      assert ops.kv_get_meta(h, keys) == m.metas(keys), (D, t, j)
      assert (ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)) == \
          (m.map_size(), m.size(), m.sum_freq())
    if family != "adam":
      assert 0 < int((~res["updated"]).sum()) < len(res["keys"])


# ---- e. the dims outside the fused kernels' range ---------------------------------------------------------------------------
# What each op does on a table of a dim that dim_supported (kvhip.hip) does not admit — 257, 258, 1028, 2048 — as
# include/kvhip.h kv_create states it: ONE table, and test_refused_dims runs every entry of it, in this order.
#   SERVED    the op runs and must match the oracle (rows, records and counters of the table compared after each);
#   REFUSING  KV_UNIMPLEMENTED from the host-side checks, before anything is queued: map size, size, frequency sum, the rows
#             and the records of the probe keys are what they were.
# Every entry is a function of the case's context c (tables h, h2, h4 with their oracle twins o, o2, o4; ids with a few
# repeats, the distinct keys, probe = keys and misses, segment ids, weights, gradient rows, the rng).
def _neutral_hps():
  """Per family, scalars that pass every hyperparameter check: a refusal is about the dim alone."""
  b1p, b2p = G.beta_pows(0)
  return {"group_adam_v4": (0.05, b1p, b2p, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 4), "group_adam_v3": (0.05, b1p, b2p, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 3),
          "adagrad": (0.05, True), "sparse_group_ftrl": (0.1, 0.0, 0.0, 0.0, 0.0, -0.5), "ftrl_v2": (0.1, 0.0, 0.0, 0.0, -0.5),
          "group_ftrl_v2": (0.1, 0.0, 0.0, 0.0, -0.5),
          "group_radam": (0.1, b1p, b2p, 0.9, 0.999, 1e-7, 0.0, 0.0, 0.0, 0.4, False, False, False),
          "adam": (0.05, b1p, b2p, 0.9, 0.999, 1e-8)}


def _eq(got, want):
  np.testing.assert_array_equal(_np(got), want)


def _srv_lookup(c):
  _eq(c.ops.kv_variable_gather_or_insert_v2(c.h, c.ids), c.o.gather_or_insert(c.ids))


def _srv_lookup_counts(c):
  counts = c.rng.integers(1, 9, c.ids.size).astype(np.int32)
  _eq(c.ops.kv_variable_gather_or_insert_with_counts(c.h, c.ids, counts), c.o.gather_or_insert(c.ids, counts))


def _srv_zeros(c):
  _eq(c.ops.kv_variable_gather_or_zeros_v2(c.h, c.probe), c.o.gather_or_zeros(c.probe))


def _srv_batch_zeros(c):
  outs = c.ops.batch_kv_variable_gather_or_zeros_v2([c.h, c.h4], [c.probe, c.keys[:40]])
  _eq(outs[0], c.o.gather_or_zeros(c.probe))
  _eq(outs[1], c.o4.gather_or_zeros(c.keys[:40]))


def _srv_insert(c):
  ins = np.concatenate([c.keys[:10], c.probe[-10:]])
  vals = c.rng.standard_normal((ins.size, c.D)).astype(F)
  c.ops.kv_variable_insert_v2(c.h, ins, vals)
  c.o.insert(ins, vals)


def _srv_assign(c):
  upd = c.rng.standard_normal((c.keys.size, c.D)).astype(F)
  c.ops.kv_variable_scatter_update_v2(c.h, c.keys, upd)
  c.o.scatter_update(c.keys, upd, 0)


def _srv_fold_one_id(c):
  """The folding operations on ONE id: nothing to fold."""
  fns = [c.ops.kv_variable_scatter_add_v2, c.ops.kv_variable_scatter_sub_v2, c.ops.kv_variable_scatter_mul_v2,
         c.ops.kv_variable_scatter_min_v2, c.ops.kv_variable_scatter_max_v2]
  for op, fn in zip((1, 2, 3, 5, 6), fns):
    upd = c.rng.uniform(0.5, 2.0, (1, c.D)).astype(F)
    fn(c.h, c.keys[op:op + 1], upd)
    c.o.scatter_update(c.keys[op:op + 1], upd, op)


def _srv_export_import(c):
  ex = _sorted_export(c.ops, c.h)
  _same_export(ex, c.o)
  c.h2, c.o2 = _import_pair(c.ops, c.D, ex, G.ENTER, 6)
  _same_export(_sorted_export(c.ops, c.h2), c.o2)
  _same_table(c.ops, c.h2, c.o2, c.probe)


def _srv_lookup_sparse(c):
  got = c.ops.kv_variable_lookup_sparse(c.h, c.ids, c.seg, c.w, 50, "mean", count_occurrences=False)
  uniq, inv = np.unique(c.ids, return_inverse=True)
  want, tol = ZR.combine(c.o.gather_or_insert(uniq)[inv], c.seg, c.w, 50, "mean")
  ZR.check(_np(got), want, tol, "D %d lookup_sparse" % c.D)


def _srv_lookup_sparse_grad(c):
  sg = c.rng.standard_normal((50, c.D)).astype(F)
  assert GR.same_bits(_np(c.ops.kv_variable_lookup_sparse_grad(c.h, sg, c.seg, c.w, 50, "sqrtn")),
                      GR.lookup_sparse_grad(sg, c.seg, c.w, 50, "sqrtn"), nan_ok=True)


def _ref_optimizers(c):
  """every family: the op with the duplicate sum inside (_tok), the _unique op, the batched op over two tables"""
  hps = _neutral_hps()
  for family in G.FAMILIES:
    slots = [_table(c.ops, d, np.zeros((1, d), F), seed=6) for d in G.slot_dims(family, c.D)]
    slots2 = [_table(c.ops, d, np.zeros((1, d), F), seed=6) for d in G.slot_dims(family, c.D)]
    _refused(_apply, c.ops, family, [c.h] + slots, c.grad, c.ids, hps[family])
    _refused(_apply, c.ops, family, [c.h] + slots, c.grad[: c.keys.size], c.keys, hps[family], unique_indices=True)
    _refused(_apply_multi, c.ops, family, [[c.h] + slots, [c.h2] + slots2], [c.grad] * 2, [c.ids] * 2, hps[family])
    for s in slots + slots2:
      assert c.ops.kv_variable_shape_v2(s)[0] == 0


def _ref_scatter_folds(c):
  """ADD, SUB, MUL, DIV, MIN, MAX on more than one id: every occurrence of a repeated id counts, which takes the
  de-duplication of the fused kernels' dims"""
  upd = c.rng.uniform(0.5, 2.0, (c.ids.size, c.D)).astype(F)
  for fn in (c.ops.kv_variable_scatter_add_v2, c.ops.kv_variable_scatter_sub_v2, c.ops.kv_variable_scatter_mul_v2,
             c.ops.kv_variable_scatter_div_v2, c.ops.kv_variable_scatter_min_v2, c.ops.kv_variable_scatter_max_v2):
    _refused(fn, c.h, c.ids, upd)
    _refused(fn, c.h, c.keys[:2], upd[:2])


SERVED = [("gather_or_insert", _srv_lookup), ("gather_or_insert_with_counts", _srv_lookup_counts), ("gather_or_zeros", _srv_zeros),
          ("batch_gather_or_zeros", _srv_batch_zeros), ("insert", _srv_insert), ("scatter_update ASSIGN", _srv_assign),
          ("scatter_update, any operation, one id", _srv_fold_one_id), ("export / import / export", _srv_export_import),
          ("lookup_sparse", _srv_lookup_sparse), ("lookup_sparse_grad", _srv_lookup_sparse_grad)]
REFUSING = [("every optimizer apply (tok, unique, batched)", _ref_optimizers),
            ("scatter_update ADD .. MAX on more than one id", _ref_scatter_folds),
            ("dedup_segment_sum", lambda c: _refused(c.ops.kv_dedup_segment_sum, c.h, c.ids, c.grad)),
            ("dedup_segment_sum_dev", lambda c: _refused(c.ops.kv_dedup_segment_sum, c.h, c.ids, c.grad, sync=False)),
            ("unsorted_segment_sum", lambda c: _refused(c.ops.kv_unsorted_segment_sum, c.h, c.grad, np.zeros(c.ids.size, np.int32), 4)),
            ("lookup_sparse_zeros", lambda c: _refused(c.ops.kv_variable_lookup_sparse_zeros, c.h, c.ids, c.seg, None, 50, "sum")),
            ("batch_lookup_sparse_zeros", lambda c: _refused(c.ops.batch_kv_variable_lookup_sparse_zeros, [c.h, c.h4], [c.ids, c.keys[:40]],
                                                             [c.seg, np.arange(40)], None, [50, 40], "sum"))]


def _refused(fn, *a, **kw):
  from tfplus_amd import _lib
  with pytest.raises(_lib.UnimplementedError):
    fn(*a, **kw)


class _Ctx(object):
  pass


@pytest.mark.parametrize("D", G.REFUSED)
def test_refused_dims(ops, D):
  assert not G.dim_supported(D)
  c = _Ctx()
  c.ops, c.D, c.rng = ops, D, np.random.default_rng([D, 5])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[0]))
  c.keys = b["keys"]
  c.ids = np.concatenate([c.keys, c.keys[:40]])             # a few repeats
  c.probe = np.concatenate([c.keys, c.keys[:10].astype(np.int64) + 5])
  c.seg = np.sort(c.rng.integers(0, 50, c.ids.size))
  c.w = c.rng.uniform(0.1, 2.0, c.ids.size).astype(F)
  c.grad = c.rng.standard_normal((c.ids.size, D)).astype(F)
  c.h, c.o = _pair(ops, D, thr=G.ENTER, seed=6)
  c.h4, c.o4 = _pair(ops, 4, seed=7)
  ops.kv_variable_gather_or_insert_v2(c.h4, c.keys[:30])
  c.o4.gather_or_insert(c.keys[:30])
  for name, fn in SERVED:
    fn(c)
    _same_table(ops, c.h, c.o, c.probe)

  def state():
    return (ops.kv_variable_shape_v2(c.h)[0], ops.kv_variable_size_v2(c.h), ops.kv_variable_frequency(c.h),
            _np(ops.kv_variable_gather_or_zeros_v2(c.h, c.probe)).tobytes(), ops.kv_get_meta(c.h, c.probe))

  before = state()
  for name, fn in REFUSING:
    fn(c)
    assert state() == before, name
  _same_table(ops, c.h, c.o, c.probe)


@pytest.mark.parametrize("D", [6, 255])
def test_batched_and_counted_forms_refuse_dims_that_are_no_multiple_of_4(ops, D):
  rng = np.random.default_rng([D, 6])
  b = G.draw_batch(np.random.default_rng(G.SEEDS[0]))
  ids = b["ids"]
  grad = rng.standard_normal((ids.size, D)).astype(F)
  hps = _neutral_hps()
  for family in G.FAMILIES:
    sets = []
    for _ in range(2):
      h, _o = _pair(ops, D, seed=8)
      ops.kv_variable_gather_or_insert_v2(h, b["keys"])
      sets.append([h] + [_table(ops, d, np.zeros((1, d), F), seed=8) for d in G.slot_dims(family, D)])
    before = [_np(ops.kv_variable_gather_or_zeros_v2(hs[0], b["keys"])) for hs in sets]
    _refused(_apply_multi, ops, family, sets, [grad] * 2, [ids] * 2, hps[family])
    uu, ss, _, nu = ops.kv_dedup_segment_sum(sets[0][0], ids, grad, sync=False)
    _refused(_apply, ops, family, sets[0], ss, uu, hps[family], unique_count=nu)
    for hs, was in zip(sets, before):
      assert np.array_equal(_np(ops.kv_variable_gather_or_zeros_v2(hs[0], b["keys"])), was)
      assert all(ops.kv_variable_shape_v2(s)[0] == 0 for s in hs[1:])
