"""Keys crafted against the hash (tests/_hash_keys.py) through the ops, against oracle.kv_oracle.OracleKv and
ko.dedup_segment_sum exactly as tests/test_gpu_fuzz.py uses them.  The oracle knows nothing of the hash, so the crafted
keys cost it nothing; the kernels meet what uniform ids never give them: one partition with thousands of distinct keys
(the sub-hash splits, a second and an eighth split level, empty sibling classes, the sentinel key INT64_MIN inside a class
that splits), every key in one LDS slot (probes that wrap), a partition's sources filed in global memory, hot keys inside
the crafted partition, probe chains of the table index that wrap from slot `mask` to slot 0 behind tombstones, and the
batch the partition pass REFUSES (device error 2).

Tolerances are the project's own: lookups, counts, time stamps, sizes, key sets, kv_unique's inverse and
kv_dedup_segment_sum's sums are exact; rows and slot rows after an apply RTOL, ATOL = 1e-6, 1e-7 (test_gpu_fuzz.py).
Where an op sums repeated ids itself the gradients are integers in [-8, 8] times 2^-10: any order of up to 4096 additions
is exact in fp32.  Every case runs at D = 8 (the entry-list kernels: k_ltile, k_part2 / k_papply) and at D = 6 (the
sorted-position pipeline, kv_kernels.h), which a var in occurrence-order mode takes at D = 8 too.  The library offers the
counted and the batched ops for dims that are multiples of 4 only, and the batched ops refuse a var in occurrence-order mode:
those two forms run where they exist.

Section B — what a refused batch leaves, read from the code before the cases were run
---------------------------------------------------------------------------------------
A partition block refuses (raise_error(.., 2)) in two places: more than 65535 entries (kv_fused.h part2_body,
kv_papply.h, kv_kernels.h part_keys_body: before it touches anything), or a class of more than UCAPK (768 / 1023) distinct
keys that is still together when the work list of classes is 24 deep.  The list grows only when the class that overflows
is the one on TOP of the list (hash bit 1 at that level: its empty sibling stays below it), so 24 equal hash bits are not
enough: bits 20 .. 43 all ONES are refused after 23 halvings; the sentinel key's own pattern (0x810af3, ten ones) is
halved 24 times without the list growing past 12 and then separates on bits 44 ..: handled (case A7).  Either way the
loop ends: every pass pops one class, and a split pushes two only while the list holds fewer than 23.
What is left behind:
  * sorted-position pipeline (D = 6, occurrence order, kv_unique): keys are inserted by the partition block itself
    (table_find_or_insert, one owner per key), a refused partition has inserted none; the kernels behind it see the flag
    and return.  Nothing is left.
  * entry-list pipeline (D = 8): the TILE pass (tile_insert) has already claimed an index entry {key, row, HINT_NEW} and
    a row for every new key; the row's record (key, frequency word, flags) and contents are written by the partition pass,
    which gave up.  Readers of that state: the fused lookup's `hint == HINT_NEW` branch and uniq_insert treat the key as
    new again (safe); table_find (gather_or_zeros, get_count, get_meta, delete) finds the row and reads a record that was
    never written; and everything that walks the ROWS — k_stats (size), k_export, k_delete_by_time, and k_rehash, which
    re-inserts "key 0" once per such row and can shadow the real key 0 — takes it for a live key.  Not safe.  Fixed
    before these cases ran: the report of code 2 (kvhip.hip flagged_error -> k_rollback_new) turns every HINT_NEW
    entry into a tombstone and returns its row to the free list, after letting a later lookup's still-pending partition
    pass run (its HINT_NEW entries are its own).  batch.drop() makes the refused batch's token stale.
The contract asserted here is include/kvhip.h "The refused batch": reported by the next call at the latest (a token
lookup defers its partition pass to the next op, so there the call behind THAT op may be the one), once, KV_INTERNAL,
both causes named; no key the table held changes; the keys the batch would have inserted are absent afterwards.
B's batches are one class each (the crafted family alone), so "nothing applied" is exact for them; the header says what
the code does otherwise: the block goes on with the classes still on its list after it has raised the error, and the ones
it finished before stay, so a partition that holds an inseparable set AND other keys is partly applied.

Measured on an MI355X in a run of the whole suite, against the budget of "a few seconds" per case:
  A5 one_partition(60000)   lookup + token apply on the device: D = 8 0.032 s (GroupAdam), 0.027 s (Adagrad); D = 6 0.070 s
                            both; the whole case with the oracle and the full checks 0.31 .. 0.38 s.  60000 stays.
  slowest other case        B1 at D = 8 as a lookup, 0.98 s (the six B1 cases 0.86 .. 0.98 s: all 66000 keys fed back in
                            132 slices of 500 with an oracle call each); every case outside A5 and B1 is below 0.25 s
"""
import time

import numpy as np
import pytest

from oracle import kv_oracle as ko

import _hash_keys as hk

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-7      # tests/test_gpu_fuzz.py
DAY0 = 20000
F = np.float32
DIMS = [8, 6]


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


class Pair(object):
  """one GPU table and its oracle twin (as tests/test_gpu_fuzz.py Pair; the check takes the keys to look at)"""

  def __init__(self, ops, D, table, seed, key_dtype=None, capacity_hint=64):
    self.ops, self.D = ops, D
    self.h = ops.kv_variable([D], capacity_hint=capacity_hint, key_dtype=key_dtype or torch.int64)
    ops.kv_set_seed(self.h, seed); ops.init_kv_variable_v2(self.h, table)
    self.o = ko.OracleKv(D, 0, table, day=DAY0, picker=1, seed=seed)
    self.set_day(DAY0)

  def set_day(self, day):
    self.ops.kv_set_clock_days(self.h, day); self.o.set_day(day)

  def check(self, keys, tag, exact=False, meta=True):
    """the whole observable state on `keys` (present or not): figures, rows, counts, stamps, kv_get_meta records"""
    ops, h, o = self.ops, self.h, self.o
    q = np.asarray(keys).astype(np.int64)
    assert ops.kv_variable_shape_v2(h)[0] == o.map_size(), tag
    assert ops.kv_variable_size_v2(h) == o.size() and ops.kv_variable_frequency(h) == o.sum_freq(), tag
    got = ops.kv_variable_gather_or_zeros_v2(h, q).cpu().numpy()
    if exact:
      np.testing.assert_array_equal(got, o.gather_or_zeros(q), err_msg=tag)
    else:
      np.testing.assert_allclose(got, o.gather_or_zeros(q), rtol=RTOL, atol=ATOL, err_msg=tag)
    np.testing.assert_array_equal(ops.kv_variable_get_count_v2(h, q).cpu().numpy(), o.get_count(q), err_msg=tag)
    np.testing.assert_array_equal(ops.kv_variable_get_time_stamp(h, q).cpu().numpy(), o.get_timestamp(q), err_msg=tag)
    if meta:
      assert ops.kv_get_meta(h, q) == [o.meta(int(k)) for k in q], tag


class Rig(object):
  """a var and its optimizer's slot table, pre-filled with 500 random keys; every op runs on both sides"""

  def __init__(self, ops, D, opt="adam", occ=False, key_dtype=None, seed=7, prefill=500):
    self.ops, self.D, self.opt = ops, D, opt
    rng = np.random.default_rng(900 + seed)
    table = rng.standard_normal((32, D)).astype(F)
    self.var = Pair(ops, D, table, seed, key_dtype)
    sd, sv = {"adam": (3 * D, 0.0), "adagrad": (D, 0.1)}[opt]
    self.slot = Pair(ops, sd, np.full((4, sd), sv, F), seed, key_dtype)
    if occ:
      ops.kv_set_deterministic(self.var.h, ops.KV_ORDER_OCCURRENCE)
    self.b1p, self.b2p = F(0.9), F(0.999)
    lo, hi = (-(1 << 31), (1 << 31) - 1) if key_dtype == torch.int32 else (-(1 << 62), 1 << 62)
    self.pre = np.unique(rng.integers(lo, hi, prefill)) if prefill else np.empty(0, np.int64)
    self.absent = rng.integers(lo, hi, 64)
    if prefill:
      self.lookup(self.pre)
    self.seen = [self.pre, self.absent]

  def dev(self, ids):
    return torch.from_numpy(np.ascontiguousarray(ids)).cuda()

  def lookup(self, ids, t=None):
    t = self.dev(ids) if t is None else t
    got = self.ops.kv_variable_gather_or_insert_v2(self.var.h, t).cpu().numpy()
    np.testing.assert_array_equal(got, self.var.o.gather_or_insert(ids))
    return t

  def oracle_apply(self, u, s):
    if self.opt == "adam":
      ko.apply_group_adam(self.var.o, self.slot.o, s, u, 1e-2, self.b1p, self.b2p, 0.9, 0.999, 1e-8)
    else:
      ko.apply_adagrad(self.var.o, self.slot.o, 0.05, s, u)

  def apply(self, ids, g, **kw):
    """the op on (ids, g) as given — it sums repeats itself —, the oracle on TF-core's unique ids and sums"""
    if self.opt == "adam":
      self.ops.kv_variable_group_sparse_apply_adam_v4(self.var.h, self.slot.h, g, ids, 1e-2, self.b1p, self.b2p, 0.9, 0.999,
                                                      1e-8, 0, 0, 0, **kw)
    else:
      self.ops.kv_variable_sparse_apply_adagrad(self.var.h, self.slot.h, 0.05, g, ids, **kw)

  def step(self, ids_np, g_np):
    u, s, _ = ko.dedup_segment_sum(ids_np, g_np)
    self.oracle_apply(u, s)
    self.b1p, self.b2p = F(self.b1p * F(0.9)), F(self.b2p * F(0.999))

  def check(self, keys, tag, **kw):
    q = np.concatenate([np.asarray(keys).astype(np.int64)] + [np.asarray(s).astype(np.int64) for s in self.seen])
    self.var.check(q, tag, **kw)
    self.slot.check(q, tag + " slot", **kw)


def grads(rng, n, D):
  return (rng.uniform(0.5, 1.5, (n, D)) * 1e-2 * rng.choice([-1.0, 1.0], (1, D))).astype(F)


def int_grads(rng, n, D):
  return (rng.integers(-8, 9, (n, D)) * 2.0 ** -10).astype(F)


def dedup_checks(ops, rig, ids, rng, tag):
  """kv_unique and kv_dedup_segment_sum on ids (repeats included), integer gradients: everything exact"""
  g = int_grads(rng, ids.size, rig.D)
  u, s, _ = ko.dedup_segment_sum(ids, g)
  gu, gs, ginv = [x.cpu().numpy() for x in ops.kv_dedup_segment_sum(rig.var.h, ids, g)]
  assert np.array_equal(gu[ginv], ids.astype(np.int64)), tag
  assert np.array_equal(np.sort(gu), np.sort(u)), tag
  assert np.array_equal(gs[np.argsort(gu)].view(np.uint32), s[np.argsort(u)].view(np.uint32)), tag
  qu, qc, qinv = [x.cpu().numpy() for x in ops.kv_unique(rig.var.h, ids)]
  assert np.array_equal(qu[qinv], ids.astype(np.int64)), tag
  wu, wc = np.unique(ids.astype(np.int64), return_counts=True)
  o = np.argsort(qu)
  assert np.array_equal(qu[o], wu) and np.array_equal(qc[o], wc), tag


def split_ops(ops, D, keys, occ, seed):
  """A1's ops: every id once — lookup, token apply, plain apply, unique apply, counted form, the batched op over two
  tables; then kv_unique / kv_dedup_segment_sum on the ids plus 3000 repeats.  The full check after each."""
  rng = np.random.default_rng(seed)
  rig = Rig(ops, D, "adam", occ)
  ids = rng.permutation(keys)
  t = rig.lookup(ids)
  rig.check(ids, "lookup", exact=True)
  g = grads(rng, ids.size, D)
  rig.apply(t, g); rig.step(ids, g)                              # the very tensor of the lookup: its token
  rig.check(ids, "token apply")
  g = grads(rng, ids.size, D)
  rig.apply(ids.copy(), g); rig.step(ids, g)
  rig.check(ids, "plain apply")
  g = grads(rng, ids.size, D)
  rig.apply(ids.copy(), g, unique_indices=True); rig.step(ids, g)
  rig.check(ids, "unique apply")
  if D % 4 == 0:
    g = int_grads(rng, ids.size, D)
    du, ds, _, nu = ops.kv_dedup_segment_sum(rig.var.h, ids, g, sync=False)
    rig.apply(du, ds, unique_count=nu); rig.step(ids, g)
    rig.check(ids, "counted apply")
  if D % 4 == 0 and not occ:
    r2 = Rig(ops, D, "adam", occ, seed=8)
    ids2 = rng.permutation(keys)
    t1, t2 = rig.dev(ids), r2.dev(ids2)
    o1, o2 = ops.kv_multi_gather_or_insert([rig.var.h, r2.var.h], [t1, t2])
    np.testing.assert_array_equal(o1.cpu().numpy(), rig.var.o.gather_or_insert(ids))
    np.testing.assert_array_equal(o2.cpu().numpy(), r2.var.o.gather_or_insert(ids2))
    g1, g2 = grads(rng, ids.size, D), grads(rng, ids.size, D)
    assert rig.b1p != r2.b1p                                      # (the batched op takes one set of scalars: rig's)
    r2.b1p, r2.b2p = rig.b1p, rig.b2p
    ops.kv_multi_group_sparse_apply_adam([rig.var.h, r2.var.h], [rig.slot.h, r2.slot.h], [g1, g2], [t1, t2], 1e-2,
                                         rig.b1p, rig.b2p, 0.9, 0.999, 1e-8, 0, 0, 0)
    rig.step(ids, g1); r2.step(ids2, g2)
    rig.check(ids, "batched apply"); r2.check(ids2, "batched apply, table 2")
  rep = np.concatenate([ids, ids[rng.integers(0, ids.size, 3000)]])
  dedup_checks(ops, rig, rng.permutation(rep), rng, "dedup")
  rig.check(ids, "after dedup")                                   # (neither op touches the table)


# ---- A. one partition, many keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("occ", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_A1_one_partition_every_apply_form(ops, D, occ):
  split_ops(ops, D, hk.case("A1"), occ, 101)


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("D", DIMS)
def test_A2_deep_split_with_empty_siblings(ops, D, k):
  split_ops(ops, D, hk.case("A2_k%d" % k), False, 102 + k)


@pytest.mark.parametrize("name", ["A3_lds", "A3_tile"])
@pytest.mark.parametrize("D", DIMS)
def test_A3_every_key_in_one_lds_slot(ops, D, name):
  rng = np.random.default_rng(103)
  rig = Rig(ops, D)
  ids = rng.permutation(hk.case(name))
  t = rig.lookup(ids)
  rig.check(ids, "lookup", exact=True)
  g = grads(rng, ids.size, D)
  rig.apply(t, g); rig.step(ids, g)
  rig.check(ids, "token apply")
  dedup_checks(ops, rig, rng.permutation(np.concatenate([ids, ids[: ids.size // 2]])), rng, "dedup")


@pytest.mark.parametrize("D", DIMS)
def test_A4_hot_keys_inside_the_crafted_partition(ops, D):
  """2000 keys once and 20 of them 2100 times more (2101 occurrences: 17 chunks of 128 rows).  The partition splits, and
  the overflow branch counts its keys per CLASS, so the 20 hot keys agree in hash bits 20 .. 22 and stay in one class
  (tests/test_hash_keys.py restates the split): D = 6 gets more than 16 keys of more than 16 chunks in it (the lbig
  overflow branch of kv_kernels.h), D = 8 the hot-chunk items of k_papply.  The op sums the repeats: integer gradients."""
  rng = np.random.default_rng(104)
  rig = Rig(ops, D)
  hot = hk.case("A4_hot")
  keys = np.concatenate([hk.case("A4"), hot])
  ids = rng.permutation(np.concatenate([keys, np.repeat(hot, 2100)]))
  assert ids.size == 44000
  rig.lookup(ids)
  rig.check(keys, "lookup", exact=True)
  g = int_grads(rng, ids.size, D)
  rig.apply(ids.copy(), g); rig.step(ids, g)
  rig.check(keys, "plain apply")
  nseg = 64
  seg = np.sort(rng.integers(0, nseg, ids.size))
  got = ops.kv_variable_lookup_sparse(rig.var.h, ids, seg, None, nseg, "sum", count_occurrences=False).cpu().numpy()
  uniq, idx = np.unique(ids, return_inverse=True)
  emb = rig.var.o.gather_or_insert(uniq)[idx]
  want = np.zeros((nseg, D), F)
  for j in range(ids.size):                                       # position order, fp32 (as tests/test_gpu_fuzz.py)
    want[seg[j]] = want[seg[j]] + emb[j]
  np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
  rig.check(keys, "sparse lookup", meta=True)


@pytest.mark.parametrize("opt", ["adam", "adagrad"])
@pytest.mark.parametrize("D", DIMS)
def test_A5_sixty_thousand_keys_in_one_partition(ops, D, opt):
  """below the 65535-entry limit: one block walks the classes of 60000 entries, their sources filed in global memory
  (E > PA_LSRC).  Times in the module docstring."""
  rng = np.random.default_rng(105)
  rig = Rig(ops, D, opt)
  ids = rng.permutation(hk.case("A5"))
  g = grads(rng, ids.size, D)
  dt = rig.dev(ids)
  torch.cuda.synchronize(); t0 = time.perf_counter()
  got = ops.kv_variable_gather_or_insert_v2(rig.var.h, dt)
  rig.apply(dt, g)                                                # the lookup's token
  torch.cuda.synchronize(); t1 = time.perf_counter()
  print("A5 D=%d %s: lookup + token apply of 60000 one-partition keys, device time %.3f s" % (D, opt, t1 - t0))
  np.testing.assert_array_equal(got.cpu().numpy(), rig.var.o.gather_or_insert(ids))
  rig.step(ids, g)
  rig.check(ids, "token apply", meta=True)


@pytest.mark.parametrize("D", DIMS)
def test_A6_int32_keys_of_one_partition(ops, D):
  """int32 keys share the sentinel's top 6 hash bits: ONE partition whenever P <= 64, which the entry-list kernels
  (D = 8) pick for up to 24576 ids and the sorted-position pipeline (D = 6) for up to 2048 — so at D = 6 these 3000 ids
  fall into two partitions of P = 128, about 1500 keys each, which still split."""
  rng = np.random.default_rng(106)
  rig = Rig(ops, D, key_dtype=torch.int32)
  ids = rng.permutation(hk.case("A6"))
  assert ids.dtype == np.int32
  t = rig.lookup(ids)
  rig.check(ids, "lookup", exact=True)
  g = grads(rng, ids.size, D)
  rig.apply(t, g); rig.step(ids, g)
  rig.check(ids, "token apply")
  g = grads(rng, ids.size, D)
  rig.apply(ids.copy(), g, unique_indices=True); rig.step(ids, g)
  rig.check(ids, "unique apply")


@pytest.mark.parametrize("D", DIMS)
def test_A7_the_sentinels_own_sub_hash_is_split_24_times_and_handled(ops, D):
  """1100 keys and INT64_MIN agree in hash bits 20 .. 43 (0x810af3): 24 halvings leave them together, the work list never
  grows past 12 (module docstring), bits 44 .. then separate them: NOT refused"""
  rng = np.random.default_rng(107)
  rig = Rig(ops, D)
  ids = rng.permutation(hk.case("A7"))
  t = rig.lookup(ids)
  rig.check(ids, "lookup", exact=True)
  g = grads(rng, ids.size, D)
  rig.apply(t, g); rig.step(ids, g)
  rig.check(ids, "token apply")
  g = grads(rng, ids.size, D)
  rig.apply(ids.copy(), g); rig.step(ids, g)
  rig.check(ids, "plain apply")


# ---- B. the refusals -------------------------------------------------------------------------------------------------------
def snapshot(ops, pair, keys):
  h = pair.h
  return (ops.kv_variable_gather_or_zeros_v2(h, keys).cpu().numpy().view(np.uint32),
          ops.kv_variable_get_count_v2(h, keys).cpu().numpy(), ops.kv_variable_get_time_stamp(h, keys).cpu().numpy(),
          ops.kv_get_meta(h, keys))


def assert_same(a, b, tag):
  for x, y in zip(a[:3], b[:3]):
    np.testing.assert_array_equal(x, y, err_msg=tag)
  assert a[3] == b[3], tag


def assert_export_equal(ops, pair, tag):
  """the full export against the oracle's: keys and rows, blacklist, frequency keys and words (row order is unspecified)"""
  k, v, bl, fk, fv = [x.cpu().numpy() for x in ops.kv_variable_export(pair.h, first_n=6)]
  ok, ov, obl, ofk, ofv = pair.o.export(6)
  assert np.array_equal(np.sort(k), np.sort(ok)) and np.array_equal(np.sort(bl), np.sort(obl)), tag
  np.testing.assert_allclose(v[np.argsort(k)], ov[np.argsort(ok)], rtol=RTOL, atol=ATOL, err_msg=tag)   # rows behind an apply
  assert np.array_equal(np.sort(fk), np.sort(ofk)), tag
  np.testing.assert_array_equal(fv[np.argsort(fk)].view(np.uint32), ofv[np.argsort(ofk)], err_msg=tag)


B_CASES = [("B1", "lookup"), ("B1", "apply"), ("B1", "unique"), ("B2", "lookup"), ("B2", "apply")]


@pytest.mark.parametrize("name,op", B_CASES)
@pytest.mark.parametrize("D", DIMS)
def test_B_refused_batch(ops, D, name, op):
  """B1: 66000 one-partition keys, E > 65535.  B2: 1100 keys whose hash bits 20 .. 43 are all ones (the split list is
  24 deep and every split adds one: refused after 23 halvings, see the module docstring).  Run once each.  The call
  behind the refused one is kv_size, which waits for the device: the report is due there."""
  from tfplus_amd import _lib
  rng = np.random.default_rng(108)
  rig = Rig(ops, D)
  # a first, ordinary step: the keys the table held before have rows, slot rows, counts and stamps worth comparing
  g0 = grads(rng, rig.pre.size, D)
  rig.apply(rig.pre.copy(), g0); rig.step(rig.pre, g0)
  rig.var.set_day(DAY0 + 1); rig.slot.set_day(DAY0 + 1)
  ids = rng.permutation(hk.case(name))
  before_v, before_s = snapshot(ops, rig.var, rig.pre), snapshot(ops, rig.slot, rig.pre)

  def refused_call():
    if op == "lookup":
      ops.kv_variable_gather_or_insert_v2(rig.var.h, ids)
    elif op == "apply":
      rig.apply(ids.copy(), grads(rng, ids.size, D))
    else:
      ops.kv_unique(rig.var.h, ids)
  errors = []
  for call in (refused_call, lambda: ops.kv_variable_size_v2(rig.var.h)):   # the refused call and the NEXT call on the table
    try:
      call()
    except _lib.KvError as e:
      errors.append(e)
    if call is refused_call:   # (the single-table reads report no deferred error and are not that next call: the header)
      ops.kv_variable_gather_or_zeros_v2(rig.var.h, rig.pre[:4]); ops.kv_variable_get_count_v2(rig.var.h, rig.pre[:4])
  assert len(errors) == 1, errors                                  # reported, by the next call at the latest ...
  e = errors[0]
  assert isinstance(e, _lib.KvError) and e.code == _lib.KV_INTERNAL
  assert "65535 entries" in str(e) and "no sub-hash separates" in str(e) and "not applied" in str(e)
  assert ops.kv_variable_size_v2(rig.var.h) == rig.var.o.size()    # ... and once: kv_size again, a call that DOES report
  # nothing the table held has changed, bit for bit; the refused keys are absent; the figures are the oracle's, which
  # never saw the batch
  assert_same(snapshot(ops, rig.var, rig.pre), before_v, "var")
  assert_same(snapshot(ops, rig.slot, rig.pre), before_s, "slot")
  assert not ops.kv_variable_gather_or_zeros_v2(rig.var.h, ids).any()
  assert not ops.kv_variable_get_count_v2(rig.var.h, ids).any()
  assert ops.kv_get_meta(rig.var.h, ids[:1024]) == [None] * 1024
  rig.check(ids[:4096], "after the refusal")
  assert_export_equal(ops, rig.var, "after the refusal")
  assert sorted(ops.kv_variable_delete_with_timestamp(rig.var.h, 1).cpu().tolist()) == \
      sorted(rig.var.o.delete_with_timestamp(1).tolist()) == sorted(rig.pre.tolist())   # the walk over the rows meets no orphan
  rig.seen = [rig.absent, rig.pre]
  # the same keys in slices of 500 (these fit), deleted, looked up again; a rebuild of the index in between
  sub = ids
  for i in range(0, sub.size, 500):
    rig.lookup(sub[i:i + 500])
  rig.check(sub, "slices", exact=True)
  for p in (rig.var, rig.slot):
    assert ops.kv_variable_delete(p.h, sub[::2]) == p.o.delete(sub[::2])
  rig.check(sub, "deleted", exact=True)
  ops.kv_reserve(rig.var.h, 300000)
  rig.check(sub, "rebuilt", exact=True)
  sub = rng.permutation(sub)
  for i in range(0, sub.size, 500):                                # (slices again: B2's keys at once ARE the refused batch)
    part = sub[i:i + 500]
    rig.lookup(part)
    g = grads(rng, part.size, D)
    rig.apply(part.copy(), g); rig.step(part, g)
  rig.check(sub, "revived and applied")


def test_B_token_lookup_followed_by_calls_that_do_not_wait(ops):
  """The training lookup defers its partition pass to the table's next op (kv_gather_or_insert_tok): the refusal is raised
  INSIDE that op.  When that op does not wait for the device — here another training lookup, whose own partition pass is
  pending in its turn when the report comes — the call behind it reports: the header's "by the call behind that op".
  Once; the refused keys are gone, the second lookup's are not."""
  from tfplus_amd import _lib
  rng = np.random.default_rng(110)
  rig = Rig(ops, 8)
  ids = rng.permutation(hk.case("B2"))
  ops.kv_variable_gather_or_insert_v2(rig.var.h, ids)              # queued; its partition pass is pending
  fresh = hk.case("B3")                                            # new keys of the same partition, in the call behind it
  raised = []
  for n, q in enumerate((fresh, rig.pre[:8], rig.pre[8:16])):
    try:
      got = ops.kv_variable_gather_or_insert_v2(rig.var.h, q).cpu().numpy()
    except _lib.KvError as e:
      raised.append((n, e))
      continue
    np.testing.assert_array_equal(got, rig.var.o.gather_or_insert(q))
  assert len(raised) == 1 and raised[0][0] == 1 and raised[0][1].code == _lib.KV_INTERNAL, raised
  assert not ops.kv_variable_gather_or_zeros_v2(rig.var.h, ids).any()
  rig.check(np.concatenate([ids, fresh]), "after the late report", exact=True)


# ---- C. the table index -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,via", [(8, "lookup"), (8, "unique_apply"), (6, "lookup")])
def test_C_probe_chains_that_wrap_tombstones_and_rebuilds(ops, D, via):
  """every key's home is slot `mask` of the index (capacity_hint = 64: it starts small and is rebuilt by growth): the
  chain wraps to slot 0 — key 0's home, mix64(0) == 0 — and must never step into the sentinel's slot mask + 1"""
  rng = np.random.default_rng(109)
  rig = Rig(ops, D, prefill=0)
  IMIN = hk.INT64_MIN
  allk = hk.case("C")
  first = np.concatenate([allk[:300], allk[-4:]])                  # 300 last_home keys + the edge keys
  more = allk[300:500]
  rig.seen = [allk, rig.absent]

  def insert(keys):
    if via == "lookup":
      rig.lookup(keys)
    else:                                                          # uniq_insert's own probe loop (kv_uapply.h)
      g = grads(rng, keys.size, D)
      rig.apply(keys.copy(), g, unique_indices=True); rig.step(keys, g)
  # 1. inserted over three calls; all found
  for part in np.array_split(rng.permutation(first), 3):
    insert(part)
  rig.check(first, "C1")
  # 2. every third key deleted, INT64_MIN among them and 0 not
  dead = np.unique(np.concatenate([first[::3][first[::3] != 0], [IMIN]]))
  for p in (rig.var, rig.slot):
    assert ops.kv_variable_delete(p.h, dead) == p.o.delete(dead)
  rig.check(first, "C2")
  assert ops.kv_get_meta(rig.var.h, [0])[0] is not None and ops.kv_get_meta(rig.var.h, [IMIN]) == [None]
  assert not ops.kv_variable_gather_or_zeros_v2(rig.var.h, [IMIN]).any()
  assert int(ops.kv_variable_get_count_v2(rig.var.h, [IMIN])[0]) == 0
  # 3. revived; 200 more chained behind; 0 deleted, INT64_MIN kept
  insert(rng.permutation(dead))
  insert(more)
  z = np.array([0], np.int64)
  for p in (rig.var, rig.slot):
    assert ops.kv_variable_delete(p.h, z) == p.o.delete(z)
  rig.check(allk, "C3")
  assert ops.kv_get_meta(rig.var.h, [0]) == [None] and ops.kv_get_meta(rig.var.h, [IMIN])[0] is not None
  # 4. the index rebuilt by kv_reserve, and again by growth
  ops.kv_reserve(rig.var.h, 5000); ops.kv_reserve(rig.slot.h, 5000)
  rig.check(allk, "C4 reserve")
  bulk = np.unique(rng.integers(-(1 << 62), 1 << 62, 60000))
  rig.lookup(bulk)
  rig.seen.append(bulk[:2000])
  rig.check(allk, "C4 growth")
  # 5. export -> import and delta export -> delta import, into this table and into a fresh one, sentinel live, then deleted
  fresh = Pair(ops, D, np.zeros((4, D), F), 7)
  for sentinel_live in (True, False):
    if not sentinel_live:
      s = np.array([IMIN], np.int64)
      assert ops.kv_variable_delete(rig.var.h, s) == rig.var.o.delete(s) == 1
    tag = "C5 sentinel %s" % ("live" if sentinel_live else "deleted")
    k, v, bl, fk, fv = ops.kv_variable_export(rig.var.h, first_n=6)
    ok, ov, obl, ofk, ofv = rig.var.o.export(6)
    kk = k.cpu().numpy()
    assert np.array_equal(np.sort(kk), np.sort(ok)) and (IMIN in kk) == sentinel_live, tag
    np.testing.assert_array_equal(v.cpu().numpy()[np.argsort(kk)], ov[np.argsort(ok)], err_msg=tag)
    for tgt in (rig.var, fresh):
      ops.kv_variable_import(tgt.h, k, v, bl, fk, fv)
      tgt.o.import_(ok, ov, obl, ofk, ofv)
      tgt.check(np.concatenate([allk, rig.absent, bulk[:2000]]), tag + " import")
    # delta: the keys touched since tracking began — the sentinel (when live), key 0 and -1 looked up, one key deleted
    for tgt in (rig.var, fresh):
      ops.kv_set_delta_tracking(tgt.h, True); tgt.o.set_delta_tracking(True)
    touch = np.array(([IMIN] if sentinel_live else []) + [0, -1, int(more[0])], np.int64)
    np.testing.assert_array_equal(ops.kv_variable_gather_or_insert_v2(rig.var.h, touch).cpu().numpy(),
                                  rig.var.o.gather_or_insert(touch))
    gone = np.array([int(more[1 + sentinel_live])], np.int64)
    assert ops.kv_variable_delete(rig.var.h, gone) == rig.var.o.delete(gone) == 1
    dk_, dv, dbl, dfk, dfv, full, ddel = ops.kv_variable_full_or_delta_export(rig.var.h, False, first_n=6)
    o_k, o_v, o_bl, o_fk, o_fv, o_del = rig.var.o.export_delta(6)
    assert not full and sorted(dk_.cpu().tolist()) == sorted(o_k.tolist()), tag
    assert sorted(ddel.cpu().tolist()) == sorted(o_del.tolist()) and (IMIN in dk_.cpu().tolist()) == sentinel_live, tag
    ops.kv_variable_full_or_delta_import(fresh.h, dk_, dv, dbl, dfk, dfv, need_full_import=False, delete_keys=ddel)
    fresh.o.import_delta(o_k, o_v, o_bl, o_fk, o_fv, o_del)
    for tgt in (rig.var, fresh):
      ops.kv_set_delta_tracking(tgt.h, False); tgt.o.set_delta_tracking(False)
      tgt.check(np.concatenate([allk, rig.absent, bulk[:2000]]), tag + " delta")
  # 6. expiry with the sentinel among the expired: it alone is looked up on an early day, the rest later
  s = np.array([IMIN], np.int64)
  for p in (rig.var, fresh):
    p.set_day(DAY0 + 2)
    np.testing.assert_array_equal(ops.kv_variable_gather_or_insert_v2(p.h, s).cpu().numpy(), p.o.gather_or_insert(s))
    p.set_day(DAY0 + 9)
    keep = allk[:100]
    np.testing.assert_array_equal(ops.kv_variable_gather_or_insert_v2(p.h, keep).cpu().numpy(), p.o.gather_or_insert(keep))
    got = sorted(ops.kv_variable_delete_with_timestamp(p.h, 5).cpu().tolist())
    assert got == sorted(p.o.delete_with_timestamp(5).tolist()) and IMIN in got and int(keep[0]) not in got
    p.check(np.concatenate([allk, rig.absent, bulk[:2000]]), "C6")
