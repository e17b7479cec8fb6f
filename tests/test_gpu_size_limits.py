"""How long a batch is: calls that the chunk loops of kv_ops.hip cut into passes (section A), the largest batch one index
pass takes (section B), and caller's buffers of more than 2^31 elements (section C).  tests/_size_cases.py states the
limits and builds the inputs; tests/test_size_cases.py checks both on the CPU.

Every input is a device tensor and every wide expectation is computed with torch on the device.  References: the CPU
oracle where a case has at most 300 k distinct keys, else key_row — a row that is an exact function of its key — and
integer-valued gradients and updates, whose sums are exact in any order.  Everything is compared bit for bit except the
Adagrad state, held to 1e-6 relative against the float64 step (adagrad_ref; rows are integers and the step stays below
0.05, so no element cancels: tests/test_size_cases.py).

Two cases differ from what one pass computes only by refusing: an optimizer call takes at most one index pass of ids
(2^23 at the dims of the entry-list kernels, 2^21 elsewhere), so the apply that would follow a chunked lookup is refused
on the host with KV_UNIMPLEMENTED (the status the optimizer ops have always given an over-long batch), with the table
untouched.  The sorted-position pipeline's pass runs at dim 257, the smallest dim outside the entry-list kernels — a
scalar row copy and an odd `off * dim`; its lookups, insert, export and import serve every dim — and at dim 260, the
smallest such dim the optimizer ops serve too.

Each case first checks the free HBM against its need (the HBM in use when the case ended on an otherwise idle MI355X,
rounded up) and skips below it; each prints the HBM in use when it ends (`pytest -s`)."""
import os
import sys

import numpy as np
import pytest

from oracle import kv_oracle as ko

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _size_cases as S  # noqa: E402

from tfplus_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DAY = 20000
READ = 1 << 20          # rows per read-back call: a length the rest of the suite covers
ADD, MUL = 1, 3         # kv_scatter_update's operation codes (the oracle's too)


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


@pytest.fixture(scope="module")
def dev():
  return torch.device("cuda", 0)


def _need_hbm(gib):
  torch.cuda.empty_cache()            # what earlier cases freed counts as free
  free, _ = torch.cuda.mem_get_info()
  if free < gib * (1 << 30):
    pytest.skip("needs %d GiB of free HBM, has %.0f" % (gib, free / (1 << 30)))


def _hbm(what):
  torch.cuda.synchronize()
  free, total = torch.cuda.mem_get_info()
  print("%s: %.1f GiB of HBM in use" % (what, (total - free) / (1 << 30)))


def _init_table(D, value=None):
  if value is not None:
    return np.full((4, D), value, np.float32)
  return np.random.default_rng(S.SEED + D).standard_normal((64, D)).astype(np.float32)


def _table(ops, D, key_dtype=torch.int64, hint=0, value=None, seed=7):
  h = ops.kv_variable([D], key_dtype=key_dtype, capacity_hint=hint)
  ops.kv_set_clock_days(h, DAY); ops.kv_set_seed(h, seed); ops.init_kv_variable_v2(h, _init_table(D, value))
  return h


def _oracle(D, value=None, seed=7):
  return ko.OracleKv(D, 0, _init_table(D, value), day=DAY, picker=1, seed=seed)


def _figures(ops, h):
  return ops.kv_variable_shape_v2(h)[0], ops.kv_variable_size_v2(h), ops.kv_variable_frequency(h)


def _read(ops, h, keys):
  """gather_or_zeros of `keys` in calls of READ"""
  return torch.cat([ops.kv_variable_gather_or_zeros_v2(h, keys[i:i + READ]) for i in range(0, keys.numel(), READ)])


def _insert(ops, h, keys, D, step=READ, sign=1.0):
  for i in range(0, keys.numel(), step):
    ops.kv_variable_insert_v2(h, keys[i:i + step], S.key_row(keys[i:i + step], D) * sign)


def _by_key(keys, *cols):
  order = torch.argsort(keys)
  return [keys[order]] + [c[order] for c in cols]


# ------------------------------------------------------------------------------------------------------------------------
# A. chunk boundaries
# ------------------------------------------------------------------------------------------------------------------------
def _class_checks(ops, h, ov, s, d_count=S.FREQ_MAX):
  """map size, size, sum of frequencies; frequency and day stamp of the keys of every class, all against the oracle"""
  assert _figures(ops, h) == (ov.map_size(), ov.size(), ov.sum_freq())
  ck, names = S.class_keys(s)                                      # every key of a, b and c; d; the two of e
  for what, got, want in (
      ("frequency", ops.kv_variable_get_count_v2(h, torch.from_numpy(ck)).cpu().numpy(), ov.get_count(ck)),
      ("day stamp", ops.kv_variable_get_time_stamp(h, torch.from_numpy(ck)).cpu().numpy(), ov.get_timestamp(ck).astype(np.int64))):
    bad = np.flatnonzero(got != want)
    if bad.size:
      first = {str(c): int(bad[names[bad] == c][0]) for c in np.unique(names[bad])}      # the first mismatch of every class
      raise AssertionError("%s: %d keys differ; %s" % (what, bad.size, "; ".join(
          "class %s: key %d got %d want %d" % (c, ck[i], got[i], want[i]) for c, i in sorted(first.items()))))
    if what == "frequency":
      assert d_count is None or got[-3] == d_count                 # d after a lookup: 65534 before the boundary, 2 after it


def _counts_for(s):
  """int32 counts in {1, 2, 3} before the boundary and 7 after it: a counts pointer that does not advance with the ids
  gives the keys of class c a frequency other than 7"""
  rng = np.random.default_rng(S.SEED + 1)
  c = rng.integers(1, 4, s["ids"].size).astype(np.int32)
  c[s["chunk"]:] = 7
  return c


def _chunked_lookup(ops, dev, name, D, key_dtype, form):
  _need_hbm(4 if D == 4 else 12)
  s = S.straddle_case(name)
  ids = s["ids"]
  assert ids.size > (S.FUSED_MAX_N if D == 4 else S.OTHER_DIM_MAX_N)
  counts = None if form == "plain" else _counts_for(s)
  ov = _oracle(D)
  want = ov.gather_or_insert(ids, counts)
  h = _table(ops, D, key_dtype, hint=64)                           # grows inside the first pass
  ids_t = torch.from_numpy(ids).to(dev).to(key_dtype)
  if form == "plain":
    out = ops.kv_variable_gather_or_insert_v2(h, ids_t)
  elif form == "counts":
    out = ops.kv_variable_gather_or_insert_with_counts(h, ids_t, torch.from_numpy(counts).to(dev))
  else:
    pairs = torch.stack([ids_t, torch.from_numpy(counts).to(dev).to(torch.int64)], 1)
    out = ops.kv_variable_gather_or_insert_pairs(h, pairs)
  want_t = torch.from_numpy(want).to(dev)
  if not torch.equal(out, want_t):
    bad = torch.nonzero((out != want_t).any(1)).squeeze(1)
    raise AssertionError("%d rows differ, first at position %d (boundary %d), last at %d" %
                         (bad.numel(), int(bad[0]), s["chunk"], int(bad[-1])))
  _class_checks(ops, h, ov, s)
  if form != "pairs":
    # more ids than one index pass: no token, and the optimizer call that would follow is refused before it queues anything
    assert h.batch is None
    acc = _table(ops, D, key_dtype, value=0.1)
    grad = torch.ones((ids.size, D), device=dev)
    before = _figures(ops, h), _figures(ops, acc)
    for i in (ids_t, ids_t.clone()):                               # the lookup's own tensor (token 0), and no token
      with pytest.raises(_lib.UnimplementedError, match="ids in one optimizer call"):
        ops.kv_variable_sparse_apply_adagrad(h, acc, 0.05, grad, i)
    assert (_figures(ops, h), _figures(ops, acc)) == before
    ck = torch.from_numpy(S.class_keys(s)[0]).to(dev)
    assert torch.equal(ops.kv_variable_gather_or_zeros_v2(h, ck), torch.from_numpy(ov.gather_or_zeros(ck.cpu().numpy())).to(dev))
  _hbm("%s dim %d %s" % (name, D, form))


@pytest.mark.parametrize("name,key_dtype,form", [
    ("fused+3", torch.int64, "plain"), ("fused+3", torch.int64, "counts"), ("fused-int32+3", torch.int32, "plain"),
    ("fused-x2", torch.int64, "plain"), ("fused+3", torch.int64, "pairs")],
    ids=["2^23+3", "2^23+3-counts", "2^23+3-int32", "2x2^23", "2^23+3-pairs"])
def test_lookup_in_two_passes_dim4(ops, dev, name, key_dtype, form):
  """A.1 and A.3: kv_gather_or_insert, _with_counts and _pairs (8-, 4- and 16-byte id strides) over 2^23 + 3 and 2 x 2^23
  ids: rows, figures, and every class's frequency and day stamp equal the oracle's one pass."""
  _chunked_lookup(ops, dev, name, 4, key_dtype, form)


@pytest.mark.parametrize("form", ["plain", "counts"])
@pytest.mark.parametrize("D", [S.NONFUSED_DIM, S.NONFUSED_DIM4])
def test_lookup_in_two_passes_beyond_the_fused_dims(ops, dev, D, form):
  """A.2: the sorted-position pipeline's pass of 2^21 ids at dim 257 (scalar rows, the smallest dim outside the entry-list
  kernels) and dim 260 (float4 rows).  Needs about 12 GiB."""
  _chunked_lookup(ops, dev, "other+3", D, torch.int64, form)


@pytest.fixture(scope="module")
def inserted22(ops, dev):
  """A.4's table: 2^22 distinct keys in ONE kv_insert (two full chunks), rows key_row, into a table that grows"""
  n = 1 << 22
  gen = torch.Generator(device=dev).manual_seed(S.SEED)
  keys = S.distinct_keys(n, dev)[torch.randperm(n, device=dev, generator=gen)]
  h = _table(ops, 4, hint=64)
  ops.kv_variable_insert_v2(h, keys, S.key_row(keys, 4))
  return h, keys


def _insert_rule(ops, h, keys, n_distinct):
  """frequencies after an insert of distinct keys follow what the oracle shows on a 5000-key sample"""
  sample = keys[:5000].cpu().numpy()
  ov = _oracle(4)
  ov.insert(sample, S.key_row(torch.from_numpy(sample), 4).numpy())
  np.testing.assert_array_equal(ops.kv_variable_get_count_v2(h, keys[:5000]).cpu().numpy(), ov.get_count(sample))
  per = ov.sum_freq() // 5000
  assert ov.sum_freq() == per * 5000 and ov.map_size() == ov.size() == 5000
  assert _figures(ops, h) == (n_distinct, n_distinct, per * n_distinct)


def test_insert_two_chunks_and_a_tail(ops, dev):
  """A.4, n = 2^21 + 3: the last three keys and their rows are read at ids + off and values + off * dim"""
  _need_hbm(10)
  n = S.SCATTER_CHUNK + 3
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 4)
  keys = S.distinct_keys(n, dev)[torch.randperm(n, device=dev, generator=gen)]
  h = _table(ops, 4, hint=64)
  ops.kv_variable_insert_v2(h, keys, S.key_row(keys, 4))
  got = _read(ops, h, keys)
  want = S.key_row(keys, 4)
  assert torch.equal(got[-3:], want[-3:]), (got[-3:], want[-3:])
  assert torch.equal(got, want)
  _insert_rule(ops, h, keys, n)
  _hbm("insert 2^21 + 3")


def test_insert_two_full_chunks(ops, inserted22):
  """A.4, n = 2^22"""
  _need_hbm(10)
  h, keys = inserted22
  assert torch.equal(_read(ops, h, keys), S.key_row(keys, 4))
  _insert_rule(ops, h, keys, keys.numel())


def test_insert_repeated_ids_across_the_boundary(ops, dev):
  """A.4 with repeats: which occurrence of a repeated id stays is unspecified for assign, so every occurrence carries the
  same row; key set and frequencies are the oracle's"""
  _need_hbm(10)
  s = S.straddle_case("other+3")
  ids = torch.from_numpy(s["ids"]).to(dev)
  ov = _oracle(4)
  ov.insert(s["ids"], S.key_row(torch.from_numpy(s["ids"]), 4).numpy())
  h = _table(ops, 4, hint=64)
  ops.kv_variable_insert_v2(h, ids, S.key_row(ids, 4))
  _class_checks(ops, h, ov, s, d_count=1)                          # an insert counts a key once, however often it is listed
  u = torch.unique(ids)
  assert torch.equal(_read(ops, h, u), S.key_row(u, 4))


@pytest.mark.parametrize("op", [ADD, MUL], ids=["add", "mul"])
def test_folding_scatter_update_across_the_boundary(ops, dev, op):
  """A.5: integer addends; factors from {1, 2, 0.5}, at most ~100 of a key's factors other than 1, so every partial product
  in any order is a row element times a power of two inside fp32's range: both are exact, compared bit for bit with the
  oracle's occurrence-by-occurrence update of the whole call"""
  _need_hbm(10)
  s = S.straddle_case("other+3")
  ids_np = s["ids"]
  ids = torch.from_numpy(ids_np).to(dev)
  u, inv, cnt = torch.unique(ids, return_inverse=True, return_counts=True)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + op)
  if op == ADD:
    upd = S.draw_int_rows(ids.numel(), 4, gen, dev)
  else:
    r = torch.rand((ids.numel(), 4), device=dev, generator=gen)
    p = (48.0 / cnt[inv].double()).clamp(max=1.0).float().unsqueeze(1)
    upd = torch.where(r < p / 2, 2.0, torch.where(r < p, 0.5, 1.0)).float()
    other = torch.zeros((u.numel(), 4), device=dev).index_add_(0, inv, (upd != 1).float())
    assert 10 < other.max().item() <= 110 and (other.sum(1) > 0).float().mean().item() > 0.5
  ov = _oracle(4)
  rows0 = S.key_row(u, 4)
  ov.insert(u.cpu().numpy(), rows0.cpu().numpy())
  ov.scatter_update(ids_np, upd.cpu().numpy(), op)
  h = _table(ops, 4, hint=u.numel() + 1024)
  ops.kv_variable_insert_v2(h, u, rows0)
  (ops.kv_variable_scatter_add_v2 if op == ADD else ops.kv_variable_scatter_mul_v2)(h, ids, upd)
  got = ops.kv_variable_gather_or_zeros_v2(h, u)
  want = torch.from_numpy(ov.gather_or_zeros(u.cpu().numpy())).to(dev)
  for cls in ("c", "d", "e"):
    k = torch.as_tensor(np.atleast_1d(np.asarray(s[cls], np.int64))[:2000]).to(dev)
    at = torch.searchsorted(u, k)
    assert torch.equal(got[at], want[at]), "class %s" % cls
  assert torch.equal(got, want)
  assert not torch.equal(got, rows0)
  _class_checks(ops, h, ov, s, d_count=None)                       # frequencies and day stamps: whatever the oracle's update leaves


def _freq_words(keys):
  """a frequency word per key: day DAY - 3, a count in 1..1000 that depends on the key"""
  return (((DAY - 3) << 16) | (keys % 1000 + 1)).to(torch.int32)


def test_import_export_round_trips(ops, dev, inserted22):
  """A.6: export(first_n = 6) of 2^22 keys -> import into a fresh table -> export: the same lists as key-sorted arrays.
  Then lists a checkpoint could hold: 5000 keys on the blacklist and a frequency word per key that depends on the key, so
  every stage's pointers (keys, values + off * dim, frequency keys and words + off) show in the second table's export."""
  _need_hbm(12)
  h, _ = inserted22
  n = 1 << 22
  k1, v1, b1, fk1, fv1 = ops.kv_variable_export(h, first_n=6)
  assert k1.numel() == n == fk1.numel() and b1.numel() == 0
  k1s, v1s = _by_key(k1, v1)
  assert torch.equal(v1s, S.key_row(k1s, 4))
  h2 = ops.kv_variable([4], capacity_hint=64)
  ops.kv_variable_import(h2, k1, v1, b1, fk1, fv1)
  k2, v2, b2, fk2, fv2 = ops.kv_variable_export(h2, first_n=6)
  assert all(torch.equal(x, y) for x, y in zip(_by_key(k1, v1), _by_key(k2, v2)))
  assert all(torch.equal(x, y) for x, y in zip(_by_key(fk1, fv1), _by_key(fk2, fv2))) and b2.numel() == 0
  # second round
  black = k1s[::839][:5000].contiguous()
  keep = torch.ones(n, dtype=torch.bool, device=dev)
  keep[torch.searchsorted(k1s, black)] = False
  kk, vv = k1s[keep], v1s[keep]
  perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(S.SEED + 6))
  fk = k1s[perm]                                                   # the frequency list in another order than the keys
  fv = _freq_words(fk)
  assert fk.numel() > S.SCATTER_CHUNK and kk.numel() > S.SCATTER_CHUNK
  h3 = ops.kv_variable([4], capacity_hint=64)
  ops.kv_variable_import(h3, kk, vv, black, fk, fv)
  k3, v3, b3, fk3, fv3 = ops.kv_variable_export(h3, first_n=6)
  k3s, v3s = _by_key(k3, v3)
  assert torch.equal(k3s, kk) and torch.equal(v3s, vv)
  assert torch.equal(torch.sort(b3).values, black)
  fk3s, fv3s = _by_key(fk3, fv3)
  assert torch.equal(fk3s, k1s) and torch.equal(fv3s, _freq_words(k1s))
  assert ops.kv_variable_shape_v2(h3)[0] == n
  _hbm("import / export")


def test_import_delta_every_list_beyond_a_chunk(ops, dev, inserted22):
  """A.7: kv_import_delta with n, n_freq and n_delete each above 2^21 onto a copy of A.4's table: the updated keys read
  minus key_row (overwritten and new ones alike), the deleted keys are gone, the rest reads key_row"""
  _need_hbm(12)
  h, _ = inserted22
  n = 1 << 22
  m = S.SCATTER_CHUNK + 5
  k1, v1, b1, fk1, fv1 = ops.kv_variable_export(h, first_n=6)
  t = ops.kv_variable([4], capacity_hint=64)
  ops.kv_variable_import(t, k1, v1, b1, fk1, fv1)
  old = S.distinct_keys(n, dev)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 7)
  old = old[torch.randperm(n, device=dev, generator=gen)]
  over, gone, stay = old[:m // 2], old[m // 2:m // 2 + m + 2], old[m // 2 + m + 2:]
  new = S.distinct_keys(m - m // 2, dev, start=n + 1)
  upd = torch.cat([over, new])[torch.randperm(m, device=dev, generator=gen)]
  assert upd.numel() > S.SCATTER_CHUNK and gone.numel() > S.SCATTER_CHUNK
  fv = _freq_words(upd)
  ops.kv_variable_full_or_delta_import(t, upd, -S.key_row(upd, 4), None, upd, fv, need_full_import=False, delete_keys=gone)
  assert ops.kv_variable_shape_v2(t)[0] == n + new.numel() - gone.numel()
  k, v = ops.read_kv_variable_op_v2(t)
  ks, vs = _by_key(k, v)
  assert torch.equal(ks, torch.sort(torch.cat([upd, stay])).values)
  is_upd = torch.isin(ks, upd)
  want = S.key_row(ks, 4)
  want[is_upd] = -want[is_upd]
  assert torch.equal(vs, want)
  assert torch.equal(_read(ops, t, upd[-3:]), -S.key_row(upd[-3:], 4))                  # the tail of the second chunk
  assert not bool(_read(ops, t, gone).any())
  sample = torch.cat([upd[:2500], upd[-2500:]])
  assert torch.equal(ops.kv_variable_get_count_v2(t, sample), (sample % 1000 + 1).to(torch.int32))
  _hbm("import delta")


# ------------------------------------------------------------------------------------------------------------------------
# B. the largest batch one index pass takes
# ------------------------------------------------------------------------------------------------------------------------
LR = 0.05


class _Big(object):
  """var (keys pre-inserted with key_row, in calls of 2^20) + Adagrad accumulator (rows start at 0.1), n ids, gradients"""

  def __init__(self, ops, dev, keys, ids, grad):
    self.var = _table(ops, 4, hint=keys.numel() + (1 << 16))
    self.acc = _table(ops, 4, hint=keys.numel() + (1 << 16), value=0.1)
    _insert(ops, self.var, keys, 4)
    self.keys, self.ids, self.grad = keys, ids, grad


@pytest.fixture(scope="module")
def distinct(ops, dev):
  """2^23 distinct ids in random order and integer gradients; the expected Adagrad state of every key"""
  n = S.FUSED_MAX_N
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 20)
  keys = S.distinct_keys(n, dev)
  ids = keys[torch.randperm(n, device=dev, generator=gen)]
  grad = S.draw_int_rows(n, 4, gen, dev)
  x1, a1 = S.adagrad_ref(S.key_row(ids, 4), torch.full((n, 4), float(np.float32(0.1)), device=dev), grad, LR)
  return dict(keys=keys, ids=ids, grad=grad, x1=x1, a1=a1, tables={})


def _close(got, want):
  """1e-6 relative on every element (the bar of an update of ids that occur once)"""
  err = (got.double() - want).abs()
  bad = err > 1e-6 * want.abs()
  assert not bool(bad.any()), "%d elements, worst %.3g relative" % (int(bad.sum()), (err[bad] / want[bad].abs()).max().item())


def _lookup_then_adagrad(ops, dev, d, with_token):
  n = S.FUSED_MAX_N
  b = _Big(ops, dev, d["keys"], d["ids"], d["grad"])
  f0 = ops.kv_variable_frequency(b.var)
  out = ops.kv_variable_gather_or_insert_v2(b.var, b.ids)
  assert torch.equal(out, S.key_row(b.ids, 4))
  assert ops.kv_variable_frequency(b.var) - f0 == n and ops.kv_variable_shape_v2(b.var)[0] == n
  assert b.var.batch is not None and b.var.batch[0] != 0           # exactly 2^23 ids: one pass indexes them, a token names it
  ops.kv_variable_sparse_apply_adagrad(b.var, b.acc, LR, b.grad, b.ids if with_token else b.ids.clone())
  return b


def test_largest_batch_lookup_and_adagrad(ops, dev, distinct):
  """B.1, B.2: 2^23 distinct ids (8192 keys per partition block at 1024 partitions): the lookup returns key_row and counts
  every id once; Adagrad with the lookup's token leaves every key's row and accumulator at the float64 step; without the
  token (the optimizer's own index pass) a twin pair ends bit-identical"""
  _need_hbm(18)
  d = distinct
  b = _lookup_then_adagrad(ops, dev, d, True)
  x, a = _read(ops, b.var, d["ids"]), _read(ops, b.acc, d["ids"])
  _close(x, d["x1"]); _close(a, d["a1"])
  assert ops.kv_variable_shape_v2(b.acc)[0] == S.FUSED_MAX_N
  t = _lookup_then_adagrad(ops, dev, d, False)
  assert torch.equal(_read(ops, t.var, d["ids"]), x) and torch.equal(_read(ops, t.acc, d["ids"]), a)
  d["tables"]["x"], d["tables"]["a"] = x, a
  _hbm("2^23 distinct ids: lookup + Adagrad, twice")


def test_largest_batch_unique_and_dedup(ops, dev, distinct):
  """B.3: kv_unique and kv_dedup_segment_sum of 2^23 distinct ids"""
  _need_hbm(12)
  d = distinct
  n = S.FUSED_MAX_N
  h = _table(ops, 4)
  uniq, ucnt, inv = ops.kv_unique(h, d["ids"])
  assert uniq.numel() == n and torch.equal(uniq[inv.long()], d["ids"]) and bool((ucnt == 1).all())
  uniq, summed, inv = ops.kv_dedup_segment_sum(h, d["ids"], d["grad"])
  assert uniq.numel() == n and torch.equal(uniq[inv.long()], d["ids"])
  assert torch.equal(summed[inv.long()], d["grad"])
  _hbm("2^23 distinct ids: unique + dedup")


def test_largest_batch_in_a_batched_call(ops, dev, distinct):
  """B.4: kv_multi_gather_or_insert and kv_multi_sparse_apply_adagrad over tables with 2^23, 1 and 0 ids: the first pair
  ends bit-identical to the single-table run"""
  _need_hbm(14)
  d = distinct
  if "x" not in d["tables"]:                                         # (run alone: the single-table result first)
    s1 = _lookup_then_adagrad(ops, dev, d, True)
    d["tables"]["x"], d["tables"]["a"] = _read(ops, s1.var, d["ids"]), _read(ops, s1.acc, d["ids"])
    del s1
  n = S.FUSED_MAX_N
  b = _Big(ops, dev, d["keys"], d["ids"], d["grad"])
  vars_ = [b.var, _table(ops, 4), _table(ops, 4)]
  accs = [b.acc, _table(ops, 4, value=0.1), _table(ops, 4, value=0.1)]
  one = d["keys"][:1].clone()
  ids = [d["ids"], one, torch.empty(0, dtype=torch.int64, device=dev)]
  grads = [d["grad"], torch.ones((1, 4), device=dev), torch.empty((0, 4), device=dev)]
  _insert(ops, vars_[1], one, 4)
  outs = ops.kv_multi_gather_or_insert(vars_, ids)
  assert torch.equal(outs[0], S.key_row(d["ids"], 4)) and outs[1].shape == (1, 4) and outs[2].shape == (0, 4)
  assert vars_[0].batch is not None and vars_[0].batch[0] != 0
  ops.kv_multi_sparse_apply_adagrad(vars_, accs, LR, grads, ids)
  assert torch.equal(_read(ops, b.var, d["ids"]), d["tables"]["x"]) and torch.equal(_read(ops, b.acc, d["ids"]), d["tables"]["a"])
  assert [ops.kv_variable_shape_v2(v)[0] for v in vars_] == [n, 1, 0]
  x1, a1 = S.adagrad_ref(outs[1], torch.full((1, 4), float(np.float32(0.1)), device=dev), grads[1], LR)
  _close(ops.kv_variable_gather_or_zeros_v2(vars_[1], one), x1); _close(ops.kv_variable_gather_or_zeros_v2(accs[1], one), a1)
  _hbm("2^23 distinct ids: batched call")


def test_largest_batch_every_key_in_every_tile(ops, dev):
  """B.5: 2^23 ids over 1024 keys — 8192 rows a key, two per tile on average — against the oracle: lookup rows and figures
  bit for bit; unique and dedup sums bit for bit (integer gradients); Adagrad with and without token, and batched, within
  1e-6 of the oracle's step on the exact sums"""
  _need_hbm(14)
  n, K = S.FUSED_MAX_N, 1024
  rng = np.random.default_rng(S.SEED + 25)
  keys = S.draw_keys(rng, K)
  ids_np = keys[rng.integers(0, K, n)]
  assert np.unique(ids_np[:S.TILE]).size > K // 2
  ids = torch.from_numpy(ids_np).to(dev)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 25)
  grad = S.draw_int_rows(n, 4, gen, dev)
  u = torch.unique(ids)
  rows0 = S.key_row(u, 4)                                            # integer rows: no element of the step cancels
  ov, oa = _oracle(4), _oracle(4, value=0.1)
  ov.insert(u.cpu().numpy(), rows0.cpu().numpy())
  want = torch.from_numpy(ov.gather_or_insert(ids_np)).to(dev)
  figures = ov.map_size(), ov.size(), ov.sum_freq()
  gsum = torch.zeros((K, 4), dtype=torch.float64, device=dev).index_add_(0, torch.searchsorted(u, ids), grad.double())
  assert gsum.abs().max().item() < 1 << 24
  u_np = u.cpu().numpy()
  ko.apply_adagrad(ov, oa, LR, gsum.float().cpu().numpy(), u_np)
  wx, wa = ov.gather_or_zeros(u_np), oa.gather_or_zeros(u_np)
  results = []
  for form in ("token", "no token", "batched"):
    var, acc = _table(ops, 4), _table(ops, 4, value=0.1)
    ops.kv_variable_insert_v2(var, u, rows0)
    if form == "batched":
      out = ops.kv_multi_gather_or_insert([var], [ids])[0]
    else:
      out = ops.kv_variable_gather_or_insert_v2(var, ids)
    assert torch.equal(out, want), form
    assert var.batch is not None and var.batch[0] != 0
    assert _figures(ops, var) == figures
    if form == "batched":
      ops.kv_multi_sparse_apply_adagrad([var], [acc], LR, [grad], [ids])
    else:
      ops.kv_variable_sparse_apply_adagrad(var, acc, LR, grad, ids if form == "token" else ids.clone())
    x, a = ops.kv_variable_gather_or_zeros_v2(var, u).cpu().numpy(), ops.kv_variable_gather_or_zeros_v2(acc, u).cpu().numpy()
    np.testing.assert_allclose(x, wx, rtol=1e-6, atol=0, err_msg=form)
    np.testing.assert_allclose(a, wa, rtol=1e-6, atol=0, err_msg=form)
    results.append((x, a))
  assert all(np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1]) for r in results[1:])
  h = _table(ops, 4)
  uq, ucnt, inv = ops.kv_unique(h, ids)
  assert uq.numel() == K and torch.equal(uq[inv.long()], ids)
  assert torch.equal(_by_key(uq, ucnt)[1].long(), torch.bincount(torch.searchsorted(u, ids), minlength=K))
  uq, summed, inv = ops.kv_dedup_segment_sum(h, ids, grad)
  assert uq.numel() == K and torch.equal(uq[inv.long()], ids)
  assert torch.equal(_by_key(uq, summed)[1], gsum.float())
  _hbm("2^23 ids over 1024 keys")


# ------------------------------------------------------------------------------------------------------------------------
# C. wide buffers: dim 1024, caller's buffers of 2^31 elements and more
# ------------------------------------------------------------------------------------------------------------------------
# The lookups, kv_insert, kv_export / kv_import and the sparse lookups' `out` take S.WIDE_N = 2^21 + 4096 rows of dim 1024:
# the last two tiles lie wholly beyond element 2^31, byte offsets pass 2^31 and 2^32 on the way.  The optimizer ops,
# kv_dedup_segment_sum and kv_lookup_sparse_grad take at most 2^21 ids a call at this dim (kvhip.h): they run at exactly
# 2^21 rows — the last element is 2^31 - 1, byte offsets pass 2^32 — and the longer call is refused on the host.
WIDE_MAX = S.OTHER_DIM_MAX_N


def _wide_keys(dev):
  keys = S.distinct_keys(S.WIDE_KEYS + S.WIDE_TAIL_KEYS, dev)
  return keys[:S.WIDE_KEYS], keys[S.WIDE_KEYS:]


def _wide_ids(n, dev, seed):
  """n ids over 65536 keys; the last 4096 positions hold 512 keys that occur nowhere else"""
  main, tail = _wide_keys(dev)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + seed)
  head = main[torch.randint(0, main.numel(), (n - S.WIDE_TAIL,), generator=gen, device=dev)]
  last = tail[torch.randperm(S.WIDE_TAIL, device=dev, generator=gen) % tail.numel()]
  return torch.cat([head, last])


def _wide_table(ops, dev, D=S.WIDE_DIM):
  main, tail = _wide_keys(dev)
  keys = torch.cat([main, tail])
  h = _table(ops, D, hint=keys.numel() + 4096)
  _insert(ops, h, keys, D, step=1 << 18)
  return h, keys


def _equal_rows(got, ids, D, what):
  """got == key_row(ids), ROW_CHUNK rows at a time (the expectation of a wide buffer never exists as a whole)"""
  assert got.shape == (ids.numel(), D)
  for i in range(0, ids.numel(), S.ROW_CHUNK):
    want = S.key_row(ids[i:i + S.ROW_CHUNK], D)
    if not torch.equal(got[i:i + S.ROW_CHUNK], want):
      bad = torch.nonzero((got[i:i + S.ROW_CHUNK] != want).any(1)).squeeze(1)
      raise AssertionError("%s: %d rows differ in positions %d..%d, first %d (element 2^31 is in row %d)" %
                           (what, bad.numel(), i, i + want.shape[0] - 1, i + int(bad[0]), (1 << 31) // D))


def test_wide_lookups(ops, dev):
  """C.1: kv_gather_or_zeros, kv_gather_or_insert (two passes) and kv_batch_gather_or_zeros write 2^21 + 4096 rows of dim
  1024.  Needs about 25 GiB."""
  _need_hbm(25)
  h, keys = _wide_table(ops, dev)
  ids = _wide_ids(S.WIDE_N, dev, 31)
  assert ids.numel() * S.WIDE_DIM > 1 << 31
  f0 = ops.kv_variable_frequency(h)
  for what, fn in (("gather_or_zeros", lambda: ops.kv_variable_gather_or_zeros_v2(h, ids)),
                   ("gather_or_insert", lambda: ops.kv_variable_gather_or_insert_v2(h, ids)),
                   ("batch_gather_or_zeros", lambda: ops.batch_kv_variable_gather_or_zeros_v2([h], [ids])[0])):
    out = fn()
    _equal_rows(out[-S.WIDE_TAIL:], ids[-S.WIDE_TAIL:], S.WIDE_DIM, what + ", the tail keys")
    _equal_rows(out, ids, S.WIDE_DIM, what)
    del out
  assert ops.kv_variable_frequency(h) - f0 == S.WIDE_N and ops.kv_variable_shape_v2(h)[0] == keys.numel()
  _hbm("wide lookups")


def _sums_by_key(keys, ids, grad):
  """per-key gradient sums in fp32: integer addends, every partial sum below 2^24, so any order is exact"""
  at = torch.searchsorted(keys, ids)
  assert torch.equal(keys[at], ids)
  return torch.zeros((keys.numel(), grad.shape[1]), device=ids.device).index_add_(0, at, grad)


def test_wide_optimizer_calls(ops, dev):
  """C.2: kv_apply_adagrad plain, with the lookup's token and _unique after kv_dedup_segment_sum, and kv_apply_group_adam,
  over 2^21 ids and an 8 GiB gradient at dim 1024.  Adagrad: every key within 1e-6 of the float64 step on its exact
  gradient sum, the tail keys first.  GroupAdam: bit-identical to a twin pair that received the same (exact) sums in a
  call of unique ids.  2^21 + 4096 ids are refused.  Needs about 30 GiB."""
  _need_hbm(30)
  D, n = S.WIDE_DIM, WIDE_MAX
  main, tail = _wide_keys(dev)
  keys = torch.cat([main, tail])                                   # ascending
  ids = _wide_ids(n, dev, 32)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 32)
  full = torch.empty((S.WIDE_N, D), device=dev)                    # the refused call's gradient: never read
  grad = S.draw_int_rows(n, D, gen, dev, out=full)[:n]
  gsum = _sums_by_key(keys, ids, grad)
  assert gsum.abs().max().item() < 1 << 24 and bool((torch.bincount(torch.searchsorted(keys, ids), minlength=keys.numel()) > 0).all())
  x1, a1 = S.adagrad_ref(S.key_row(keys, D), torch.full((keys.numel(), D), float(np.float32(0.1)), device=dev), gsum, LR)
  nt = tail.numel()
  first = None
  for form in ("plain", "token", "unique"):
    var, _ = _wide_table(ops, dev)
    acc = _table(ops, D, hint=keys.numel() + 4096, value=0.1)
    if form == "plain":
      ops.kv_variable_sparse_apply_adagrad(var, acc, LR, grad, ids.clone())
    elif form == "token":
      out = ops.kv_variable_gather_or_insert_v2(var, ids)
      assert var.batch is not None and var.batch[0] != 0
      _equal_rows(out[-S.WIDE_TAIL:], ids[-S.WIDE_TAIL:], D, "lookup before the apply")
      del out
      ops.kv_variable_sparse_apply_adagrad(var, acc, LR, grad, ids)
    else:
      uniq, summed, inv = ops.kv_dedup_segment_sum(var, ids, grad)
      assert uniq.numel() == keys.numel() and torch.equal(uniq[inv.long()], ids)
      assert torch.equal(_by_key(uniq, summed)[1], gsum), "dedup sums"
      ops.kv_variable_sparse_apply_adagrad(var, acc, LR, summed, uniq, unique_indices=True)
      del summed
    x, a = ops.kv_variable_gather_or_zeros_v2(var, keys), ops.kv_variable_gather_or_zeros_v2(acc, keys)
    _close(x[-nt:], x1[-nt:]); _close(a[-nt:], a1[-nt:])          # the tail keys: their gradient rows end at element 2^31 - 1
    _close(x, x1); _close(a, a1)
    if first is None:
      first = x, a
    else:
      assert torch.equal(x, first[0]) and torch.equal(a, first[1]), form     # exact sums: every form takes the same step
    with pytest.raises(_lib.UnimplementedError, match="ids in one optimizer call"):
      ops.kv_variable_sparse_apply_adagrad(var, acc, LR, full, _wide_ids(S.WIDE_N, dev, 32))
    del var, acc, x, a
  # GroupAdam
  res = []
  for wide in (True, False):
    var, _ = _wide_table(ops, dev)
    slot = _table(ops, 3 * D, hint=keys.numel() + 4096, value=0.0)
    if wide:
      ops.kv_variable_group_sparse_apply_adam_v4(var, slot, grad, ids.clone(), 1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
    else:
      ops.kv_variable_group_sparse_apply_adam_v4(var, slot, gsum, keys, 1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 0, 0, 0)
    res.append((ops.kv_variable_gather_or_zeros_v2(var, keys), ops.kv_variable_gather_or_zeros_v2(slot, keys)))
    del var, slot
  assert torch.equal(res[0][0][-nt:], res[1][0][-nt:]) and torch.equal(res[0][1][-nt:], res[1][1][-nt:]), "tail keys"
  assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
  assert not torch.equal(res[0][0], S.key_row(keys, D))
  _hbm("wide optimizer calls")


def test_wide_dedup_of_distinct_ids(ops, dev):
  """C.3: kv_dedup_segment_sum of 2^21 distinct ids at dim 1024: `summed` is 8 GiB.  Needs about 36 GiB."""
  _need_hbm(36)
  D, n = S.WIDE_DIM, WIDE_MAX
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 33)
  ids = S.distinct_keys(n, dev)[torch.randperm(n, device=dev, generator=gen)]
  full = torch.empty((S.WIDE_N, D), device=dev)                    # the refused call's gradient: never read
  grad = S.draw_int_rows(n, D, gen, dev, out=full)[:n]
  h = _table(ops, D)
  uniq, summed, inv = ops.kv_dedup_segment_sum(h, ids, grad)
  assert uniq.numel() == n and torch.equal(uniq[inv.long()], ids)
  inv = inv.long()
  for i in range(n - S.ROW_CHUNK, -1, -S.ROW_CHUNK):               # the last rows first: a wrapped offset names itself
    assert torch.equal(summed[inv[i:i + S.ROW_CHUNK]], grad[i:i + S.ROW_CHUNK]), "positions from %d" % i
  del summed
  with pytest.raises(_lib.UnimplementedError, match=r"ids in one call \(limit 2\^21\)"):
    ops.kv_dedup_segment_sum(h, S.distinct_keys(S.WIDE_N, dev), full)
  _hbm("wide dedup")


def test_wide_insert_export_import(ops, dev):
  """C.4: kv_insert of 2^21 + 4096 distinct keys of dim 1024 in one call (the second chunk's values start beyond element
  2^31) into a table that grows; kv_export of that table (`values`: 8 GiB); kv_import of the export into another table,
  read back in calls of 2^18.  Needs about 45 GiB."""
  _need_hbm(45)
  D, n = S.WIDE_DIM, S.WIDE_N
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 34)
  keys = S.distinct_keys(n, dev)[torch.randperm(n, device=dev, generator=gen)]
  h = _table(ops, D, hint=64)
  rows = S.key_row(keys, D)
  ops.kv_variable_insert_v2(h, keys, rows)
  del rows
  assert ops.kv_variable_shape_v2(h)[0] == n
  last = keys[-S.WIDE_TAIL:]
  _equal_rows(ops.kv_variable_gather_or_zeros_v2(h, last), last, D, "the keys of the second chunk")
  k, v, bl, fk, fv = ops.kv_variable_export(h, first_n=6)
  assert k.numel() == n and v.shape == (n, D) and bl.numel() == 0 and fk.numel() == n
  assert torch.equal(torch.sort(k).values, torch.sort(keys).values)
  _equal_rows(v[-S.WIDE_TAIL:], k[-S.WIDE_TAIL:], D, "export, the last rows")     # (an export row goes with its key in any order)
  _equal_rows(v, k, D, "export")
  ops.destroy_kv_variable_op_v2(h)
  h2 = ops.kv_variable([D], capacity_hint=64)
  ops.kv_variable_import(h2, k, v, bl, fk, fv)
  del v
  assert ops.kv_variable_shape_v2(h2)[0] == n
  for i in range(n - (1 << 18), -1, -(1 << 18)):
    part = k[i:i + (1 << 18)]
    _equal_rows(ops.kv_variable_gather_or_zeros_v2(h2, part), part, D, "import, keys from %d" % i)
  _hbm("wide insert / export / import")


def test_wide_sparse_lookups(ops, dev):
  """C.5: kv_lookup_sparse and kv_lookup_sparse_zeros into 2^21 + 8 segments of dim 1024 (`out` passes 2^31 elements):
  4096 ids, half of them in the last 8 segments; sum and mean (every segment holds 0, 2 or 256 ids, so the mean's
  division is exact).  The backward over 2^21 positions and 16 segments: values[i] is the gradient row of position i's
  segment; 2^21 + 4096 positions are refused.  Needs about 40 GiB."""
  _need_hbm(40)
  D = S.WIDE_DIM
  nseg = WIDE_MAX + 8
  assert nseg * D > 1 << 31
  h, keys = _wide_table(ops, dev)
  gen = torch.Generator(device=dev).manual_seed(S.SEED + 35)
  ids = keys[torch.randint(0, keys.numel(), (4096,), generator=gen, device=dev)]
  seg = torch.cat([torch.arange(1024, device=dev).repeat_interleave(2) * 2039 + 5,            # 1024 segments of two ids
                   (nseg - 8 + torch.arange(8, device=dev)).repeat_interleave(256)])          # the last 8: 256 each
  assert seg.numel() == 4096 and bool((seg[1:] >= seg[:-1]).all()) and int(seg[2047]) < nseg - 8
  rows = S.key_row(ids, D)
  total = torch.zeros((nseg, D), device=dev).index_add_(0, seg, rows)      # integers below 2^24: exact in any order
  cnt = torch.bincount(seg, minlength=nseg).float().clamp(min=1).unsqueeze(1)
  for combiner in ("sum", "mean"):
    want = total if combiner == "sum" else total / cnt               # counts 1 (empty), 2, 256: exact quotients
    for what, fn in (("lookup_sparse", ops.kv_variable_lookup_sparse), ("lookup_sparse_zeros", ops.kv_variable_lookup_sparse_zeros)):
      out = fn(h, ids, seg, None, nseg, combiner=combiner)
      assert out.shape == (nseg, D)
      assert torch.equal(out[-8:], want[-8:]), (what, combiner, "the last 8 segments")
      assert bool(out[-8:].any(1).all())
      assert torch.equal(out, want), (what, combiner)
      del out
    del want
  del total, rows
  # backward
  n = WIDE_MAX
  gseg = S.draw_int_rows(16, D, gen, dev)
  pos_seg = torch.arange(n, device=dev) // (n // 16)
  values = ops.kv_variable_lookup_sparse_grad(h, gseg, pos_seg, None, 16, combiner="sum")
  assert values.shape == (n, D)
  assert torch.equal(values[-S.TILE:], gseg[pos_seg[-S.TILE:]])
  for i in range(0, n, S.ROW_CHUNK):
    assert torch.equal(values[i:i + S.ROW_CHUNK], gseg[pos_seg[i:i + S.ROW_CHUNK]]), "positions from %d" % i
  del values
  with pytest.raises(_lib.InvalidArgumentError, match=r"sp_ids: %d values \(at most 2\^21 per call\)" % S.WIDE_N):
    ops.kv_variable_lookup_sparse_grad(h, gseg, torch.zeros(S.WIDE_N, dtype=torch.int64, device=dev), None, 16, combiner="sum")
  _hbm("wide sparse lookups")
