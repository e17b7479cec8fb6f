"""Where every op of the C ABI writes: each output a caller hands in sits between guard bands and is prefilled with a
sentinel (tests/_guarded.py), each input is snapshotted and compared byte for byte afterwards.  An op must write ALL of the
extent kvhip.h defines (no element keeps the sentinel: a skipped row cannot read as the previous call's answer out of a
recycled allocation), ONLY that extent (the guards keep the sentinel in every byte: the lane of a masked row class that
stores its whole float4, a last partial tile that files one row too many) and must leave its inputs alone (`ids`,
`counts`, `grad`, `weights`, `segment_ids` are const, and the batch token relies on it).

Values are compared bit for bit against closed forms computed in numpy (tests/_extent_cases.py, held against the oracle
by tests/test_buffer_extents_cases.py): rows that are exact functions of their key, sums that are exact in every order.
Outputs whose order the header leaves open (unique lists, exports, bucket order) are compared keyed by id.

Shapes: every dim of _row_geometry.DIMS for the ops that move rows (plus 257 and 1028 where the op serves dims outside the
fused range), dims 4 and 100 for the others; n = 1, 65, TILE - 1, TILE + 1, the 2 172-id batch of _row_geometry for the
training lookups, and the zero-length calls, after which the whole buffer still holds the sentinel.  int32 and uint64
tables once each at dims 4 and 100 (the uint64 keys have their top bit set).

Every pointer handed to the library here is aligned as kvhip.h ("Buffers") asks: Guarded keeps row buffers on 16 bytes.
The last test holds the binding to its side of that contract: a gradient that is a view at an odd storage offset."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _extent_cases as X  # noqa: E402
from _extent_cases import ABSENT, BLACK, PRESENT, UNDER, F, NS, TILE  # noqa: E402
from _guarded import Guarded, frozen, same_bits  # noqa: E402
from tfplus_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

I32, I64, U64 = _lib.KV_DT_INT32, _lib.KV_DT_INT64, _lib.KV_DT_UINT64
KEY_DT = {"int64": I64, "int32": I32, "uint64": U64}
ROW_DIMS, WIDE_DIMS, SMALL_DIMS = X.ROW_DIMS, X.WIDE_DIMS, X.SMALL_DIMS
F4_DIMS = tuple(d for d in ROW_DIMS if d % 4 == 0)
COUNTED_DIMS = tuple(d for d in F4_DIMS if d <= 256)
KEYED = [(4, "int64"), (100, "int64"), (4, "int32"), (100, "int32"), (4, "uint64"), (100, "uint64")]
ALL_PARTS = (PRESENT, ABSENT, BLACK, UNDER)


def L():
  return _lib.lib()


def _dev():
  return torch.device("cuda", 0)


def _st():
  return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _ok(rc):
  assert rc == 0, (rc, L().kv_last_error().decode())


def _t(a):
  """a numpy array on the device (one element at least, so that an empty input still has an address)"""
  a = np.ascontiguousarray(a)
  if a.size == 0:
    return torch.zeros((1,) + a.shape[1:], dtype=torch.from_numpy(a).dtype, device=_dev())[:0]
  return torch.from_numpy(a).to(_dev())


def _p(t):
  if t is None:
    return None
  if isinstance(t, Guarded):
    return ctypes.c_void_p(t.ptr())
  return ctypes.c_void_p(t.data_ptr() if t.numel() else t.untyped_storage().data_ptr())


def _ptrs(ts):
  return (ctypes.c_void_p * len(ts))(*[None if t is None else _p(t).value for t in ts])


def _i64s(vals):
  return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _sync():
  torch.cuda.synchronize()


def _out(n, D, name="out"):
  return Guarded((n, D), torch.float32, _dev(), name)


def _parts(pop):
  """an int32 table cannot be imported into: it holds no blacklisted keys"""
  return ALL_PARTS if pop.key_dtype != "int32" else (PRESENT, ABSENT, UNDER)


# ---- tables ----------------------------------------------------------------------------------------------------------------
class Table:
  def __init__(self, D, key_dtype="int64", enter=0, init=None):
    self.D, self.key_dtype, self.h = D, key_dtype, ctypes.c_void_p()
    _ok(L().kv_create(KEY_DT[key_dtype], _lib.KV_DT_FLOAT, D, enter, 0, 0, ctypes.byref(self.h)))
    _ok(L().kv_set_clock_days(self.h, X.DAY))
    _ok(L().kv_set_seed(self.h, 1))
    self.init = _t(X.init_table(D) if init is None else X.init_table(D, init))
    _ok(L().kv_init_table(self.h, _p(self.init), 4, _st()))

  def close(self):
    if self.h:
      _sync()
      L().kv_destroy(self.h)
      self.h = None

  # the plain calls the tests build state with (inputs the library is not being tested on here)
  def insert(self, ids, rows):
    ids, rows = _t(ids), _t(rows)
    _ok(L().kv_insert(self.h, _p(ids), _p(rows), ids.numel(), _st()))
    _sync()

  def lookup(self, ids):
    ids = _t(ids)
    out = torch.empty((ids.numel(), self.D), device=_dev())
    _ok(L().kv_gather_or_insert(self.h, _p(ids), None, ids.numel(), _p(out), _st()))
    _sync()

  def read(self, ids, name="rows read back"):
    """kv_gather_or_zeros into a guarded buffer -> numpy"""
    ids = _t(ids)
    g = _out(ids.numel(), self.D, name)
    with frozen(ids=ids):
      _ok(L().kv_gather_or_zeros(self.h, _p(ids), ids.numel(), _p(g), _st()))
    g.check(ids.numel())
    return g.t.cpu().numpy()


def prepared(D, key_dtype="int64", enter=X.ENTER):
  """(table, population): blacklisted keys imported on the blacklist, present keys inserted and looked up once, the keys
  under the threshold inserted by one training lookup (tests/test_buffer_extents_cases.py runs this on the oracle)"""
  pop = X.Population(key_dtype)
  t = Table(D, key_dtype, enter)
  b, p, u = (pop.parts[i] for i in (BLACK, PRESENT, UNDER))
  if key_dtype != "int32":
    kb, vb = _t(b), _t(X.key_rows(b, D))
    _ok(L().kv_import(t.h, _p(kb), _p(vb), b.size, _p(kb), b.size, None, None, 0, _st()))
  t.insert(pop.ids(p), X.key_rows(p, D))
  t.lookup(pop.ids(p))
  t.lookup(pop.ids(u))
  return t, pop


@pytest.fixture(scope="module")
def shared():
  """read-only prepared tables, one per (D, key dtype)"""
  cache = {}
  def get(D, key_dtype="int64"):
    if (D, key_dtype) not in cache:
      cache[(D, key_dtype)] = prepared(D, key_dtype)
    return cache[(D, key_dtype)]
  yield get
  for t, _ in cache.values():
    t.close()


@pytest.fixture
def fresh():
  """tables a test changes: closed when it ends"""
  made = []
  def make(D, key_dtype="int64", enter=X.ENTER, bare=False, init=None):
    if bare:
      made.append(Table(D, key_dtype, enter, init))
      return made[-1]
    t, pop = prepared(D, key_dtype, enter)
    made.append(t)
    return t, pop
  yield make
  for t in made:
    t.close()


def _rng(*seed):
  return np.random.default_rng([X.SEED] + [int(s) for s in seed])


# ---- the read-only lookups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_gather_or_zeros(shared, D):
  t, pop = shared(D)
  rng = _rng(1, D)
  for n in NS + (0,):
    ids = _t(pop.draw(n, rng))
    out = _out(n, D)
    with frozen(ids=ids):
      _ok(L().kv_gather_or_zeros(t.h, _p(ids), n, _p(out), _st()))
    out.check(n)
    same_bits(out.t, pop.rows_read(ids.cpu().numpy(), D), "kv_gather_or_zeros n=%d" % n)


@pytest.mark.parametrize("D", [3, 4, 1024])
def test_the_checks_see_a_kernel_that_writes_a_row_too_many_or_too_few(shared, D):
  """the checker on device memory and real stores: the same op told one id more than the buffer has rows, and one id
  fewer (the last row keeps the sentinel).  The extra row is NOT outside allocated memory: a Guarded buffer is followed, in
  the same allocation, by a back guard of at least 8 rows and 8 KiB, and the one row (4 KiB at the most) lands there.  Never
  hand an op a length beyond a buffer that has no such guard behind it."""
  t, pop = shared(D)
  n = 65
  ids = _t(pop.draw(n + 1, _rng(0, D), (PRESENT,)))
  out = _out(n, D)
  _ok(L().kv_gather_or_zeros(t.h, _p(ids), n + 1, _p(out), _st()))
  with pytest.raises(AssertionError, match=r"out: back guard, written at element %d \(row %d\)" % (n * D, n)):
    out.check(n)
  out = _out(n, D)
  _ok(L().kv_gather_or_zeros(t.h, _p(ids), n - 1, _p(out), _st()))
  with pytest.raises(AssertionError, match=r"out: buffer, not written at element %d \(row %d\)" % ((n - 1) * D, n - 1)):
    out.check(n)
  out.check(n - 1, rest_untouched=True)


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_batch_gather_or_zeros(shared, D):
  """tables of different dims and lengths in one launch, one of them without ids"""
  tabs = [shared(D), shared(4), shared(100), shared(D)]
  rng = _rng(2, D)
  for ns in ((TILE + 1, 0, 65, 1), (1, TILE - 1, 0, 65), (0, 0, 0, 0)):
    ids = [_t(pop.draw(n, rng)) for (t, pop), n in zip(tabs, ns)]
    outs = Guarded.many([((n, t.D), torch.float32, "outs[%d]" % i) for i, ((t, _), n) in enumerate(zip(tabs, ns))], _dev())
    f = frozen(*ids)
    _ok(L().kv_batch_gather_or_zeros(len(tabs), _handles([t for t, _ in tabs]), _ptrs(ids), _i64s(ns), _ptrs(outs), _st()))
    f.verify()
    for (t, pop), i, n, o in zip(tabs, ids, ns, outs):
      o.check(n)
      same_bits(o.t, pop.rows_read(i.cpu().numpy(), t.D), o.name)


def _handles(tabs):
  return (ctypes.c_void_p * len(tabs))(*[t.h.value for t in tabs])


@pytest.mark.parametrize("D, key_dtype", KEYED)
def test_counts_days_and_meta(shared, D, key_dtype):
  t, pop = shared(D, key_dtype)
  rng = _rng(3, D)
  for n in NS + (0,):
    ids_np = pop.draw(n, rng, _parts(pop))
    ids, ids64 = _t(ids_np), _t(ids_np.astype(np.int64))
    cnt, days = Guarded(n, torch.int32, _dev(), "counts"), Guarded(n, torch.int32, _dev(), "days")
    fw, fl = Guarded.many([(n, torch.int32, "freq_words"), (n, torch.uint8, "flags")], _dev())
    with frozen(ids=ids, ids64=ids64):
      _ok(L().kv_get_count(t.h, _p(ids), n, _p(cnt), _st()))
      _ok(L().kv_get_timestamp(t.h, _p(ids), n, _p(days), _st()))
      _ok(L().kv_get_meta(t.h, _p(ids64), n, _p(fw), _p(fl), _st()))
    for g in (cnt, days, fw, fl):
      g.check(n)
    same_bits(cnt.t, pop.counts(ids_np), "kv_get_count")
    same_bits(days.t, pop.days(ids_np), "kv_get_timestamp")
    same_bits(fw.t, pop.freq_words(ids_np), "kv_get_meta freq_words")
    same_bits(fl.t.cpu().numpy() & X.FLAG_BITS, pop.flags(ids_np), "kv_get_meta flags")


# ---- the training lookups ----------------------------------------------------------------------------------------------
def _lookup_call(form, t, ids, counts, n, out):
  if form == "plain":
    return L().kv_gather_or_insert(t.h, _p(ids), _p(counts), n, _p(out), _st())
  if form == "tok":
    tok = ctypes.c_uint64(0)
    return L().kv_gather_or_insert_tok(t.h, _p(ids), _p(counts), n, _p(out), ctypes.byref(tok), _st())
  return L().kv_gather_or_insert_pairs(t.h, _p(ids), n, _p(out), _st())


def _training_lookups(fresh, D, key_dtype, forms):
  for k, (form, with_counts) in enumerate(forms):
    t, pop = fresh(D, key_dtype)
    rng = _rng(4, D, k)
    for n in NS + (0,):
      ids_np = pop.draw(n, rng, _parts(pop))
      cnt_np = rng.integers(1, 4, n).astype(np.int32)
      if form == "pairs":
        ids = _t(np.stack([ids_np, cnt_np.astype(np.int64)], axis=1))
        counts = None
      else:
        ids, counts = _t(ids_np), _t(cnt_np) if with_counts else None
      out = _out(n, D)
      with frozen(ids=ids, counts=counts):
        _ok(_lookup_call(form, t, ids, counts, n, out))
      out.check(n)
      same_bits(out.t, pop.rows_lookup(ids_np, D), "%s lookup n=%d" % (form, n))


LOOKUP_FORMS = (("plain", False), ("plain", True), ("tok", False), ("tok", True), ("pairs", True))


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_gather_or_insert(fresh, D):
  _training_lookups(fresh, D, "int64", LOOKUP_FORMS)


@pytest.mark.parametrize("D, key_dtype", KEYED[2:])
def test_gather_or_insert_key_dtypes(fresh, D, key_dtype):
  _training_lookups(fresh, D, key_dtype, LOOKUP_FORMS[:4] if key_dtype == "int32" else LOOKUP_FORMS)


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_gather_or_insert_two_tiles_of_repeated_ids(fresh, D):
  """the batch of _row_geometry: 2 172 ids over two tiles, keys with 1 to 500 occurrences; every other key is held"""
  for k, form in enumerate(("plain", "tok")):
    t = fresh(D, enter=0, bare=True)
    b = X.draw_batch(_rng(5, k))
    held = b["keys"][::2]
    t.insert(held, X.key_rows(held, D))
    want = X.key_rows(b["ids"], D)
    want[~np.isin(b["ids"], held)] = X.init_row(D)
    ids = _t(b["ids"])
    out = _out(ids.numel(), D)
    with frozen(ids=ids):
      _ok(_lookup_call(form, t, ids, None, ids.numel(), out))
    out.check(ids.numel())
    same_bits(out.t, want, form)


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_multi_gather_or_insert(fresh, D):
  """three tables of one dim, different lengths, one without ids; with and without counts and tokens"""
  for k, (tok, with_counts) in enumerate(((False, False), (True, True))):
    tabs = [fresh(D) for _ in range(3)]
    rng = _rng(6, D, k)
    for ns in ((65, 0, TILE + 1), (TILE - 1, 1, 0), (0, 0, 0)):
      ids_np = [pop.draw(n, rng) for (_, pop), n in zip(tabs, ns)]
      ids = [_t(i) for i in ids_np]
      cnts = [_t(rng.integers(1, 4, n).astype(np.int32)) for n in ns] if with_counts else None
      outs = Guarded.many([((n, D), torch.float32, "outs[%d]" % i) for i, n in enumerate(ns)], _dev())
      f = frozen(*(ids + (cnts or [])))
      h = _handles([t for t, _ in tabs])
      if tok:
        toks = (ctypes.c_uint64 * 3)()
        _ok(L().kv_multi_gather_or_insert_tok(3, h, _ptrs(ids), _ptrs(cnts) if cnts else None, _i64s(ns), _ptrs(outs), toks, _st()))
      else:
        _ok(L().kv_multi_gather_or_insert(3, h, _ptrs(ids), _ptrs(cnts) if cnts else None, _i64s(ns), _ptrs(outs), _st()))
      f.verify()
      for (t, pop), i, n, o in zip(tabs, ids_np, ns, outs):
        o.check(n)
        same_bits(o.t, pop.rows_lookup(i, D), o.name)


# ---- the sparse lookups ------------------------------------------------------------------------------------------------
def _sparse_cases(n, rng, k):
  """(segment ids, num_segments, [(combiner, weights or None, segment dtype)]): the three combiners with and without
  weights, the segment dtype alternating"""
  seg, nseg = X.draw_segments(n, rng)
  w = X.draw_weights(n, rng)
  cases = [(c, wts, (np.int32, np.int64)[(c + j + k) % 2]) for c in (0, 1, 2) for j, wts in enumerate((None, w))]
  return seg, nseg, cases


SEG_DT = {np.int32: I32, np.int64: I64}


def _sparse_forward(call, t, pop, D, rows_of, seed):
  rng = _rng(seed, D)
  for k, n in enumerate(NS + (0,)):
    ids_np = pop.draw(n, rng, _parts(pop))
    seg_np, nseg, cases = _sparse_cases(n, rng, k)
    rows = rows_of(ids_np, D)
    ids = _t(ids_np)
    for combiner, w_np, sdt in cases:
      seg, w = _t(seg_np.astype(sdt)), None if w_np is None else _t(w_np)
      out = _out(nseg, D)
      with frozen(ids=ids, segment_ids=seg, weights=w):
        _ok(call(t, ids, seg, SEG_DT[sdt], w, n, nseg, combiner, out))
      out.check(nseg)          # every segment is written, the empty ones included
      want = X.combine(rows, seg_np, w_np, nseg, combiner)
      if n == 0 and call is _call_lookup_sparse:
        want[:] = 0            # kvhip.h: "n == 0 writes zero rows for every segment whatever `weights` is"
      same_bits(out.t, want, "n=%d combiner=%d weights=%s" % (n, combiner, w_np is not None))
    # no segments: a no-op, whatever n is
    out = _out(0, D)
    seg = _t(seg_np)
    _ok(call(t, ids, seg, I64, None, n, 0, 0, out))
    out.check(0)


def _call_lookup_sparse(t, ids, seg, sdt, w, n, nseg, combiner, out):
  return L().kv_lookup_sparse(t.h, _p(ids), _p(seg), sdt, _p(w), n, nseg, combiner, 1, _p(out), _st())


def _call_lookup_sparse_zeros(t, ids, seg, sdt, w, n, nseg, combiner, out):
  return L().kv_lookup_sparse_zeros(t.h, _p(ids), _p(seg), sdt, _p(w), n, nseg, combiner, _p(out), _st())


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_lookup_sparse(fresh, D):
  t, pop = fresh(D)
  _sparse_forward(_call_lookup_sparse, t, pop, D, pop.rows_lookup, 7)


@pytest.mark.parametrize("D", ROW_DIMS)
def test_lookup_sparse_zeros(shared, D):
  t, pop = shared(D)
  _sparse_forward(_call_lookup_sparse_zeros, t, pop, D, pop.rows_read, 8)


@pytest.mark.parametrize("D, key_dtype", KEYED[2:])
def test_lookup_sparse_key_dtypes(fresh, shared, D, key_dtype):
  t, pop = fresh(D, key_dtype)
  _sparse_forward(_call_lookup_sparse, t, pop, D, pop.rows_lookup, 9)
  t, pop = shared(D, key_dtype)
  _sparse_forward(_call_lookup_sparse_zeros, t, pop, D, pop.rows_read, 10)


def _multi_sparse(tabs, D_of, rows_of, batch_zeros, seed):
  """four tables, two calls per combiner: every n of NS on some table, a table with segments but no ids (zero rows / the
  empty-segment rule) in each call, and in the first a table with ids but no segments (nothing written)"""
  rng = _rng(seed, D_of(0))
  combos = ((0, False, np.int32), (1, True, np.int64), (2, True, np.int32), (1, False, np.int64))
  lengths = (((65, 0, TILE + 1, 1), 3), ((TILE - 1, 1, 0, 65), None))         # (ns, the table without segments)
  for (combiner, weighted, sdt), (ns, bare) in ((c, l) for c in combos for l in lengths):
    ids_np = [pop.draw(n, rng) for (_, pop), n in zip(tabs, ns)]
    segs = [X.draw_segments(n, rng) for n in ns]
    nsegs = [0 if i == bare else (m if n else 5) for i, (n, (_, m)) in enumerate(zip(ns, segs))]
    w_np = [X.draw_weights(n, rng) if weighted and i != 0 else None for i, n in enumerate(ns)]     # weights[i] may be NULL
    ids, seg = [_t(i) for i in ids_np], [_t(s.astype(sdt)) for s, _ in segs]
    w = [None if x is None else _t(x) for x in w_np]
    outs = Guarded.many([((m, D_of(i)), torch.float32, "outs[%d]" % i) for i, m in enumerate(nsegs)], _dev())
    f = frozen(*(ids + seg + [x for x in w if x is not None]))
    h = _handles([t for t, _ in tabs])
    wp = _ptrs(w) if weighted else None
    if batch_zeros:
      _ok(L().kv_batch_lookup_sparse_zeros(4, h, _ptrs(ids), _ptrs(seg), SEG_DT[sdt], wp, _i64s(ns), _i64s(nsegs), combiner,
                                           _ptrs(outs), _st()))
    else:
      _ok(L().kv_multi_lookup_sparse(4, h, _ptrs(ids), _ptrs(seg), SEG_DT[sdt], wp, _i64s(ns), _i64s(nsegs), combiner, None,
                                     _ptrs(outs), _st()))
    f.verify()
    for i, ((t, pop), o) in enumerate(zip(tabs, outs)):
      o.check(nsegs[i])
      if nsegs[i] == 0:
        continue
      want = X.combine(rows_of(pop, ids_np[i], D_of(i)), segs[i][0], w_np[i], nsegs[i], combiner)
      if ns[i] == 0 and not batch_zeros:
        want[:] = 0            # "ns[i] == 0 yields zero rows for table i's segments"
      same_bits(o.t, want, "%s combiner=%d" % (o.name, combiner))


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_multi_lookup_sparse(fresh, D):
  tabs = [fresh(D) for _ in range(4)]
  _multi_sparse(tabs, lambda i: D, lambda pop, ids, d: pop.rows_lookup(ids, d), False, 11)


@pytest.mark.parametrize("D", ROW_DIMS)
def test_batch_lookup_sparse_zeros(shared, D):
  """the tables differ in dim; one is listed twice (it is only read)"""
  dims = (D, 100, D, 4)
  tabs = [shared(d) for d in dims]
  _multi_sparse(tabs, lambda i: dims[i], lambda pop, ids, d: pop.rows_read(ids, d), True, 12)


def _grad_cases(D, seed):
  rng = _rng(seed, D)
  for k, n in enumerate(NS):
    seg_np, nseg, cases = _sparse_cases(n, rng, k)
    yield n, seg_np, nseg, X.int_rows(nseg, D, rng), cases


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_lookup_sparse_grad(shared, D):
  t, _ = shared(D)
  for n, seg_np, nseg, sg_np, cases in _grad_cases(D, 13):
    sg = _t(sg_np)
    for combiner, w_np, sdt in cases:
      seg, w = _t(seg_np.astype(sdt)), None if w_np is None else _t(w_np)
      values = _out(n, D, "values")
      with frozen(seg_grad=sg, segment_ids=seg, weights=w):
        _ok(L().kv_lookup_sparse_grad(t.h, _p(sg), _p(seg), SEG_DT[sdt], _p(w), n, nseg, combiner, _p(values), _st()))
      values.check(n)
      same_bits(values.t, X.expand(sg_np, seg_np, w_np, nseg, combiner), "n=%d combiner=%d weights=%s" % (n, combiner, w_np is not None))
  # n == 0 and num_segments == 0 are no-ops
  values = _out(5, D, "values")
  _ok(L().kv_lookup_sparse_grad(t.h, _p(sg), _p(seg), SEG_DT[sdt], None, 0, nseg, 1, _p(values), _st()))
  _ok(L().kv_lookup_sparse_grad(t.h, _p(sg), _p(seg), SEG_DT[sdt], None, 5, 0, 1, _p(values), _st()))
  values.check(0, rest_untouched=True)


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_multi_lookup_sparse_grad(shared, fresh, D):
  tabs = [shared(D)[0]] + [fresh(D, enter=0, bare=True) for _ in range(2)]
  rng = _rng(14, D)
  combos = ((0, True, np.int64), (1, False, np.int32), (2, True, np.int32))
  for (combiner, weighted, sdt), ns in ((c, l) for c in combos for l in ((TILE + 1, 0, 65), (1, TILE - 1, 0))):
    segs = [X.draw_segments(n, rng) for n in ns]
    nsegs = [m for _, m in segs]
    sg_np = [X.int_rows(m, D, rng) for m in nsegs]
    w_np = [X.draw_weights(n, rng) if weighted else None for n in ns]
    sg, seg = [_t(x) for x in sg_np], [_t(s.astype(sdt)) for s, _ in segs]
    w = [None if x is None else _t(x) for x in w_np]
    values = Guarded.many([((n, D), torch.float32, "values[%d]" % i) for i, n in enumerate(ns)], _dev())
    f = frozen(*(sg + seg + [x for x in w if x is not None]))
    _ok(L().kv_multi_lookup_sparse_grad(3, _handles(tabs), _ptrs(sg), _ptrs(seg), SEG_DT[sdt], _ptrs(w) if weighted else None,
                                        _i64s(ns), _i64s(nsegs), combiner, _ptrs(values), _st()))
    f.verify()
    for i, v in enumerate(values):
      v.check(ns[i])           # ns[i] == 0 writes nothing
      same_bits(v.t, X.expand(sg_np[i], segs[i][0], w_np[i], nsegs[i], combiner), "%s combiner=%d" % (v.name, combiner))


# ---- sums, de-duplication ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ROW_DIMS)
def test_unsorted_segment_sum(shared, D):
  t, _ = shared(D)
  rng = _rng(15, D)
  for n in NS + (0,):
    nseg = max(4, n // 3)
    seg_np = rng.integers(-2, nseg + 2, n).astype(np.int32)
    data_np = X.int_rows(n, D, rng)
    seg, data = _t(seg_np), _t(data_np)
    out = _out(nseg, D)
    with frozen(segment_ids=seg, data=data):
      _ok(L().kv_unsorted_segment_sum(t.h, _p(seg), _p(data), n, nseg, _p(out), _st()))
    out.check(nseg)
    same_bits(out.t, X.segment_sum(data_np, seg_np.astype(np.int64), nseg), "n=%d" % n)
  out = _out(0, D)
  _ok(L().kv_unsorted_segment_sum(t.h, _p(seg), _p(data), n, 0, _p(out), _st()))
  out.check(0)


def _check_unique(ids_np, n, U, uniq, inverse, name):
  """the first U entries of uniq are the distinct ids, each once; inverse names each position's entry"""
  u = uniq.t.cpu().numpy()[:U]
  want = np.unique(ids_np.astype(np.int64))
  assert U == want.size and np.array_equal(np.sort(u), want), name
  inv = inverse.t.cpu().numpy()
  assert inv.min(initial=0) >= 0 and inv.max(initial=0) < max(U, 1), name
  assert np.array_equal(u[inv], ids_np.astype(np.int64)), name
  return u


def _dedup(t, pop, D, on_device, seed):
  rng = _rng(seed, D)
  for n in NS + (0,):
    ids_np = pop.draw(n, rng, _parts(pop))
    g_np = X.int_rows(n, D, rng)
    ids, g = _t(ids_np), _t(g_np)
    uniq, inverse, word = Guarded.many([(n, torch.int64, "uniq_ids"), (n, torch.int32, "inverse"), (1, torch.int64, "num_unique_dev")], _dev())
    summed = _out(n, D, "summed")
    host = ctypes.c_int64(-1)
    with frozen(ids=ids, grad=g):
      if on_device:
        _ok(L().kv_dedup_segment_sum_dev(t.h, _p(ids), _p(g), n, _p(uniq), _p(summed), _p(inverse), _p(word), _st()))
      else:
        _ok(L().kv_dedup_segment_sum(t.h, _p(ids), _p(g), n, _p(uniq), _p(summed), _p(inverse), ctypes.byref(host), _st()))
    word.check(1 if on_device else 0, rest_untouched=True)
    U = int(word.t.item()) if on_device else host.value
    for buf in (uniq, summed):
      buf.check(U)             # beyond U: unspecified, but inside the buffer
    inverse.check(n)
    u = _check_unique(ids_np, n, U, uniq, inverse, "n=%d" % n)
    wu, ws, _ = X.dedup(ids_np, g_np)
    same_bits(summed.t.cpu().numpy()[:U][np.argsort(u)], ws if n else np.zeros((0, D), F), "summed n=%d" % n)


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("D", ROW_DIMS)
def test_dedup_segment_sum(shared, D, on_device):
  t, pop = shared(D)
  _dedup(t, pop, D, on_device, 16)


@pytest.mark.parametrize("D, key_dtype", KEYED[2:])
def test_dedup_segment_sum_key_dtypes(shared, D, key_dtype):
  t, pop = shared(D, key_dtype)
  _dedup(t, pop, D, False, 17)
  _dedup(t, pop, D, True, 18)


@pytest.mark.parametrize("D, key_dtype", KEYED)
def test_unique(shared, D, key_dtype):
  t, pop = shared(D, key_dtype)
  rng = _rng(19, D)
  for k, n in enumerate(NS + (0,)):
    for with_counts, on_device in ((False, False), (True, True)):
      ids_np = pop.draw(n, rng, _parts(pop))
      cnt_np = rng.integers(1, 4, n).astype(np.int32)
      ids, cnt = _t(ids_np), _t(cnt_np) if with_counts else None
      uniq, ucnt, inverse, word = Guarded.many([(n, torch.int64, "uniq"), (n, torch.int32, "uniq_counts"), (n, torch.int32, "inverse"),
                                                (1, torch.int64, "num_unique_dev")], _dev())
      host = ctypes.c_int64(-1)
      with frozen(ids=ids, counts=cnt):
        _ok(L().kv_unique(t.h, _p(ids), _p(cnt), n, _p(uniq), _p(ucnt), _p(inverse), None if on_device else ctypes.byref(host),
                          _p(word) if on_device else None, _st()))
      word.check(1 if on_device else 0, rest_untouched=True)
      U = int(word.t.item()) if on_device else host.value
      uniq.check(U), ucnt.check(U), inverse.check(n)
      u = _check_unique(ids_np, n, U, uniq, inverse, "n=%d" % n)
      per_key = np.bincount(inverse.t.cpu().numpy(), weights=cnt_np if with_counts else None, minlength=U)[:U]
      assert np.array_equal(ucnt.t.cpu().numpy()[:U], per_key.astype(np.int32))


# ---- exports, deletes --------------------------------------------------------------------------------------------------
def _by_key(keys, *cols):
  order = np.argsort(keys)
  return [keys[order]] + [c[order] for c in cols]


@pytest.mark.parametrize("first_n", [2, 4, 6])
@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_export_fill(shared, D, first_n):
  """the prepared table: present keys over the threshold, keys under it, blacklisted keys"""
  t, pop = shared(D)
  p, b, u = (pop.parts[i] for i in (PRESENT, BLACK, UNDER))
  want_keys = np.sort(np.concatenate([p, u]) if first_n <= 3 else p)
  want_black = np.sort(b) if first_n > 3 else np.zeros(0, np.int64)
  want_freq = np.sort(np.concatenate([p, b, u])) if first_n > 4 else np.zeros(0, np.int64)
  counts = (ctypes.c_int64 * 3)()
  _ok(L().kv_export_count(t.h, first_n, counts, _st()))
  assert list(counts) == [want_keys.size, want_black.size, want_freq.size]
  keys, black, fkeys, fvals = Guarded.many([(counts[0], torch.int64, "keys"), (counts[1], torch.int64, "blacklist"),
                                            (counts[2], torch.int64, "freq_keys"), (counts[2], torch.int32, "freq_values")], _dev())
  values = _out(counts[0], D, "values")
  _ok(L().kv_export_fill(t.h, first_n, _p(keys), _p(values), _p(black), _p(fkeys), _p(fvals), _st()))
  _sync()
  for g, m in ((keys, counts[0]), (values, counts[0]), (black, counts[1]), (fkeys, counts[2]), (fvals, counts[2])):
    g.check(m)
  k, v = _by_key(keys.t.cpu().numpy(), values.t.cpu().numpy())
  assert np.array_equal(k, want_keys)
  same_bits(v, pop.rows_read(k, D), "values")
  assert np.array_equal(np.sort(black.t.cpu().numpy()), want_black)
  fk, fv = _by_key(fkeys.t.cpu().numpy(), fvals.t.cpu().numpy())
  assert np.array_equal(fk, want_freq)
  same_bits(fv, pop.freq_words(fk), "freq_values")


@pytest.mark.parametrize("first_n", [2, 4, 6])
@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_export_delta_fill(fresh, D, first_n):
  """with delta tracking on: keys inserted (some of them blacklisted before), five of them deleted again"""
  pop = X.Population("int64")
  t = fresh(D, enter=0, bare=True)
  p, b = pop.parts[PRESENT][:300], pop.parts[BLACK][:40]
  gone, kept = p[:5], p[5:]
  kb = _t(b)
  _ok(L().kv_import_delta(t.h, None, None, 0, _p(kb), b.size, None, None, 0, None, 0, 6, _st()))
  _ok(L().kv_set_delta_tracking(t.h, 1, 0))
  both = np.concatenate([p, b])
  t.insert(both, X.key_rows(both, D))
  kg = _t(gone)
  with frozen(ids=kg):
    _ok(L().kv_delete(t.h, _p(kg), gone.size, None, _st()))
  want = {"keys": np.sort(kept), "black": np.sort(b) if first_n > 3 else np.zeros(0, np.int64),
          "freq": np.sort(np.concatenate([kept, b, gone])) if first_n > 4 else np.zeros(0, np.int64),
          "delete": np.sort(gone if first_n > 3 else np.concatenate([gone, b]))}
  counts = (ctypes.c_int64 * 4)()
  _ok(L().kv_export_delta_count(t.h, first_n, counts, _st()))
  assert list(counts) == [want[k].size for k in ("keys", "black", "freq", "delete")]
  keys, black, fkeys, fvals, dele = Guarded.many([(counts[0], torch.int64, "keys"), (counts[1], torch.int64, "blacklist"),
                                                  (counts[2], torch.int64, "freq_keys"), (counts[2], torch.int32, "freq_values"),
                                                  (counts[3], torch.int64, "delete_keys")], _dev())
  values = _out(counts[0], D, "values")
  _ok(L().kv_export_delta_fill(t.h, first_n, _p(keys), _p(values), _p(black), _p(fkeys), _p(fvals), _p(dele), _st()))
  _sync()
  for g, m in ((keys, counts[0]), (values, counts[0]), (black, counts[1]), (fkeys, counts[2]), (fvals, counts[2]), (dele, counts[3])):
    g.check(m)
  k, v = _by_key(keys.t.cpu().numpy(), values.t.cpu().numpy())
  assert np.array_equal(k, want["keys"])
  same_bits(v, X.key_rows(k, D), "values")
  assert np.array_equal(np.sort(black.t.cpu().numpy()), want["black"])
  assert np.array_equal(np.sort(dele.t.cpu().numpy()), want["delete"])
  fk, fv = _by_key(fkeys.t.cpu().numpy(), fvals.t.cpu().numpy())
  assert np.array_equal(fk, want["freq"])
  same_bits(fv, np.where(np.isin(fk, gone), 0, 1).astype(np.uint32), "freq_values")      # inserted: word 1; deleted: 0


@pytest.mark.parametrize("D", SMALL_DIMS)
def test_delete_with_timestamp(fresh, D):
  pop = X.Population("int64")
  t = fresh(D, enter=0, bare=True)
  old, new, never = pop.parts[PRESENT][:70], pop.parts[ABSENT][:50], pop.parts[UNDER][:30]
  t.insert(never, X.key_rows(never, D))          # day stamp 0: never expires
  _ok(L().kv_set_clock_days(t.h, X.DAY - 10))
  t.lookup(old)
  _ok(L().kv_set_clock_days(t.h, X.DAY))
  t.lookup(new)
  count = ctypes.c_int64(-1)
  _ok(L().kv_delete_with_timestamp(t.h, 5, 1, None, ctypes.byref(count), _st()))
  assert count.value == old.size
  keys = Guarded(count.value, torch.int64, _dev(), "delete_keys")
  _ok(L().kv_delete_with_timestamp(t.h, 5, 0, _p(keys), ctypes.byref(count), _st()))
  _sync()
  keys.check(count.value)
  assert count.value == old.size and np.array_equal(np.sort(keys.t.cpu().numpy()), np.sort(old))
  ids = np.concatenate([old, new, never])
  want = np.concatenate([np.zeros((old.size, D), F), np.tile(X.init_row(D), (new.size, 1)), X.key_rows(never, D)])
  same_bits(t.read(ids), want, "rows after the delete")


# ---- routing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_dtype", ["int64", "int32"])
@pytest.mark.parametrize("rule", [0, 1])
def test_bucket_by_owner(shared, key_dtype, rule):
  t, pop = shared(4, key_dtype)
  rng = _rng(20, rule)
  world = 5
  for k, n in enumerate(NS + (0,)):
    for short, extras in ((False, True), (True, False), (True, True)):
      ids_np = pop.draw(n, rng, _parts(pop))
      m = max(0, n - 3) if short else n
      ic_np = rng.integers(1, 9, n).astype(np.int32)
      ids, ic, n_dev = _t(ids_np), _t(ic_np), _t(np.array([m], np.int64))
      out_ids, perm, counts, pairs, pos = Guarded.many(
          [(n, torch.int64, "out_ids"), (n, torch.int32, "perm"), (world, torch.int64, "counts_dev"),
           ((n, 2), torch.int64, "pairs_out"), (n, torch.int32, "pos_out")], _dev())
      with frozen(ids=ids, id_counts=ic, n_dev=n_dev):
        _ok(L().kv_bucket_by_owner(t.h, _p(ids), n, _p(n_dev) if short else None, world, rule, _p(out_ids), _p(perm), _p(counts),
                                   _p(ic) if extras else None, _p(pairs) if extras else None, _p(pos) if extras else None, _st()))
      out_ids.check(m), perm.check(m), counts.check(world)
      pairs.check(m if extras else 0, rest_untouched=not extras)
      pos.check(m if extras else 0, rest_untouched=not extras)
      got, pm = out_ids.t.cpu().numpy()[:m], perm.t.cpu().numpy()[:m]
      own = X.owners(ids_np[:m], world, rule)
      assert np.array_equal(np.sort(pm), np.arange(m)), "perm is a permutation of the input positions"
      assert np.array_equal(got, ids_np[:m].astype(np.int64)[pm])
      assert (np.diff(own[pm]) >= 0).all(), "grouped by owner, rank 0 first"
      assert np.array_equal(counts.t.cpu().numpy(), np.bincount(own, minlength=world))
      if extras:
        assert np.array_equal(pos.t.cpu().numpy()[:m][pm], np.arange(m))
        assert np.array_equal(pairs.t.cpu().numpy()[:m], np.stack([got, ic_np[:m][pm].astype(np.int64)], axis=1))


@pytest.mark.parametrize("D", ROW_DIMS)
def test_take_rows(D):
  """rows of 4 D bytes: the 16-byte path for the multiples of 4, the 4-byte path for the others (the stated exception of
  the alignment contract: both buffers are 16-byte aligned here all the same)"""
  rng = _rng(21, D)
  for n in NS + (0,):
    nsrc = n + 9
    src_np = X.int_rows(nsrc, D, rng, values=(-4095, -1, 1, 2, 4096))
    src = _t(src_np)
    # gather
    idx_np = rng.integers(0, nsrc, n).astype(np.int32)
    idx = _t(idx_np)
    out = _out(n, D)
    with frozen(src=src, index=idx):
      _ok(L().kv_take_rows(0, _p(src), _p(idx), None, n, 4 * D, 0, _p(out), _st()))
    out.check(n)
    same_bits(out.t, src_np[idx_np], "gather n=%d" % n)
    # two-level gather: out[i] = src[index[index_outer[i]]]
    outer_np = rng.integers(0, max(n, 1), n).astype(np.int32)
    outer = _t(outer_np)
    out = _out(n, D)
    with frozen(src=src, index=idx, index_outer=outer):
      _ok(L().kv_take_rows(0, _p(src), _p(idx), _p(outer), n, 4 * D, 0, _p(out), _st()))
    out.check(n)
    same_bits(out.t, src_np[idx_np[outer_np]] if n else src_np[:0], "two-level gather n=%d" % n)
    # scatter into a longer buffer: the rows no index names keep the sentinel
    to_np = rng.permutation(nsrc)[:n].astype(np.int32)
    to = _t(to_np)
    out = _out(nsrc, D)
    with frozen(src=src, index=to):
      _ok(L().kv_take_rows(0, _p(src), _p(to), None, n, 4 * D, 1, _p(out), _st()))
    named = np.zeros(nsrc, bool)
    named[to_np] = True
    out.check(named, rest_untouched=True)
    same_bits(out.t.cpu().numpy()[to_np], src_np[:n], "scatter n=%d" % n)


# ---- the ops without a caller output: inputs intact, the table holds the closed form -----------------------------------
@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_insert_and_assign(fresh, D):
  t, pop = fresh(D)
  rng = _rng(22, D)
  for n in NS + (0,):
    for op in ("insert", "assign"):
      parts = (PRESENT, ABSENT, UNDER) if op == "insert" else ALL_PARTS
      ids_np = pop.draw(n, rng, parts, unique=True)
      rows_np = X.int_rows(n, D, rng, values=(-4095, -2, 3, 4096))
      ids, rows = _t(ids_np), _t(rows_np)
      with frozen(ids=ids, values=rows):
        if op == "insert":
          _ok(L().kv_insert(t.h, _p(ids), _p(rows), n, _st()))
        else:
          _ok(L().kv_scatter_update(t.h, _p(ids), _p(rows), n, _lib_op("ASSIGN"), _st()))
      want = rows_np.copy()
      want[pop.part_of(ids_np) == BLACK] = 0       # blacklisted rows are left untouched
      same_bits(t.read(ids_np), want, "%s n=%d" % (op, n))


def _lib_op(name):
  return {"ASSIGN": 0, "ADD": 1, "SUB": 2, "MUL": 3, "DIV": 4, "MIN": 5, "MAX": 6}[name]


@pytest.mark.parametrize("D", ROW_DIMS)
def test_scatter_add_on_repeated_ids(fresh, D):
  """a folding operation: the update rows of a repeated id are summed, then applied once"""
  t, pop = fresh(D)
  rng = _rng(23, D)
  rows_now = {}
  for n in NS + (0,):
    ids_np = pop.draw(n, rng, (PRESENT, ABSENT, UNDER))
    upd_np = X.int_rows(n, D, rng)
    ids, upd = _t(ids_np), _t(upd_np)
    before = t.read(ids_np, "rows before") if n else np.zeros((0, D), F)
    absent = pop.part_of(ids_np) == ABSENT
    seen = np.array([int(k) in rows_now for k in ids_np], bool)
    before[absent & ~seen] = X.init_row(D)         # a missing key is inserted with the init rule first
    with frozen(ids=ids, updates=upd):
      _ok(L().kv_scatter_update(t.h, _p(ids), _p(upd), n, _lib_op("ADD"), _st()))
    u, s, _ = X.dedup(ids_np, upd_np)
    first = np.array([np.flatnonzero(ids_np.astype(np.int64) == k)[0] for k in u], np.int64)
    want = before[first] + s if n else before
    same_bits(t.read(pop.ids(u)), want.astype(F), "n=%d" % n)
    rows_now.update((int(k), None) for k in u)


@pytest.mark.parametrize("D", ROW_DIMS + WIDE_DIMS)
def test_import_and_import_delta(fresh, D):
  pop = X.Population("int64")
  t = fresh(D, enter=0, bare=True)
  rng = _rng(24, D)
  univ = rng.permutation(pop.parts.reshape(-1))      # 2 816 keys: [0, n) imported, the rest by role
  b, never, nb_np = univ[2100:2200], univ[2200:2207], univ[2210:2213]
  for n in NS + (0,):
    keys_np = univ[:n]
    rows_np = X.int_rows(n, D, rng, values=(-4095, 5, 4096))
    fk_np = keys_np[:n // 3 + 1]
    fv_np = (np.uint32(X.DAY << 16) | rng.integers(1, 100, fk_np.size).astype(np.uint32)).view(np.int32)
    keys, rows, black, fk, fv = _t(keys_np), _t(rows_np), _t(b), _t(fk_np), _t(fv_np)
    with frozen(keys=keys, values=rows, blacklist=black, freq_keys=fk, freq_values=fv):
      _ok(L().kv_import(t.h, _p(keys), _p(rows), n, _p(black), b.size, _p(fk), _p(fv), fk_np.size, _st()))
    probe = np.concatenate([keys_np, b, never])
    want = np.concatenate([rows_np, np.zeros((b.size + never.size, D), F)])
    same_bits(t.read(probe), want, "import n=%d" % n)
    cnt = Guarded(fk_np.size, torch.int32, _dev(), "counts")
    _ok(L().kv_get_count(t.h, _p(fk), fk_np.size, _p(cnt), _st()))
    cnt.check(fk_np.size)
    same_bits(cnt.t, (fv_np.view(np.uint32) & 0xFFFF).astype(np.int32), "imported frequencies")
    # the delta on top: some keys overwritten, some new, two of the blacklisted keys lifted by a row, some keys deleted
    over, new, lifted = keys_np[:n // 2 + 1], univ[2300:2300 + n // 4 + 1], b[:2]
    dk_np = keys_np[n // 2 + 1:][:5]
    dkeys_np = np.concatenate([over, new, lifted])
    drows_np = X.int_rows(dkeys_np.size, D, rng, values=(-7, 9))
    # (nb_np: blacklisted by the delta — absent keys enter as blacklisted)
    dkeys, drows, nb, dk = _t(dkeys_np), _t(drows_np), _t(nb_np), _t(dk_np)
    with frozen(keys=dkeys, values=drows, blacklist=nb, delete_keys=dk):
      _ok(L().kv_import_delta(t.h, _p(dkeys), _p(drows), dkeys_np.size, _p(nb), nb_np.size, None, None, 0, _p(dk), dk_np.size, 6, _st()))
    rest = np.setdiff1d(keys_np, np.concatenate([over, dk_np]))
    probe = np.concatenate([dkeys_np, nb_np, dk_np, b[2:], rest])
    at = np.argsort(keys_np)
    want = np.concatenate([drows_np, np.zeros((nb_np.size + dk_np.size + b.size - 2, D), F),
                           rows_np[at[np.searchsorted(keys_np, rest, sorter=at)]]])
    same_bits(t.read(probe), want, "import_delta n=%d" % n)


@pytest.mark.parametrize("D, key_dtype", KEYED)
def test_delete(fresh, D, key_dtype):
  t, pop = fresh(D, key_dtype)
  rng = _rng(25, D)
  left = {int(k) for k in pop.parts[PRESENT]}
  for n in NS + (0,):
    ids_np = pop.draw(n, rng, (PRESENT, ABSENT))
    ids = _t(ids_np)
    gone = ctypes.c_int64(-1)
    with frozen(ids=ids):
      _ok(L().kv_delete(t.h, _p(ids), n, ctypes.byref(gone), _st()))
    hit = {int(k) for k in ids_np} & left
    assert gone.value == len(hit)
    left -= hit
    probe = pop.ids(pop.parts[PRESENT])
    want = X.key_rows(probe, D)
    want[[int(k) not in left for k in probe]] = 0
    same_bits(t.read(probe), want, "n=%d" % n)


# ---- the optimizer applies ---------------------------------------------------------------------------------------------
def _adagrad(fresh, D, form, seed, key_dtype="int64"):
  """lookup, then one Adagrad step in `form`, on a table with enter_threshold 2: keys the lookup has just inserted stay
  under the threshold (skipped: no accumulator row), keys it counted twice do not; a blacklisted key's row is lifted to
  zeros first.  Integer gradients: the step is exact (tests/_extent_cases.py)."""
  unique = form in ("unique", "counted")
  rng = _rng(seed, D)
  for n in NS + (0,):
    var, pop = fresh(D, key_dtype)
    acc = fresh(D, key_dtype, enter=0, bare=True, init=X.ACC0)
    ids_np, grad = X.apply_batch(pop, n, rng, _parts(pop), unique)
    g_np = grad(D)
    ids, g = _t(ids_np), _t(g_np)
    out = _out(n, D)
    tok = ctypes.c_uint64(0)
    f = frozen(ids=ids, grad=g)
    _ok(L().kv_gather_or_insert_tok(var.h, _p(ids), None, n, _p(out), ctypes.byref(tok), _st()))
    lr = ctypes.c_float(X.LR)
    if form == "plain":
      _ok(L().kv_apply_adagrad(var.h, acc.h, lr, _p(g), _p(ids), n, 1, _st()))
    elif form == "tok":
      _ok(L().kv_apply_adagrad_tok(var.h, acc.h, lr, _p(g), _p(ids), n, 1, tok, _st()))
    elif form == "unique":
      _ok(L().kv_apply_adagrad_unique(var.h, acc.h, lr, _p(g), _p(ids), n, 1, _st()))
    else:
      n_dev = _t(np.array([n], np.int64))
      hp = (ctypes.c_float * 2)(X.LR, 1.0)
      with frozen(n_dev=n_dev):
        _ok(L().kv_apply_unique_counted(var.h, 2, acc.h, None, hp, _p(g), _p(ids), KEY_DT[key_dtype] if key_dtype == "int32" else I64,
                                        n, _p(n_dev), _st()))
    f.verify()
    out.check(n)
    same_bits(out.t, pop.rows_lookup(ids_np, D), "%s: the lookup, n=%d" % (form, n))
    if n:
      _check_step(var, acc, pop, ids_np, g_np, D, "%s n=%d" % (form, n))


def _check_step(var, acc, pop, ids_np, g_np, D, name):
  u, s, cnt = X.dedup(ids_np, g_np)
  part = pop.part_of(u)
  x0 = pop.rows_lookup(u, D)
  x0[part == BLACK] = 0
  want_x, want_a = X.adagrad_step(x0, s, (part == ABSENT) & (cnt == 1))
  same_bits(var.read(pop.ids(u)), want_x, name + ": var")
  same_bits(acc.read(pop.ids(u)), want_a, name + ": accumulator")


@pytest.mark.parametrize("D", ROW_DIMS)
def test_apply_adagrad(fresh, D):
  _adagrad(fresh, D, "plain", 26)


@pytest.mark.parametrize("D", ROW_DIMS)
def test_apply_adagrad_tok(fresh, D):
  _adagrad(fresh, D, "tok", 27)


@pytest.mark.parametrize("D", ROW_DIMS)
def test_apply_adagrad_unique(fresh, D):
  _adagrad(fresh, D, "unique", 28)


@pytest.mark.parametrize("D", COUNTED_DIMS)
def test_apply_unique_counted(fresh, D):
  _adagrad(fresh, D, "counted", 29)


@pytest.mark.parametrize("D, key_dtype", KEYED[2:])
def test_apply_adagrad_key_dtypes(fresh, D, key_dtype):
  _adagrad(fresh, D, "tok", 30, key_dtype)
  _adagrad(fresh, D, "unique", 31, key_dtype)


@pytest.mark.parametrize("D", F4_DIMS)
def test_multi_apply_adagrad(fresh, D):
  """three (var, accumulator) pairs of one dim in one call, one of them without ids"""
  rng = _rng(32, D)
  for ns in ((65, 0, TILE + 1), (TILE - 1, 1, 0)):
    pairs = [(fresh(D), fresh(D, enter=0, bare=True, init=X.ACC0)) for _ in ns]
    batches = [X.apply_batch(pop, n, rng, ALL_PARTS, False) for ((_, pop), _), n in zip(pairs, ns)]
    ids_np = [b[0] for b in batches]
    g_np = [b[1](D) for b in batches]
    ids, g = [_t(i) for i in ids_np], [_t(x) for x in g_np]
    outs = Guarded.many([((n, D), torch.float32, "outs[%d]" % i) for i, n in enumerate(ns)], _dev())
    toks = (ctypes.c_uint64 * 3)()
    f = frozen(*(ids + g))
    hv, ha = _handles([v for (v, _), _ in pairs]), _handles([a for _, a in pairs])
    _ok(L().kv_multi_gather_or_insert_tok(3, hv, _ptrs(ids), None, _i64s(ns), _ptrs(outs), toks, _st()))
    _ok(L().kv_multi_apply_adagrad_tok(3, hv, ha, ctypes.c_float(X.LR), _ptrs(g), _ptrs(ids), _i64s(ns), 1, toks, _st()))
    f.verify()
    for i, (((var, pop), acc), n) in enumerate(zip(pairs, ns)):
      outs[i].check(n)
      same_bits(outs[i].t, pop.rows_lookup(ids_np[i], D), "outs[%d]" % i)
      if n:
        _check_step(var, acc, pop, ids_np[i], g_np[i], D, "table %d" % i)


# ---- the binding keeps the alignment contract --------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 100])
def test_binding_aligns_a_view_at_an_odd_offset(D):
  """a gradient that is flat[1 : 1 + n D].view(n, D) — 4 bytes off a 16-byte boundary — gives the bits of an aligned copy"""
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
  pop = X.Population("int64")
  rng = _rng(33, D)
  n = TILE + 1
  ids_np, grad = X.apply_batch(pop, n, rng, (PRESENT, ABSENT, UNDER), False)       # (these tables hold the present keys only)
  g_np = grad(D)
  flat = torch.zeros(n * D + 8, device=_dev())
  flat[1:1 + n * D] = _t(g_np).reshape(-1)
  view = flat[1:1 + n * D].view(n, D)
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  aligned = view.clone()
  assert aligned.data_ptr() % 16 == 0
  ids = _t(ids_np)
  state = []
  for gradient in (view, aligned):
    hv = ops.kv_variable([D], device=0)
    ha = ops.kv_variable([D], device=0)
    for h, table in ((hv, X.init_table(D)), (ha, X.init_table(D, X.ACC0))):
      ops.kv_set_clock_days(h, X.DAY)
      ops.kv_set_seed(h, 1)
      ops.init_kv_variable_v2(h, table)
    p = pop.parts[PRESENT]
    ops.kv_variable_insert_v2(hv, p, X.key_rows(p, D))
    rows = ops.kv_variable_gather_or_insert_v2(hv, ids)
    with frozen(grad=flat):
      ops.kv_variable_sparse_apply_adagrad(hv, ha, X.LR, gradient, ids)
    u = np.unique(ids_np)
    state.append((rows.cpu().numpy(), ops.kv_variable_gather_or_zeros_v2(hv, u).cpu().numpy(),
                  ops.kv_variable_gather_or_zeros_v2(ha, u).cpu().numpy()))
  for a, b, name in zip(state[0], state[1], ("lookup", "var", "accumulator")):
    same_bits(a, b, name)
  u, s, cnt = X.dedup(ids_np, g_np)
  want_x, want_a = X.adagrad_step(pop.rows_lookup(u, D), s, np.zeros(u.size, bool))
  same_bits(state[0][1], want_x, "var")
  same_bits(state[0][2], want_a, "accumulator")
