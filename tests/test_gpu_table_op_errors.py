"""The argument paths of the table ops (tfplus_amd/csrc/kv_ops.hip) through the raw C ABI: for every entry point, each
bad argument it checks for and each early KV_OK, as the pair (status, kv_last_error() text).  The order of an op's checks
mirrors the reference op by op — where n == 0 returns and where the uninitialised table is refused differs between
them — so the table below is the contract: it was read off the source, case by case, and every case returns before the
op's first kernel launch (no kernel ever sees the null or undersized pointers passed here).

Left out because the library does NOT refuse them before launching: kv_batch_gather_or_zeros with a table listed twice or
with mixed dims (a legitimate gather per table), kv_scatter_update with a folding operation on more than one id of an
uninitialised table (the de-duplication runs first), an uninitialised table in the ops that only borrow a table's
workspace (kv_dedup_segment_sum, kv_unsorted_segment_sum, kv_unique).

The second test holds the id-type fork of the kernels that take the table's ids as int32 or int64: the same sequence of
ops on an int32-key and an int64-key table gives equal outputs, element for element.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tfplus_amd import _lib  # noqa: E402

OK, INVALID, PRECOND, UNIMPL = _lib.KV_OK, _lib.KV_INVALID_ARGUMENT, _lib.KV_FAILED_PRECONDITION, _lib.KV_UNIMPLEMENTED
NULLH = "null table handle"
UNINIT = "Failed to use uninitialized variables: KvVariable init table not set"
NULL_IO = "indices / output pointer is null"
NULL_ARRAY = "null argument array"
BAD = "bad arguments"
COMBINER = "combiner must be one of 'mean', 'sqrtn' or 'sum'"
SPARSE_NULL = "ids / segment ids / output pointer is null"
TAKE = "kv_take_rows: n %d, row_bytes %d (a positive multiple of 4)"
RECOUNT = "the buffers sized from the counts may be too small; count again"
# what kv_last_error() holds before every case (kv_create without an out pointer): a case that returns KV_OK leaves it
SENTINEL = "out is null"
N = 8                      # ids per call
OVER = (1 << 23) + 1       # one id more than an entry-list index pass takes (dim 8)
I32, I64 = _lib.KV_DT_INT32, _lib.KV_DT_INT64


def _arr(ctype, *vals):
  return (ctype * len(vals))(*vals)


def _ptrs(*vals):
  return _arr(ctypes.c_void_p, *vals)


def _cnt():
  """an int64 the library writes through (num_unique, num_deleted, count)"""
  return ctypes.byref(ctypes.c_int64(-1))


# ---- the cases that need no table: (id, function, arguments(P), status, message); P is some non-null pointer -------------
def _no_table_cases():
  c = []
  def add(cid, fn, args, rc=INVALID, msg=NULLH):
    c.append(pytest.param(fn, args, rc, msg, id=cid))
  for fn in ("kv_size", "kv_sum_freq", "kv_map_size"):
    add(fn + "-null", fn, lambda P: (None, _cnt(), None))
  add("kv_get_meta-null", "kv_get_meta", lambda P: (None, P, N, P, P, None))
  add("kv_gather_or_insert-null", "kv_gather_or_insert", lambda P: (None, P, None, N, P, None))
  add("kv_gather_or_insert_tok-null", "kv_gather_or_insert_tok",
      lambda P: (None, P, None, N, P, ctypes.byref(ctypes.c_uint64()), None))
  add("kv_gather_or_insert_pairs-null", "kv_gather_or_insert_pairs", lambda P: (None, P, N, P, None))
  add("kv_lookup_sparse-null", "kv_lookup_sparse", lambda P: (None, P, P, I32, None, N, 4, 0, 1, P, None))
  add("kv_gather_or_zeros-null", "kv_gather_or_zeros", lambda P: (None, P, N, P, None))
  add("kv_dedup_segment_sum-null", "kv_dedup_segment_sum", lambda P: (None, P, P, N, P, P, None, _cnt(), None))
  add("kv_unsorted_segment_sum-null", "kv_unsorted_segment_sum", lambda P: (None, P, P, N, 4, P, None))
  add("kv_unique-null", "kv_unique", lambda P: (None, P, None, N, P, None, None, _cnt(), None, None))
  add("kv_delete-null", "kv_delete", lambda P: (None, P, N, _cnt(), None))
  add("kv_delete_with_timestamp-null", "kv_delete_with_timestamp", lambda P: (None, 7, 1, None, _cnt(), None))
  add("kv_get_count-null", "kv_get_count", lambda P: (None, P, N, P, None))
  add("kv_get_timestamp-null", "kv_get_timestamp", lambda P: (None, P, N, P, None))
  add("kv_export_count-null", "kv_export_count", lambda P: (None, 2, _arr(ctypes.c_int64, 0, 0, 0), None))
  add("kv_export_fill-null", "kv_export_fill", lambda P: (None, 2, P, P, None, None, None, None))
  add("kv_set_delta_tracking-null", "kv_set_delta_tracking", lambda P: (None, 1, 0))
  add("kv_export_delta_count-null", "kv_export_delta_count", lambda P: (None, 6, _arr(ctypes.c_int64, 0, 0, 0, 0), None))
  add("kv_export_delta_fill-null", "kv_export_delta_fill", lambda P: (None, 6, P, P, P, P, P, P, None))
  add("kv_insert-null", "kv_insert", lambda P: (None, P, P, N, None))
  add("kv_scatter_update-null", "kv_scatter_update", lambda P: (None, P, P, N, 1, None))
  add("kv_import-null", "kv_import", lambda P: (None, P, P, N, None, 0, None, None, 0, None))
  add("kv_import_delta-null", "kv_import_delta", lambda P: (None, P, P, N, None, 0, None, None, 0, None, 0, 6, None))
  # the batched forms: the table array itself, its length, a null handle inside it
  for fn, tail in (("kv_batch_gather_or_zeros", lambda P: (_ptrs(P), _arr(ctypes.c_int64, N), _ptrs(P), None)),
                   ("kv_multi_gather_or_insert", lambda P: (_ptrs(P), None, _arr(ctypes.c_int64, N), _ptrs(P), None)),
                   ("kv_multi_gather_or_insert_tok",
                    lambda P: (_ptrs(P), None, _arr(ctypes.c_int64, N), _ptrs(P), None, None))):
    add(fn + "-no-tables", fn, lambda P, tail=tail: (0, _ptrs(None)) + tail(P), msg="N must be >= 1")
    add(fn + "-null-array", fn, lambda P, tail=tail: (1, None) + tail(P), msg=NULL_ARRAY)
    add(fn + "-null", fn, lambda P, tail=tail: (1, _ptrs(None)) + tail(P))
  # kv_take_rows(device, src, index, index_outer, n, row_bytes, scatter, out, stream)
  take = "kv_take_rows"
  add(take + "-two-level-scatter", take, lambda P: (0, P, P, P, N, 32, 1, P, None),
      msg="kv_take_rows: the two-level index is gather only")
  add(take + "-n<0", take, lambda P: (0, P, P, None, -1, 32, 0, P, None), msg=TAKE % (-1, 32))
  add(take + "-row_bytes-6", take, lambda P: (0, P, P, None, N, 6, 0, P, None), msg=TAKE % (N, 6))
  add(take + "-row_bytes-0", take, lambda P: (0, P, P, None, N, 0, 0, P, None), msg=TAKE % (N, 0))
  add(take + "-null-src", take, lambda P: (0, None, P, None, N, 32, 0, P, None), msg=TAKE % (N, 32))
  add(take + "-null-index", take, lambda P: (0, P, None, None, N, 32, 0, P, None), msg=TAKE % (N, 32))
  add(take + "-null-out", take, lambda P: (0, P, P, None, N, 32, 0, None, None), msg=TAKE % (N, 32))
  add(take + "-n=0", take, lambda P: (0, None, None, None, 0, 32, 0, None, None), rc=OK, msg=SENTINEL)
  return c


def _call(fn, args, rc, msg):
  L = _lib.lib()
  assert L.kv_create(0, 0, 0, 0, 0, 0, None) == INVALID and L.kv_last_error().decode() == SENTINEL
  got = getattr(L, fn)(*args)
  assert (got, L.kv_last_error().decode()) == (rc, msg)


@pytest.mark.parametrize("fn, args, rc, msg", _no_table_cases())
def test_refused_without_a_table(fn, args, rc, msg):
  host = ctypes.create_string_buffer(1024)   # never read: every case returns on its arguments alone
  _call(fn, args(ctypes.addressof(host)), rc, msg)


# ---- the cases on tables ----------------------------------------------------------------------------------------------
class _Tables:
  """T: dim 8, a 16-row init table; U: dim 8, never initialised; T32: int32 keys; T16: dim 16 — P: 1 KB of device memory"""
  def __init__(self):
    L = _lib.lib()
    self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    self.buf = torch.zeros(256, dtype=torch.float32, device="cuda")
    self.P = self.buf.data_ptr()
    self.handles = []
    init = torch.ones((16, 16), dtype=torch.float32, device="cuda")
    def make(key_dtype, dim, initialise):
      h = ctypes.c_void_p()
      _lib.check(L.kv_create(key_dtype, _lib.KV_DT_FLOAT, dim, 0, 0, 0, ctypes.byref(h)))
      self.handles.append(h)
      if initialise:
        _lib.check(L.kv_init_table(h, init[:, :dim].contiguous().data_ptr(), 16, self.st))
      return h.value
    self.T, self.U = make(I64, 8, True), make(I64, 8, False)
    self.T32, self.T16 = make(I32, 8, True), make(I64, 16, True)
    torch.cuda.synchronize()

  def close(self):
    torch.cuda.synchronize()
    for h in self.handles:
      _lib.lib().kv_destroy(h)


@pytest.fixture(scope="module")
def tables():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  t = _Tables()
  yield t
  t.close()


def _table_cases():
  c = []
  def add(cid, fn, args, rc, msg):
    c.append(pytest.param(fn, args, rc, msg, id=cid))
  def tok():
    return ctypes.byref(ctypes.c_uint64())

  # kv_get_meta(t, ids, n, freq_words, flags, stream): nothing to do for n <= 0, whatever the pointers
  add("kv_get_meta-n=0", "kv_get_meta", lambda c: (c.T, None, 0, None, None, c.st), OK, SENTINEL)
  add("kv_get_meta-n<0", "kv_get_meta", lambda c: (c.T, None, -1, None, None, c.st), OK, SENTINEL)

  # the training lookups (ids, counts, n, out): n == 0 returns before the precondition (kv_variable_ops.cc:530-532)
  for fn, args in (("kv_gather_or_insert", lambda c, t, ids, n, out: (t, ids, None, n, out, c.st)),
                   ("kv_gather_or_insert_tok", lambda c, t, ids, n, out: (t, ids, None, n, out, tok(), c.st)),
                   ("kv_gather_or_insert_pairs", lambda c, t, ids, n, out: (t, ids, n, out, c.st))):
    add(fn + "-uninit-n=0", fn, lambda c, a=args: a(c, c.U, c.P, 0, c.P), OK, SENTINEL)
    add(fn + "-n<0", fn, lambda c, a=args: a(c, c.T, c.P, -1, c.P), INVALID, "indices: bad length -1")
    add(fn + "-n-over", fn, lambda c, a=args: a(c, c.T, c.P, (1 << 30) + 1, c.P), INVALID, "indices: bad length 1073741825")
    add(fn + "-null-ids", fn, lambda c, a=args: a(c, c.T, None, N, c.P), INVALID, NULL_IO)
    add(fn + "-null-out", fn, lambda c, a=args: a(c, c.T, c.P, N, None), INVALID, NULL_IO)
    add(fn + "-uninit", fn, lambda c, a=args: a(c, c.U, c.P, N, c.P), PRECOND, UNINIT)
  add("kv_gather_or_insert_pairs-int32-table", "kv_gather_or_insert_pairs", lambda c: (c.T32, c.P, N, c.P, c.st),
      INVALID, "id/count pairs carry int64 ids")

  # kv_lookup_sparse(t, ids, segment_ids, segment_dtype, weights, n, num_segments, combiner, count_occurrences, out, stream)
  sp = "kv_lookup_sparse"
  def sparse(c, t=None, ids=0, seg=0, sdt=I32, n=N, nseg=4, comb=0, out=0):
    pick = lambda p: c.P if p == 0 else p
    return (t or c.T, pick(ids), pick(seg), sdt, None, n, nseg, comb, 1, pick(out), c.st)
  add(sp + "-combiner<0", sp, lambda c: sparse(c, comb=-1), INVALID, COMBINER)
  add(sp + "-combiner-3", sp, lambda c: sparse(c, comb=3), INVALID, COMBINER)
  add(sp + "-combiner-before-uninit", sp, lambda c: sparse(c, t=c.U, comb=3), INVALID, COMBINER)
  add(sp + "-segment_dtype", sp, lambda c: sparse(c, sdt=_lib.KV_DT_FLOAT), INVALID, "segment ids must be int32 or int64")
  add(sp + "-n<0", sp, lambda c: sparse(c, n=-1), INVALID, "sp_ids: -1 values (at most 2^23 per call)")
  add(sp + "-n-over", sp, lambda c: sparse(c, n=OVER), INVALID, "sp_ids: 8388609 values (at most 2^23 per call)")
  add(sp + "-num_segments<0", sp, lambda c: sparse(c, nseg=-1), INVALID, "bad num_segments")
  add(sp + "-num_segments-over", sp, lambda c: sparse(c, nseg=(1 << 31) - 1), INVALID, "bad num_segments")
  add(sp + "-num_segments=0", sp, lambda c: sparse(c, nseg=0, out=None), OK, SENTINEL)
  add(sp + "-uninit-num_segments=0", sp, lambda c: sparse(c, t=c.U, nseg=0), OK, SENTINEL)
  add(sp + "-null-out", sp, lambda c: sparse(c, out=None), INVALID, SPARSE_NULL)
  add(sp + "-null-out-n=0", sp, lambda c: sparse(c, n=0, out=None), INVALID, SPARSE_NULL)
  add(sp + "-null-ids", sp, lambda c: sparse(c, ids=None), INVALID, SPARSE_NULL)
  add(sp + "-null-segment-ids", sp, lambda c: sparse(c, seg=None), INVALID, SPARSE_NULL)
  add(sp + "-uninit", sp, lambda c: sparse(c, t=c.U), PRECOND, UNINIT)
  add(sp + "-uninit-n=0", sp, lambda c: sparse(c, t=c.U, n=0), PRECOND, UNINIT)

  # kv_gather_or_zeros(t, ids, n, out, stream): the precondition comes first, n == 0 behind it (kv_variable.h:242)
  goz = "kv_gather_or_zeros"
  add(goz + "-uninit-n=0", goz, lambda c: (c.U, c.P, 0, c.P, c.st), PRECOND, UNINIT)
  add(goz + "-uninit", goz, lambda c: (c.U, c.P, N, c.P, c.st), PRECOND, UNINIT)
  add(goz + "-n=0", goz, lambda c: (c.T, None, 0, None, c.st), OK, SENTINEL)
  add(goz + "-n<0", goz, lambda c: (c.T, c.P, -1, c.P, c.st), INVALID, NULL_IO)
  add(goz + "-null-ids", goz, lambda c: (c.T, None, N, c.P, c.st), INVALID, NULL_IO)
  add(goz + "-null-out", goz, lambda c: (c.T, c.P, N, None, c.st), INVALID, NULL_IO)

  # kv_batch_gather_or_zeros(num_tables, tables, ids, ns, outs, stream)
  bg = "kv_batch_gather_or_zeros"
  def batch(c, tabs, ids=0, ns=0, outs=0):
    k = len(tabs)
    ids = _ptrs(*[c.P] * k) if ids == 0 else ids
    ns = _arr(ctypes.c_int64, *[N] * k) if ns == 0 else ns
    outs = _ptrs(*[c.P] * k) if outs == 0 else outs
    return (k, _ptrs(*tabs), ids, ns, outs, c.st)
  add(bg + "-null-ids-array", bg, lambda c: batch(c, [c.T], ids=None), INVALID, NULL_ARRAY)
  add(bg + "-null-ns-array", bg, lambda c: batch(c, [c.T], ns=None), INVALID, NULL_ARRAY)
  add(bg + "-null-outs-array", bg, lambda c: batch(c, [c.T], outs=None), INVALID, NULL_ARRAY)
  add(bg + "-n<0", bg, lambda c: batch(c, [c.T], ns=_arr(ctypes.c_int64, -1)), INVALID, NULL_IO)
  add(bg + "-null-ids", bg, lambda c: batch(c, [c.T], ids=_ptrs(None)), INVALID, NULL_IO)
  add(bg + "-null-out", bg, lambda c: batch(c, [c.T], outs=_ptrs(None)), INVALID, NULL_IO)
  add(bg + "-uninit", bg, lambda c: batch(c, [c.T, c.U]), PRECOND, UNINIT)
  add(bg + "-uninit-n=0", bg, lambda c: batch(c, [c.U], ns=_arr(ctypes.c_int64, 0)), PRECOND, UNINIT)

  # kv_multi_gather_or_insert[_tok](num_tables, tables, ids, counts, ns, outs, [tokens,] stream)
  for fn, end in (("kv_multi_gather_or_insert", lambda c: (c.st,)), ("kv_multi_gather_or_insert_tok", lambda c: (None, c.st))):
    def multi(c, tabs, ids=0, ns=0, outs=0, end=end):
      k = len(tabs)
      ids = _ptrs(*[c.P] * k) if ids == 0 else ids
      ns = _arr(ctypes.c_int64, *[N] * k) if ns == 0 else ns
      outs = _ptrs(*[c.P] * k) if outs == 0 else outs
      return (k, _ptrs(*tabs), ids, None, ns, outs) + end(c)
    add(fn + "-null-ids-array", fn, lambda c, m=multi: m(c, [c.T], ids=None), INVALID, NULL_ARRAY)
    add(fn + "-null-ns-array", fn, lambda c, m=multi: m(c, [c.T], ns=None), INVALID, NULL_ARRAY)
    add(fn + "-null-outs-array", fn, lambda c, m=multi: m(c, [c.T], outs=None), INVALID, NULL_ARRAY)
    add(fn + "-mixed-dims", fn, lambda c, m=multi: m(c, [c.T, c.T16]), INVALID,
        "batched op: tables must share dim and key dtype (group them by shape)")
    add(fn + "-mixed-key-dtypes", fn, lambda c, m=multi: m(c, [c.T, c.T32]), INVALID,
        "batched op: tables must share dim and key dtype (group them by shape)")
    add(fn + "-n<0", fn, lambda c, m=multi: m(c, [c.T], ns=_arr(ctypes.c_int64, -1)), INVALID, "indices: bad length -1")
    add(fn + "-n-over", fn, lambda c, m=multi: m(c, [c.T], ns=_arr(ctypes.c_int64, OVER)), INVALID, "indices: bad length 8388609")
    add(fn + "-null-ids", fn, lambda c, m=multi: m(c, [c.T], ids=_ptrs(None)), INVALID, "indices pointer is null")
    add(fn + "-uninit", fn, lambda c, m=multi: m(c, [c.T, c.U]), PRECOND, UNINIT)
    add(fn + "-uninit-n=0", fn, lambda c, m=multi: m(c, [c.U], ns=_arr(ctypes.c_int64, 0)), PRECOND, UNINIT)
    add(fn + "-listed-twice", fn, lambda c, m=multi: m(c, [c.T, c.T]), INVALID, "batched op: table listed twice")
    add(fn + "-null-out", fn, lambda c, m=multi: m(c, [c.T], outs=_ptrs(None)), INVALID, "output pointer is null")

  # kv_dedup_segment_sum(t, ids, grad, n, uniq, summed, inverse, num_unique, stream): `t` only lends its workspace
  dd = "kv_dedup_segment_sum"
  def dedup(c, t=None, ids=0, grad=0, n=N, uniq=0, summed=0, nu=0):
    pick = lambda p: c.P if p == 0 else p
    return (t or c.T, pick(ids), pick(grad), n, pick(uniq), pick(summed), None, _cnt() if nu == 0 else nu, c.st)
  add(dd + "-null-num_unique", dd, lambda c: dedup(c, nu=None), INVALID, "num_unique is null")
  add(dd + "-uninit-n=0", dd, lambda c: dedup(c, t=c.U, n=0), OK, SENTINEL)
  add(dd + "-n<0", dd, lambda c: dedup(c, n=-1), INVALID, BAD)
  add(dd + "-null-ids", dd, lambda c: dedup(c, ids=None), INVALID, BAD)
  add(dd + "-null-grad", dd, lambda c: dedup(c, grad=None), INVALID, BAD)
  add(dd + "-null-uniq", dd, lambda c: dedup(c, uniq=None), INVALID, BAD)
  add(dd + "-null-summed", dd, lambda c: dedup(c, summed=None), INVALID, BAD)
  add(dd + "-n-over", dd, lambda c: dedup(c, n=OVER), UNIMPL, "8388609 ids in one call (limit 2^23)")

  # kv_unsorted_segment_sum(t, segment_ids, data, n, num_segments, out, stream)
  us = "kv_unsorted_segment_sum"
  def segsum(c, seg=0, data=0, n=N, nseg=4, out=0):
    pick = lambda p: c.P if p == 0 else p
    return (c.T, pick(seg), pick(data), n, nseg, pick(out), c.st)
  add(us + "-n<0", us, lambda c: segsum(c, n=-1), INVALID, BAD)
  add(us + "-num_segments<0", us, lambda c: segsum(c, nseg=-1), INVALID, BAD)
  add(us + "-num_segments-over", us, lambda c: segsum(c, nseg=1 << 31), INVALID, BAD)
  add(us + "-null-segment-ids", us, lambda c: segsum(c, seg=None), INVALID, BAD)
  add(us + "-null-data", us, lambda c: segsum(c, data=None), INVALID, BAD)
  add(us + "-null-out", us, lambda c: segsum(c, out=None), INVALID, BAD)
  add(us + "-n-over", us, lambda c: segsum(c, n=OVER), UNIMPL, "8388609 rows in one call (limit 2^23)")
  add(us + "-num_segments=0", us, lambda c: segsum(c, nseg=0, out=None), OK, SENTINEL)

  # kv_unique(t, ids, counts, n, uniq, uniq_counts, inverse, num_unique, num_unique_dev, stream)
  uq = "kv_unique"
  def unique(c, ids=0, n=N, uniq=0, nu=0):
    pick = lambda p: c.P if p == 0 else p
    return (c.T, pick(ids), None, n, pick(uniq), None, None, _cnt() if nu == 0 else nu, None, c.st)
  add(uq + "-both-counts-null", uq, lambda c: unique(c, nu=None), INVALID, "num_unique and num_unique_dev are both null")
  add(uq + "-n=0", uq, lambda c: unique(c, ids=None, n=0, uniq=None), OK, SENTINEL)
  add(uq + "-n<0", uq, lambda c: unique(c, n=-1), INVALID, BAD)
  add(uq + "-null-ids", uq, lambda c: unique(c, ids=None), INVALID, BAD)
  add(uq + "-null-uniq", uq, lambda c: unique(c, uniq=None), INVALID, BAD)
  add(uq + "-n-over", uq, lambda c: unique(c, n=OVER), UNIMPL, "8388609 ids in one call (limit 2^23)")

  # kv_delete(t, ids, n, num_deleted, stream): the pointer check, the precondition, then n == 0
  add("kv_delete-n<0", "kv_delete", lambda c: (c.T, c.P, -1, _cnt(), c.st), INVALID, "indices pointer is null")
  add("kv_delete-null-ids", "kv_delete", lambda c: (c.T, None, N, _cnt(), c.st), INVALID, "indices pointer is null")
  add("kv_delete-null-ids-before-uninit", "kv_delete", lambda c: (c.U, None, N, _cnt(), c.st), INVALID, "indices pointer is null")
  add("kv_delete-uninit-n=0", "kv_delete", lambda c: (c.U, None, 0, _cnt(), c.st), PRECOND, UNINIT)
  add("kv_delete-uninit", "kv_delete", lambda c: (c.U, c.P, N, _cnt(), c.st), PRECOND, UNINIT)
  add("kv_delete-n=0", "kv_delete", lambda c: (c.T, None, 0, None, c.st), OK, SENTINEL)

  # kv_delete_with_timestamp(t, threshold, dry_run, out_keys, count, stream)
  dt = "kv_delete_with_timestamp"
  add(dt + "-null-count", dt, lambda c: (c.T, 7, 1, None, None, c.st), INVALID, "count / delete_keys pointer is null")
  add(dt + "-null-keys", dt, lambda c: (c.T, 7, 0, None, _cnt(), c.st), INVALID, "count / delete_keys pointer is null")
  add(dt + "-uninit", dt, lambda c: (c.U, 7, 1, None, _cnt(), c.st), PRECOND, UNINIT)
  add(dt + "-no-dry-run", dt, lambda c: (c.T, 7, 0, c.P, _cnt(), c.st), PRECOND,
      "the table was used between the dry run and kv_delete_with_timestamp: the key buffer sized from the count may be "
      "too small; count again")

  # the point queries (t, ids, n, out, stream): pointers, the precondition, then n == 0
  for fn in ("kv_get_count", "kv_get_timestamp"):
    add(fn + "-n<0", fn, lambda c: (c.T, c.P, -1, c.P, c.st), INVALID, NULL_IO)
    add(fn + "-null-ids", fn, lambda c: (c.T, None, N, c.P, c.st), INVALID, NULL_IO)
    add(fn + "-null-out", fn, lambda c: (c.T, c.P, N, None, c.st), INVALID, NULL_IO)
    add(fn + "-uninit", fn, lambda c: (c.U, c.P, N, c.P, c.st), PRECOND, UNINIT)
    add(fn + "-uninit-n=0", fn, lambda c: (c.U, None, 0, None, c.st), PRECOND, UNINIT)
    add(fn + "-n=0", fn, lambda c: (c.T, None, 0, None, c.st), OK, SENTINEL)

  # the two-phase exports: a fill without a count in front of it
  add("kv_export_fill-no-count", "kv_export_fill", lambda c: (c.T, 2, c.P, c.P, None, None, None, c.st), PRECOND,
      "the table was used between kv_export_count and kv_export_fill: " + RECOUNT)
  add("kv_export_delta_count-null-counts", "kv_export_delta_count", lambda c: (c.T, 6, None, c.st), INVALID, "counts pointer is null")
  add("kv_export_delta_count-uninit", "kv_export_delta_count",
      lambda c: (c.U, 6, _arr(ctypes.c_int64, 0, 0, 0, 0), c.st), PRECOND, UNINIT)
  add("kv_export_delta_fill-uninit", "kv_export_delta_fill", lambda c: (c.U, 6, c.P, c.P, c.P, c.P, c.P, c.P, c.st), PRECOND, UNINIT)
  add("kv_export_delta_fill-no-count", "kv_export_delta_fill", lambda c: (c.T, 6, c.P, c.P, c.P, c.P, c.P, c.P, c.st), PRECOND,
      "the table was used between kv_export_delta_count and kv_export_delta_fill: " + RECOUNT)

  # kv_insert(t, ids, values, n, stream) — never asks for an init table
  add("kv_insert-n=0", "kv_insert", lambda c: (c.U, None, None, 0, c.st), OK, SENTINEL)
  add("kv_insert-n<0", "kv_insert", lambda c: (c.T, c.P, c.P, -1, c.st), INVALID, BAD)
  add("kv_insert-null-ids", "kv_insert", lambda c: (c.T, None, c.P, N, c.st), INVALID, BAD)
  add("kv_insert-null-values", "kv_insert", lambda c: (c.T, c.P, None, N, c.st), INVALID, BAD)

  # kv_scatter_update(t, ids, updates, n, op, stream): op 0 assign .. 6 max
  su = "kv_scatter_update"
  add(su + "-op<0", su, lambda c: (c.T, c.P, c.P, N, -1, c.st), INVALID, "unsupported update operation -1")
  add(su + "-op-7", su, lambda c: (c.T, c.P, c.P, N, 7, c.st), INVALID, "unsupported update operation 7")
  add(su + "-uninit-n=0", su, lambda c: (c.U, None, None, 0, 1, c.st), OK, SENTINEL)
  add(su + "-n<0", su, lambda c: (c.T, c.P, c.P, -1, 1, c.st), INVALID, BAD)
  add(su + "-null-ids", su, lambda c: (c.T, None, c.P, N, 1, c.st), INVALID, BAD)
  add(su + "-null-updates", su, lambda c: (c.T, c.P, None, N, 1, c.st), INVALID, BAD)
  add(su + "-assign-uninit", su, lambda c: (c.U, c.P, c.P, N, 0, c.st), PRECOND, UNINIT)
  add(su + "-add-one-id-uninit", su, lambda c: (c.U, c.P, c.P, 1, 1, c.st), PRECOND, UNINIT)

  # the imports take int64 keys
  add("kv_import-int32-keys", "kv_import", lambda c: (c.T32, c.P, c.P, N, None, 0, None, None, 0, c.st), UNIMPL,
      "import with int32 keys")
  add("kv_import_delta-int32-keys", "kv_import_delta",
      lambda c: (c.T32, c.P, c.P, N, None, 0, None, None, 0, None, 0, 6, c.st), UNIMPL, "import with int32 keys")
  return c


@pytest.mark.gpu
@pytest.mark.parametrize("fn, args, rc, msg", _table_cases())
def test_refused_before_any_launch(tables, fn, args, rc, msg):
  _call(fn, args(tables), rc, msg)


@pytest.mark.gpu
def test_int32_and_int64_keys_give_equal_outputs():
  """kv_gather_or_insert, kv_gather_or_zeros, kv_get_count, kv_get_timestamp, kv_lookup_sparse (int32, then int64 segment
  ids) and kv_delete on two tables that differ in the key type alone: bit-equal outputs (a key's row and init row depend
  on its value, not on its width)."""
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  L = _lib.lib()
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  D, NSEG = 8, 40
  rng = np.random.default_rng(17)
  keys = rng.choice(np.arange(-60, 140), 100, replace=False)
  ids = rng.permutation(np.concatenate([keys, rng.choice(keys, 200)]))      # 300 ids over 100 keys, every key met
  probe = np.concatenate([keys, np.arange(1000, 1050)])                  # hits and misses
  gone = keys[::3]
  seg = np.sort(rng.integers(0, NSEG, ids.size))
  init = torch.as_tensor(rng.standard_normal((16, D)).astype(np.float32)).cuda()
  dev = lambda a, dt: torch.as_tensor(np.asarray(a).astype(dt)).cuda()
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  seg32, seg64 = dev(seg, np.int32), dev(seg, np.int64)
  outs = []
  for key_dtype, np_dt in ((I32, np.int32), (I64, np.int64)):
    h = ctypes.c_void_p()
    _lib.check(L.kv_create(key_dtype, _lib.KV_DT_FLOAT, D, 0, 0, 0, ctypes.byref(h)))
    try:
      _lib.check(L.kv_set_clock_days(h, 20000))
      _lib.check(L.kv_set_seed(h, 5))
      _lib.check(L.kv_init_table(h, p(init), 16, st))
      d_ids, d_probe, d_gone = dev(ids, np_dt), dev(probe, np_dt), dev(gone, np_dt)
      rows = lambda n: torch.full((n, D), float("nan"), device="cuda")
      words = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda")
      got = [rows(ids.size), rows(probe.size), words(probe.size), words(probe.size), rows(NSEG), rows(NSEG), rows(probe.size)]
      _lib.check(L.kv_gather_or_insert(h, p(d_ids), None, ids.size, p(got[0]), st))
      _lib.check(L.kv_gather_or_zeros(h, p(d_probe), probe.size, p(got[1]), st))
      _lib.check(L.kv_get_count(h, p(d_probe), probe.size, p(got[2]), st))
      _lib.check(L.kv_get_timestamp(h, p(d_probe), probe.size, p(got[3]), st))
      _lib.check(L.kv_lookup_sparse(h, p(d_ids), p(seg32), I32, None, ids.size, NSEG, _lib.KV_COMBINER_MEAN, 1, p(got[4]), st))
      _lib.check(L.kv_lookup_sparse(h, p(d_ids), p(seg64), I64, None, ids.size, NSEG, _lib.KV_COMBINER_SQRTN, 1, p(got[5]), st))
      n_del = ctypes.c_int64()
      _lib.check(L.kv_delete(h, p(d_gone), gone.size, ctypes.byref(n_del), st))
      _lib.check(L.kv_gather_or_zeros(h, p(d_probe), probe.size, p(got[6]), st))
      torch.cuda.synchronize()
      outs.append([g.cpu().numpy() for g in got] + [np.array([n_del.value])])
    finally:
      L.kv_destroy(h)
  names = ["gather_or_insert", "gather_or_zeros", "get_count", "get_timestamp", "lookup_sparse int32 segments",
           "lookup_sparse int64 segments", "gather_or_zeros after delete", "num_deleted"]
  for name, a, b in zip(names, outs[0], outs[1]):
    assert not np.isnan(a.astype(np.float64)).any(), name
    np.testing.assert_array_equal(a, b, err_msg=name)
  # the sequence did something: hits and misses, counts of the two lookups, a third of the keys gone
  a = outs[1]
  assert a[1][:100].any(axis=1).all() and not a[1][100:].any()
  assert (a[2][:100] > 0).all() and a[7][0] == gone.size == 34
  assert not a[6][:100:3].any() and a[6][1:100:3].any(axis=1).all()
