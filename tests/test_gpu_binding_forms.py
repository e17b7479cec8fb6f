"""The Python wrappers of the optimizer ops against the C ABI called by hand: argument order and marshalling.

For every optimizer family the public wrapper (gen_kv_variable_ops) runs one step on one set of tables, and the same call
is made through _lib.lib() with every argument written out here on a twin set built from the same seed; var and slot
exports, and the rows at the ids, must be equal bit for bit.  Three forms each, single-table and batched (2 tables): the token of a preceding
lookup of the same tensor, no token (by hand: the plain entry point, which is the token form with token 0 — kvhip.h), and
unique_indices=True.  The 64 ids of a table are distinct, so no summation order takes part and the _unique promise holds:
bit equality is the expectation, not a tolerance.  Every hyper-parameter has its own value, so two swapped floats change
the result; RectifiedAdam's three flags run in two settings, so that every swap of two of them changes one of them, and
Adagrad runs with update_slots on and off."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

D, N = 8, 64
F = np.float32
FORMS = ["tok", "plain", "unique"]
vp, u64, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


@pytest.fixture(scope="module")
def L():
  from tfplus_amd import _lib
  return _lib.lib()


# family -> (dims of the slot tables in units of D, their init values)
SLOTS = {"group_adam_v4": [(3, 0.0)], "group_adam_v3": [(3, 0.0)], "adagrad": [(1, 0.1)], "adagrad_keep": [(1, 0.1)],
         "sparse_group_ftrl": [(1, 0.1), (1, 0.0)], "ftrl_v2": [(1, 0.1), (1, 0.0)], "group_ftrl_v2": [(1, 0.1), (1, 0.0)],
         "radam_tan": [(5, 0.0)], "radam_tna": [(5, 0.0)]}
FAMILIES = sorted(SLOTS)


def _table(ops, dim, init, seed):
  h = ops.kv_variable([dim])
  ops.kv_set_clock_days(h, 20000)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, init)
  return h


def _tables(ops, family, k):
  """[var, slot...] of table k; twins come from calling this twice."""
  rng = np.random.default_rng(40 + k)
  var = _table(ops, D, rng.uniform(0.01, 0.05, (32, D)).astype(F), 5 + k)
  return [var] + [_table(ops, m * D, np.full((16, m * D), v, F), 5 + k) for m, v in SLOTS[family]]


def _batch(k):
  rng = np.random.default_rng(7 + k)
  ids = torch.from_numpy(rng.choice(1000, N, replace=False).astype(np.int64) - 100).cuda()
  grad = torch.from_numpy(rng.normal(0, 0.1, (N, D)).astype(F)).cuda()
  return ids, grad


def _stream():
  return vp(torch.cuda.current_stream().cuda_stream)


def _p(t):
  return vp(t.data_ptr())


def _same(ops, a, b, ids):
  """Every table of the set, bit for bit: its export (keys and rows, blacklist, and the frequency list, which names every
  key of the table) and its rows at the batch's ids.  The export leaves out a row whose values are all under the cutoff
  (a slot table's zero rows, say), so the rows at the ids are compared as well: those are always N."""
  for j, (x, y) in enumerate(zip(a, b)):
    ex, ey = ops.kv_variable_export(x), ops.kv_variable_export(y)
    ox, oy = torch.argsort(ex[0]), torch.argsort(ey[0])
    assert torch.equal(ex[0][ox], ey[0][oy])
    assert torch.equal(ex[1][ox].view(torch.int32), ey[1][oy].view(torch.int32))
    assert torch.equal(torch.sort(ex[2])[0], torch.sort(ey[2])[0])
    fx, fy = torch.argsort(ex[3]), torch.argsort(ey[3])
    assert torch.equal(ex[3][fx], ey[3][fy]) and torch.equal(ex[4][fx], ey[4][fy])
    assert j > 0 or ex[3].numel() == N                  # the var holds every id of the lookup (a slot row need not exist)
    rx, ry = ops.kv_variable_gather_or_zeros_v2(x, ids), ops.kv_variable_gather_or_zeros_v2(y, ids)
    assert torch.equal(rx.view(torch.int32), ry.view(torch.int32))


# ---- the wrapper calls: the documented parameter order, the literals of the calls by hand below ---------------------------
def _wrapper(ops, family, multi):
  m = "multi" if multi else "single"
  return {
      ("group_adam_v4", "single"): lambda t, g, i, u: ops.kv_variable_group_sparse_apply_adam_v4(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, unique_indices=u),
      ("group_adam_v3", "single"): lambda t, g, i, u: ops.kv_variable_group_sparse_apply_adam_v3(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, unique_indices=u),
      ("adagrad", "single"): lambda t, g, i, u: ops.kv_variable_sparse_apply_adagrad(
          t[0], t[1], 0.05, g, i, update_slots=True, unique_indices=u),
      ("adagrad_keep", "single"): lambda t, g, i, u: ops.kv_variable_sparse_apply_adagrad(
          t[0], t[1], 0.05, g, i, update_slots=False, unique_indices=u),
      ("sparse_group_ftrl", "single"): lambda t, g, i, u: ops.kv_variable_sparse_group_sparse_apply_ftrl_v2(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 2e-4, 3e-3, -0.5, unique_indices=u),
      ("ftrl_v2", "single"): lambda t, g, i, u: ops.kv_variable_sparse_apply_ftrl_v2(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 3e-3, -0.5, unique_indices=u),
      ("group_ftrl_v2", "single"): lambda t, g, i, u: ops.kv_variable_group_sparse_apply_ftrl_v2(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 3e-3, -0.5, unique_indices=u),
      ("radam_tan", "single"): lambda t, g, i, u: ops.kv_variable_group_sparse_apply_rectified_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, 0.4, True, True, False, unique_indices=u),
      ("radam_tna", "single"): lambda t, g, i, u: ops.kv_variable_group_sparse_apply_rectified_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, 0.4, True, False, True, unique_indices=u),
      ("group_adam_v4", "multi"): lambda t, g, i, u: ops.kv_multi_group_sparse_apply_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, version=4, unique_indices=u),
      ("group_adam_v3", "multi"): lambda t, g, i, u: ops.kv_multi_group_sparse_apply_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, version=3, unique_indices=u),
      ("adagrad", "multi"): lambda t, g, i, u: ops.kv_multi_sparse_apply_adagrad(
          t[0], t[1], 0.05, g, i, update_slots=True, unique_indices=u),
      ("adagrad_keep", "multi"): lambda t, g, i, u: ops.kv_multi_sparse_apply_adagrad(
          t[0], t[1], 0.05, g, i, update_slots=False, unique_indices=u),
      ("sparse_group_ftrl", "multi"): lambda t, g, i, u: ops.kv_multi_sparse_group_sparse_apply_ftrl(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 2e-4, 3e-3, -0.5, unique_indices=u),
      ("ftrl_v2", "multi"): lambda t, g, i, u: ops.kv_multi_sparse_apply_ftrl_v2(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 3e-3, -0.5, unique_indices=u),
      ("group_ftrl_v2", "multi"): lambda t, g, i, u: ops.kv_multi_group_sparse_apply_ftrl_v2(
          t[0], t[1], t[2], g, i, 0.05, 1e-4, 1e-2, 3e-3, -0.5, unique_indices=u),
      ("radam_tan", "multi"): lambda t, g, i, u: ops.kv_multi_group_sparse_apply_rectified_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, 0.4, True, True, False, unique_indices=u),
      ("radam_tna", "multi"): lambda t, g, i, u: ops.kv_multi_group_sparse_apply_rectified_adam(
          t[0], t[1], g, i, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4, 0.4, True, False, True, unique_indices=u),
  }[family, m]


# ---- the calls by hand: include/kvhip.h's order.  `lead` is (num_tables,) for the batched entry points, else () -------------
def _by_hand(L, family, form, multi, lead, t, g, i, n, tok, st):
  pre = "kv_multi_apply_" if multi else "kv_apply_"
  tail = {"tok": (tok, st), "plain": (st,), "unique": (st,)}[form]
  sfx = {"tok": "_tok", "plain": "", "unique": "_unique"}[form]
  if family in ("group_adam_v4", "group_adam_v3"):
    fn = getattr(L, pre + "group_adam" + sfx)
    return fn(*lead, t[0], t[1], g, i, n, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4,
              {"group_adam_v4": 4, "group_adam_v3": 3}[family], *tail)
  if family == "adagrad":
    return getattr(L, pre + "adagrad" + sfx)(*lead, t[0], t[1], 0.05, g, i, n, 1, *tail)
  if family == "adagrad_keep":                                        # update_slots=False: the accumulator stays as it is
    return getattr(L, pre + "adagrad" + sfx)(*lead, t[0], t[1], 0.05, g, i, n, 0, *tail)
  if family == "sparse_group_ftrl":
    return getattr(L, pre + "sparse_group_ftrl" + sfx)(*lead, t[0], t[1], t[2], g, i, n, 0.05, 1e-4, 1e-2, 2e-4, 3e-3, -0.5, *tail)
  if family == "ftrl_v2":
    return getattr(L, pre + "ftrl_v2" + sfx)(*lead, t[0], t[1], t[2], g, i, n, 0.05, 1e-4, 1e-2, 3e-3, -0.5, *tail)
  if family == "group_ftrl_v2":
    return getattr(L, pre + "group_ftrl_v2" + sfx)(*lead, t[0], t[1], t[2], g, i, n, 0.05, 1e-4, 1e-2, 3e-3, -0.5, *tail)
  flags = {"radam_tan": (1, 1, 0), "radam_tna": (1, 0, 1)}[family]
  return getattr(L, pre + "group_rectified_adam" + sfx)(*lead, t[0], t[1], g, i, n, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4,
                                                         1e-2, 2e-4, 0.4, *flags, *tail)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
def test_single_table_wrapper_equals_the_call_by_hand(ops, L, family, form):
  a, b = _tables(ops, family, 0), _tables(ops, family, 0)
  ids, grad = _batch(0)
  before = ops.kv_variable_gather_or_insert_v2(a[0], ids if form == "tok" else ids.clone())
  _wrapper(ops, family, False)(a, grad, ids, form == "unique")

  ids_b, st = ids.clone(), _stream()
  out, tok = torch.empty((N, D), dtype=torch.float32, device=ids.device), u64(0)
  assert L.kv_gather_or_insert_tok(vp(b[0].ptr), _p(ids_b), None, N, _p(out), ctypes.byref(tok), st) == 0
  assert form != "tok" or tok.value != 0
  rc = _by_hand(L, family, form, False, (), [vp(h.ptr) for h in b], _p(grad), _p(ids_b), N, u64(tok.value), st)
  assert rc == 0, L.kv_last_error()
  _same(ops, a, b, ids)
  assert not torch.equal(ops.kv_variable_gather_or_zeros_v2(a[0], ids), before)      # ... and the step was one


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
def test_batched_wrapper_equals_the_call_by_hand(ops, L, family, form):
  a, b = [_tables(ops, family, k) for k in range(2)], [_tables(ops, family, k) for k in range(2)]
  ids, grads = zip(*[_batch(k) for k in range(2)])
  if form == "tok":
    before = ops.kv_multi_gather_or_insert([t[0] for t in a], list(ids))
  else:
    before = [ops.kv_variable_gather_or_insert_v2(t[0], i.clone()) for t, i in zip(a, ids)]
  by_role = [[t[j] for t in a] for j in range(len(a[0]))]          # vars, then each slot role
  _wrapper(ops, family, True)(by_role, list(grads), list(ids), form == "unique")

  ids_b, st = [i.clone() for i in ids], _stream()
  outs = [torch.empty((N, D), dtype=torch.float32, device=ids[0].device) for _ in range(2)]
  arr = lambda ps: (vp * 2)(*ps)
  roles = [arr([t[j].ptr for t in b]) for j in range(len(b[0]))]
  idp, gp, ns = arr([i.data_ptr() for i in ids_b]), arr([g.data_ptr() for g in grads]), (i64 * 2)(N, N)
  toks = (u64 * 2)()
  assert L.kv_multi_gather_or_insert_tok(2, roles[0], idp, None, ns, arr([o.data_ptr() for o in outs]), toks, st) == 0
  assert form != "tok" or (toks[0] != 0 and toks[1] != 0)
  rc = _by_hand(L, family, form, True, (2,), roles, gp, idp, ns, toks, st)
  assert rc == 0, L.kv_last_error()
  for k in range(2):
    _same(ops, a[k], b[k], ids[k])
    assert not torch.equal(ops.kv_variable_gather_or_zeros_v2(a[k][0], ids[k]), before[k])


def test_rectified_adam_takes_the_callers_token(ops, L):
  """token=: the caller's own batch token, from a lookup made by hand (the wrapper's lookup never saw these ids)."""
  family = "radam_tan"
  a, b = _tables(ops, family, 0), _tables(ops, family, 0)
  ids, grad = _batch(0)
  st, toks = _stream(), []
  for t in (a, b):
    out, tok = torch.empty((N, D), dtype=torch.float32, device=ids.device), u64(0)
    assert L.kv_gather_or_insert_tok(vp(t[0].ptr), _p(ids), None, N, _p(out), ctypes.byref(tok), st) == 0
    assert tok.value != 0
    toks.append(tok.value)
  ops.kv_variable_group_sparse_apply_rectified_adam(a[0], a[1], grad, ids, 0.05, 0.81, 0.998, 0.9, 0.999, 1e-7, 1e-4, 1e-2, 2e-4,
                                                    0.4, True, True, False, token=toks[0])
  rc = _by_hand(L, family, "tok", False, (), [vp(h.ptr) for h in b], _p(grad), _p(ids), N, u64(toks[1]), st)
  assert rc == 0, L.kv_last_error()
  _same(ops, a, b, ids)
