"""The two per-key update paths of csrc/kv_key_update.h agree bit for bit: the LEAN one (LeanCtx / key_update: the var
row's slot mirror stands, nobody looks at the slot table's index or records) and the GENERAL one (prefetch_state /
finish_key: the slot row is resolved, validated, marked).  Two (var, slot) pairs get the same batches.  Pair L is what
every pre-sized training table is — one chunk, the slot attached, deterministic sums — so its applies are lean; pair G is
the same plus delta tracking on the var, which sends every key of every launch through finish_key.  Both apply kernels
are driven: k_papply (token lookup + the apply of the same batch) and k_uapply (unique ids), at the row geometries the
kernels distinguish (dim 4: one lane per row; 32 and 64: eight lanes, one and two steps; 256: a whole wave).  What is
compared — var rows, slot rows, frequency words and flags of every key — is compared between L and G, exactly; the
oracle is not asked (tests/test_gpu_slot_mirrors.py and the parity suites do that).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F = np.float32
DAY = 20000
NKEYS, NIDS, HOT, LATE = 40, 300, 60, 5


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


@pytest.fixture(scope="module")
def batches():
  """three steps of 300 ids over 40 keys (negative ones too): key 7 carries 60 ids of every step — a hot item with more
  than 16 sources —, every other key of the step at least one, and five keys appear first in step 2"""
  rng = np.random.default_rng(20261)
  keys = np.arange(NKEYS, dtype=np.int64) * 37 - 300
  late = keys[-LATE:]
  out = []
  for t in range(3):
    pool = keys if t >= 1 else keys[:-LATE]
    rest = pool[pool != keys[7]]
    ids = np.concatenate([np.full(HOT, keys[7]), rest, rng.choice(rest, NIDS - HOT - rest.size)])
    rng.shuffle(ids)
    assert ids.size == NIDS and np.unique(ids).size == pool.size
    out.append(ids)
  assert not np.isin(late, out[0]).any() and np.isin(late, out[1]).all()
  return keys, out


def _table(ops, D, init, thr=0, seed=5):
  h = ops.kv_variable([D], enter_threshold=thr, capacity_hint=4096)   # the whole slab is chunk 0
  ops.kv_set_clock_days(h, DAY)
  ops.kv_set_seed(h, seed)
  ops.init_kv_variable_v2(h, np.asarray(init, F))
  return h


SLOT = {"adam4": (3, 0.0), "adagrad": (1, 0.1), "radam": (5, 0.0)}   # slot row = mult x dim floats, init value


def _pairs(ops, name, D, thr=0):
  """(L, G): same init tables and seeds; G's var tracks deltas"""
  rng = np.random.default_rng(7 + D)
  init = (rng.uniform(0.5, 1.0, (64, D)) * 0.05).astype(F)
  mult, val = SLOT[name]
  out = []
  for general in (False, True):
    hv = _table(ops, D, init, thr)
    hs = _table(ops, mult * D, np.full((16, mult * D), val, F))
    ops.kv_attach_slot(hv, hs)
    ops.kv_set_deterministic(hv, 1)
    if general:
      ops.kv_set_delta_tracking(hv, True)
    out.append((hv, hs))
  return out


def _beta_pows(t):
  p1, p2 = F(0.9), F(0.999)
  for _ in range(t):
    p1, p2 = F(p1 * F(0.9)), F(p2 * F(0.999))
  return float(p1), float(p2)


def _apply(ops, name, hs, grad, ids, t, unique, l21=0.0):
  b1p, b2p = _beta_pows(t)
  if name == "adam4":
    ops.kv_variable_group_sparse_apply_adam_v4(hs[0], hs[1], grad, ids, 0.05, b1p, b2p, 0.9, 0.999, 1e-8, 1e-4, 1e-3, l21,
                                               unique_indices=unique)
  elif name == "adagrad":
    ops.kv_variable_sparse_apply_adagrad(hs[0], hs[1], 0.05, grad, ids, unique_indices=unique)
  else:
    ops.kv_variable_group_sparse_apply_rectified_adam(hs[0], hs[1], grad, ids, 0.05, b1p, b2p, 0.9, 0.999, 1e-7, 1e-4, 1e-3, l21,
                                                      0.4, True, True, False, unique_indices=unique)


def _run(ops, name, D, steps, unique, lookup, thr=0, l21=0.0):
  """the steps on fresh pairs L and G; returns both.  lookup: a training lookup of the step's ids in front of the apply
  (not unique: the apply gets the very same tensor, so it consumes the lookup's index — the token); l21: step 1's only"""
  L, G = _pairs(ops, name, D, thr)
  rng = np.random.default_rng(99 + D)
  for t, ids in enumerate(steps):
    raw = ids
    if unique:
      ids = np.unique(ids)
    grad = rng.normal(0, 1e-2, (ids.size, D)).astype(F)
    for hs in (L, G):
      dids = torch.from_numpy(ids).cuda()
      if lookup:
        ops.kv_variable_gather_or_insert_v2(hs[0], torch.from_numpy(raw).cuda() if unique else dids)
      _apply(ops, name, hs, torch.from_numpy(grad).cuda(), dids, t, unique, l21 if t == 0 else 0.0)
  return L, G


def _np(t):
  return t.detach().cpu().numpy()


def _assert_paths_agree(ops, L, G, keys):
  # the comparison is void unless L was lean and G was not
  assert ops.kv_get_stat(L[0], ops.KV_STAT_MIRROR_APPLIES) > 0
  assert ops.kv_get_stat(G[0], ops.KV_STAT_MIRROR_APPLIES) == 0
  for a, b in zip(L, G):   # (reading the slot table ends L's mirror epoch: the dirty copies go back first)
    ra, rb = _np(ops.kv_variable_gather_or_zeros_v2(a, keys)), _np(ops.kv_variable_gather_or_zeros_v2(b, keys))
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
    ma, mb = ops.kv_get_meta(a, keys), ops.kv_get_meta(b, keys)
    assert all(m is not None for m in ma)
    assert ma == mb
  return ops.kv_get_meta(L[0], keys), ops.kv_get_meta(L[1], keys)


@pytest.mark.parametrize("D", [4, 32, 64, 256])
@pytest.mark.parametrize("name", ["adam4", "adagrad", "radam"])
def test_token_apply_lean_equals_general(ops, batches, name, D):
  keys, steps = batches
  L, G = _run(ops, name, D, steps, unique=False, lookup=True)
  mv, ms = _assert_paths_agree(ops, L, G, keys)
  occ = sum(int((s == keys[7]).sum()) for s in steps)
  assert mv[7]["freq"] == occ and ms[7]["freq"] == len(steps)   # the lookups count ids, the applies steps


@pytest.mark.parametrize("D", [4, 32, 64, 256])
@pytest.mark.parametrize("name", ["adam4", "adagrad", "radam"])
def test_unique_apply_lean_equals_general(ops, batches, name, D):
  """no lookup: the op itself inserts the keys it meets first (35 in step 1, five in step 2), from the init rule"""
  keys, steps = batches
  L, G = _run(ops, name, D, steps, unique=True, lookup=False)
  mv, ms = _assert_paths_agree(ops, L, G, keys)
  assert mv[7]["freq"] == 1 and ms[7]["freq"] == len(steps)


@pytest.mark.parametrize("unique", [False, True])
def test_frequency_filter_and_blacklist_lean_equals_general(ops, batches, unique):
  """enter_threshold 2: a key seen once so far is skipped (its slot row is not even created), so keys enter in different
  steps; l21 above every row's lasso norm in step 1 only: the rows updated there are blacklisted (all zeros), and taken off
  the blacklist by step 2's update — on L through the mirror"""
  keys, steps = batches
  D = 32
  L, G = _run(ops, "adam4", D, steps[:1], unique, lookup=True, thr=2, l21=10.0)
  assert any(m["blacklist"] for m in ops.kv_get_meta(L[0], keys) if m)
  L, G = _run(ops, "adam4", D, steps, unique, lookup=True, thr=2, l21=10.0)
  _assert_paths_agree(ops, L, G, keys)
