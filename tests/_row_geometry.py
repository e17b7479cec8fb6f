"""The row geometry of every kernel family, restated: which instantiation a dim runs in each pipeline, the committed
list of dims that reaches every one of them at its edges, and the one batch the row-geometry tests run on.

  class_of(pipeline, D)   the instantiation dim D takes in `pipeline`, restated from the one dispatch table in the sources,
                          kv_row_geom.h (tests/test_row_geometry.py holds this restatement, for every dim, against what
                          that header selects, and the launchers below against the header):
      "sorted"        (V, LPR, K) of k_apply / k_apply_fin            with_row_geom<SORTED_MAX_Q, true>   kv_kernels.h launch_apply_t
      "entry"         (V, LPR, K) of k_papply / k_uapply, or None     with_row_geom<ENTRY_MAX_Q>          kv_papply.h, kv_uapply.h, kv_sums.hip
      "row_copy"      lanes per row of the row-copy kernels, or None  row_lanes / with_lanes
      "gather"        VQ of k_gather (0: the generic body)            pow2_vectors(D, 256)                kvhip.hip launch_gather
      "gather_zeros"  q of k_gather_or_zeros_w, or 0 (8-lane kernel)  pow2_vectors(D, 64)                 kv_ops.hip kv_gather_or_zeros
      "sparse_zeros"  VQ of lsz_body (0: the whole wave)              pow2_vectors(D, 64)                 kv_ops.hip sparse_zeros_lanes
      "occ_sum"       NC of k_occ_sum                                 kvhip.hip      launch_occ_sum
  DIMS                for every class of every pipeline its smallest dim, its largest dim and, where the class has one,
                      a dim whose last lane or k vector is partly masked
  REFUSED             dims the fused kernels do not serve (kvhip.hip dim_supported)
  draw_batch          ids at the smallest size that reaches every branch of the apply kernels (kv_device.h LCOLD, HC, TILE)
"""
import numpy as np

F = np.float32

# kv_device.h
LCOLD, HC, TBT, IPT = 16, 128, 512, 4
TILE = TBT * IPT
# kv_kernels.h: k_apply_fin
TBF = 1024
LDS_NO_ASK = 64 * 1024          # what a launch gets without asking (kv_kernels.h LDS_NO_ASK)
LDS_PER_CU = 160 * 1024         # gfx950

PIPELINES = ("sorted", "entry", "row_copy", "gather", "gather_zeros", "sparse_zeros", "occ_sum")

# (largest q = D / 4, (V, LPR, K)): kv_row_geom.h Float4Ladder, launch_apply_t's float4 rows; the entry-list kernels stop at q = 64
_F4 = [(1, (4, 1, 1)), (2, (4, 2, 1)), (4, (4, 4, 1)), (8, (4, 8, 1)), (16, (4, 8, 2)), (32, (4, 16, 2)), (64, (4, 64, 1)),
       (128, (4, 64, 2)), (256, (4, 64, 4))]
# (largest D, (V, LPR, K)): kv_row_geom.h ScalarLadder, launch_apply_t's scalar rows
_SC = [(1, (1, 1, 1)), (2, (1, 2, 1)), (4, (1, 4, 1)), (8, (1, 8, 1)), (16, (1, 16, 1)), (32, (1, 32, 1)), (64, (1, 64, 1)),
       (128, (1, 64, 2)), (256, (1, 64, 4))]
_ENTRY_Q = 64                   # kv_row_geom.h ENTRY_MAX_Q (fused_ok)
_OCC = [1, 2, 4, 8, 16]         # launch_occ_sum: nc = ceil(D / 64) -> the first NC that holds it


def dim_supported(D):
  """kvhip.hip dim_supported."""
  return D >= 1 and (D <= 1024 if D % 4 == 0 else D <= 256)


def _first(table, x):
  for top, cls in table:
    if x <= top:
      return cls
  return None


def _pow2ceil(x):
  p = 1
  while p < x:
    p *= 2
  return p


def class_of(pipeline, D):
  D = int(D)
  q = D // 4
  vec = D % 4 == 0
  pow2 = vec and q >= 1 and (q & (q - 1)) == 0
  if pipeline == "sorted":
    return _first(_F4, q) if vec else _first(_SC, D)
  if pipeline == "entry":
    return _first(_F4, q) if vec and q <= _ENTRY_Q else None
  if pipeline == "row_copy":
    return min(64, _pow2ceil(max(1, q))) if vec else None
  if pipeline == "gather":
    return q if pow2 and q <= 256 else 0
  if pipeline in ("gather_zeros", "sparse_zeros"):
    return q if pow2 and q <= 64 else 0
  if pipeline == "occ_sum":
    nc = (D + 63) // 64
    return next((c for c in _OCC[:-1] if nc <= c), _OCC[-1])
  raise KeyError(pipeline)


def width_of(pipeline, D):
  """Elements the class of D spans (a dim below it leaves lanes or k vectors masked); None: the class has no width."""
  c = class_of(pipeline, D)
  if pipeline in ("sorted", "entry"):
    return None if c is None else c[0] * c[1] * c[2]
  if pipeline == "row_copy":
    return None if c is None else 4 * c
  if pipeline == "occ_sum":
    return 64 * c
  return 4 * c if c else None


def masked(pipeline, D):
  w = width_of(pipeline, D)
  return w is not None and D < w


SCALAR_DIMS = [1, 2, 3, 5, 7, 9, 15, 17, 31, 33, 63, 65, 127, 129, 254, 255]
FLOAT4_DIMS = [4, 8, 12, 16, 20, 32, 36, 60, 64, 68, 124, 128, 132, 252, 256, 260, 508, 512, 516, 572, 576, 1020, 1024]
DIMS = sorted(SCALAR_DIMS + FLOAT4_DIMS)
REFUSED = [257, 258, 1028, 2048]


def fin_lds_bytes(D):
  """(static, dynamic) LDS of a k_apply_fin block (kv_kernels.h apply_fin_body: lkeys[TBF][7] and lnk; lsum[TBF / 64][D])."""
  return TBF * 7 * 4 + 16, (TBF // 64) * D * 4 + 16


# ---- the batch -----------------------------------------------------------------------------------------------------------
# occurrences per key: cold (the per-count source lists 1..4, the last cold count LCOLD), hot in one chunk (LCOLD + 1, HC),
# hot in several chunks (HC + 1, 300: k_apply_fin, one key per wave), and one key whose occurrences lie in both tiles
PLAN = [(1, 80), (2, 12), (3, 8), (4, 8), (LCOLD, 4), (LCOLD + 1, 1), (HC, 1), (HC + 1, 1), (300, 1)] + \
       [(c, 2) for c in range(5, LCOLD)] + [(40, 1), (64, 1), (100, 1), (200, 1), (250, 1), (500, 1)]
SEEDS = (11, 12, 13)             # the seeds tests/test_gpu_row_geometry.py draws its batches with


def draw_batch(rng, key_dtype=np.int64):
  """-> {"ids": the batch (just over one tile), "keys": its distinct keys, "counts": their occurrences, "span": the key
  with occurrences in both tiles, "pre": ids of the lookup that pre-inserts half of the keys (half of those twice: with
  enter_threshold = 2 the others stay below the threshold), "new": the keys the batch inserts}."""
  counts = np.array([c for c, k in PLAN for _ in range(k)], np.int64)
  nk = counts.size
  key_dtype = np.dtype(key_dtype)
  keys = set()
  while len(keys) < nk:
    if key_dtype == np.int64 and len(keys) % 4 == 3:
      k = int(rng.integers(1 << 32, 1 << 62))          # above 2^32
    else:
      k = int(rng.integers(1, 1 << 20))
    keys.add(-k if rng.integers(0, 2) else k)
  keys = np.array(sorted(keys), np.int64)
  rng.shuffle(keys)
  ids = np.repeat(keys, counts)
  rng.shuffle(ids)
  span = int(keys[np.argmax(counts)])
  at = np.flatnonzero(ids == span)
  for want, have in ((0, at[0]), (ids.size - 1, at[-1])):      # the span key in the first and in the second tile
    ids[have], ids[want] = ids[want], ids[have]
  pre_keys = keys[::2]
  pre = np.concatenate([pre_keys, pre_keys[::2]])
  rng.shuffle(pre)
  return {"ids": ids.astype(key_dtype), "keys": keys.astype(key_dtype), "counts": counts, "span": span,
          "pre": pre.astype(key_dtype), "new": keys[1::2].astype(key_dtype)}


GQ = 2.0 ** -10                  # repeated ids: gradients are small integers times this, which any order sums exactly


def draw_grads(rng, batch, D, scale=1e-2):
  """Gradient rows of batch["ids"]: keys that occur once get full-mantissa normals, repeated ids integers in [-8, 8] times
  GQ (a key's sum stays below 2^12 GQ: exact in float32 in every order; the rule of tests/test_gpu_fuzz_optimizers.py)."""
  ids = batch["ids"]
  g = (rng.standard_normal((ids.size, D)) * scale).astype(F)
  once = set(batch["keys"][batch["counts"] == 1].tolist())
  rep = np.array([int(k) not in once for k in ids.tolist()])
  g[rep] = (rng.integers(-8, 9, (int(rep.sum()), D)) * GQ).astype(F)
  return g + F(0)


# ---- the optimizer cases: one reference trajectory per (family, dim), shared by every apply form ---------------------------
# Three steps on the batch of OPT_SEED, each a training lookup of the batch's ids and then the family's step on them; the
# state is carried.  The reference is oracle.kv_oracle for the families it restates and tests/_kv_model.py for the others;
# nothing here asks a device for anything, so tests/test_row_geometry.py asserts the generator's conditions on the CPU.
#
# Regularizers: the group families get their lasso threshold in the widest gap between the rows' norms (_kv_model
# lasso_threshold, the rule of tests/test_gpu_group_radam.py), so by the reference alone some rows blacklist and some do not
# and no row's scale 1 - threshold / norm is within 1e-4 of zero; the norms do not depend on the threshold, so the oracle
# families find theirs by running the trajectory up to the step once more.  FTRL-V2's l1 is the median |linear'|.
#
# Bars (the project's): ids, flags, frequency words and counters exact; rows rtol 1e-6 with the atol of the family's own test
# file; a var that went through a group norm (1e-6 / scale) |x| + atol per row (tests/test_gpu_parity.py
# test_group_adam_parity_with_regularizers_and_blacklist), for the two families of tests/_kv_model.py its step_allowance.
# The var of a group step is held against the same step in float64 from the reference's float32 inputs, within
# max(bar, 4 x the float32 reference's own distance from that float64 result): the reference and the kernel are two float32
# orders of one D-term sum.
FAMILIES = ("group_adam_v4", "group_adam_v3", "adagrad", "sparse_group_ftrl", "ftrl_v2", "group_ftrl_v2", "group_radam", "adam")
ORACLE_FAMILIES = FAMILIES[:4]
GROUP_FAMILIES = ("group_adam_v4", "group_adam_v3", "sparse_group_ftrl", "group_ftrl_v2", "group_radam")
OPT_SEED = SEEDS[0]
STEPS = 3
DAY = 20000
ENTER = 2
RTOL = 1e-6
SKIP_BELOW = 1e-4               # rows whose scale lies this close to the threshold may flip: not compared
# (atol of the var, atol of each slot table): tests/test_gpu_parity.py for the oracle's families, test_gpu_ftrl_v2.py
# _check, test_gpu_adam.py _assert_twins
ATOL = {"group_adam_v4": (1e-9, [1e-10]), "group_adam_v3": (1e-9, [1e-10]), "adagrad": (1e-9, [0.0]),
        "sparse_group_ftrl": (1e-8, [0.0, 1e-8]), "ftrl_v2": (1e-9, [1e-9, 1e-9]), "adam": (1e-9, [1e-9])}


def slot_dims(family, D):
  return {"group_adam_v4": [3 * D], "group_adam_v3": [3 * D], "adagrad": [D], "sparse_group_ftrl": [D, D], "ftrl_v2": [D, D],
          "group_ftrl_v2": [D, D], "group_radam": [5 * D], "adam": [2 * D]}[family]


def beta_pows(t):
  p1, p2 = F(0.9), F(0.999)
  for _ in range(t):
    p1, p2 = F(p1 * F(0.9)), F(p2 * F(0.999))
  return float(p1), float(p2)


def inits(family, D, rng):
  """(var init table, slot init tables)."""
  if family in ("group_ftrl_v2", "group_radam"):     # rows of two magnitudes (tests/_kv_model.py Program)
    v = rng.uniform(0.5, 1.0, (32, D)) * 0.05
    v[::2] *= 1e-3
    v = v.astype(F)
  else:
    v = (rng.standard_normal((32, D)) * 0.1).astype(F)
  const = {"adagrad": [0.1], "sparse_group_ftrl": [0.1, 0.0], "ftrl_v2": [0.1, 0.0], "group_ftrl_v2": [0.1, 0.0]}.get(family, [0.0])
  return v, [np.full((4, d), c, F) for d, c in zip(slot_dims(family, D), const)]


def step_grads(rng, batch, D):
  """draw_grads with every key's rows scaled by a power of two of its own (exact sums stay exact): the rows' norms spread."""
  g = draw_grads(rng, batch, D, scale=3e-2)
  sc = dict(zip(batch["keys"].tolist(), (2.0 ** -rng.integers(0, 7, batch["keys"].size)).tolist()))
  return (g * np.array([sc[int(k)] for k in batch["ids"].tolist()], F)[:, None]).astype(F)


def group_adam64(x, slot, g, lr, b1p, b2p, b1, b2, eps, l1, l2, l21, version):
  """oracle/kv_oracle.cc kvo_apply_group_adam's row arithmetic in float64 (the scalars start from their float32 values)
  -> (var', updated)."""
  T = np.float64
  x, slot, g = (np.asarray(t, T) for t in (x, slot, g))
  D = x.shape[1]
  lr, b1p, b2p, b1, b2, eps, l1, l2, l21 = (T(F(t)) for t in (lr, b1p, b2p, b1, b2, eps, l1, l2, l21))
  m, v, z = slot[:, :D], slot[:, D:2 * D], slot[:, 2 * D:]
  if version == 4:
    l1s, l2s, l21s, alpha = l1 * lr, l2 * lr, l21 * lr, lr * np.sqrt(1 - b2p) / (1 - b1p)
  else:
    l1s, l2s, l21s, alpha = l1, l2, l21, np.sqrt(1 - b2p) / (1 - b1p)
  m1 = b1 * m + (1 - b1) * g
  nv = b2 * v + (1 - b2) * (g * g)
  sq = np.sqrt(nv)
  first = b1 > b1p
  if version == 4:
    coef = (sq - np.sqrt(v)) if first else (sq + eps)
  else:
    coef = (sq - np.sqrt(v)) / lr if first else (sq - np.sqrt(v) + eps) / lr
  z1 = z + (alpha * m1 - coef * x)
  u = np.clip(z1, -l1s, l1s) - z1
  norm = np.sqrt((u * u).sum(axis=1))[:, None]
  thr = l21s * np.sqrt(T(D))
  y = (sq + eps) + 2 * l2s if version == 4 else (sq + eps) / lr + 2 * l2s
  with np.errstate(all="ignore"):
    x1 = np.where(norm > thr, u * (1 - thr / norm) / y, 0.0)
  return x1, (norm > thr)[:, 0]


def sparse_group_ftrl64(x, a, z, g, lr, l1, l2, l21, l2s, lrp):
  """oracle/kv_oracle.cc kvo_apply_sparse_group_ftrl's row arithmetic in float64 -> (var', updated)."""
  T = np.float64
  x, a, z, g = (np.asarray(t, T) for t in (x, a, z, g))
  D = x.shape[1]
  lr, l1, l2, l21, l2s, lrp = (T(F(t)) for t in (lr, l1, l2, l21, l2s, lrp))
  gs = g + 2 * l2s * x
  na = a + gs * gs
  z1 = z + (gs - (na ** -lrp - a ** -lrp) / lr * x)
  u = np.clip(z1, -l1, l1) - z1
  norm = np.sqrt((u * u).sum(axis=1))[:, None]
  thr = l21 * np.sqrt(T(D))
  with np.errstate(all="ignore"):
    x1 = np.where(norm > thr, u * (1 - thr / norm) / (na ** -lrp / lr + 2 * l2), 0.0)
  return x1, (norm > thr)[:, 0]


class _OracleSide(object):
  """var + slots on oracle.kv_oracle."""

  def __init__(self, family, D, seed, vinit, sinits):
    from oracle import kv_oracle as ko
    self.ko, self.family, self.D = ko, family, D
    self.tables = [ko.OracleKv(D, ENTER, vinit, day=DAY, picker=1, seed=seed)] + \
                  [ko.OracleKv(d, 0, t, day=DAY, picker=1, seed=seed) for d, t in zip(slot_dims(family, D), sinits)]

  def lookup(self, ids):
    self.tables[0].gather_or_insert(ids)

  def rows(self, j, keys):
    return self.tables[j].gather_or_zeros(keys)

  def metas(self, j, keys):
    return [self.tables[j].meta(int(k)) for k in keys]

  def counters(self, j):
    t = self.tables[j]
    return (t.map_size(), t.size(), t.sum_freq())

  def apply(self, u, s, hp):
    ko, t, f = self.ko, self.tables, self.family
    if f.startswith("group_adam"):
      ko.apply_group_adam(t[0], t[1], s, u, *hp[:9], version=hp[9])
    elif f == "adagrad":
      ko.apply_adagrad(t[0], t[1], hp[0], s, u, hp[1])
    else:
      ko.apply_sparse_group_ftrl(t[0], t[1], t[2], s, u, *hp)


class _ModelSide(object):
  """var + slots on tests/_kv_model.py."""

  def __init__(self, family, D, seed, vinit, sinits):
    import _kv_model as M
    self.M, self.family, self.D = M, family, D
    self.tables = [M.Table(D, vinit, seed, DAY, ENTER)] + [M.Table(d, t, seed, DAY, 0) for d, t in zip(slot_dims(family, D), sinits)]

  def lookup(self, ids):
    self.tables[0].gather_or_insert(ids)

  def rows(self, j, keys):
    return self.tables[j].gather_or_zeros(keys)

  def metas(self, j, keys):
    return self.tables[j].metas(keys)

  def counters(self, j):
    t = self.tables[j]
    return (t.map_size(), t.size(), t.sum_freq())


def _oracle_hp(family, t, l21):
  b1p, b2p = beta_pows(t)
  if family == "group_adam_v4":
    return (0.05, b1p, b2p, 0.9, 0.999, 1e-8, 1e-3, 1e-2, l21 / 0.05, 4)        # l21s = l21 lr
  if family == "group_adam_v3":
    return (0.05, b1p, b2p, 0.9, 0.999, 1e-8, 5e-5, 1e-2, l21, 3)
  if family == "adagrad":
    return (0.05, t != 1)
  return (0.1, 1e-3, 1e-2, l21, 1e-2, -0.5)


def _oracle_norms(family, side, keys, D, hp):
  """Per key, in float64 from the float32 linear' the step stored: |clamp(linear', l1) - linear'|_2, which the op compares
  with l21 sqrt(D) and which does not depend on l21."""
  if family.startswith("group_adam"):
    z = side.rows(1, keys)[:, 2 * D:].astype(np.float64)
    l1 = float(F(hp[6]) * F(hp[0])) if hp[9] == 4 else float(F(hp[6]))
  else:
    z = side.rows(2, keys).astype(np.float64)
    l1 = float(F(hp[1]))
  u = np.clip(z, -l1, l1) - z
  return np.sqrt((u * u).sum(axis=1))


_CACHE = {}


def trajectory(family, D, seed=OPT_SEED):
  """-> {"batch", "vinit", "sinits", "pre", "steps": [per step {"ids", "grad", "u", "s", "hp", "tables": [per table {"rows"
  (what the table must hold, per batch key; a group step's var: the float64 step), "tol" (absolute, per element), "metas",
  "counters"}], "clear" (keys compared), "widen" (per key: max(1, 4 x the reference's own error on that row in units of its bar)), "ref_err",
  "black" (keys blacklisted now), "live" (keys the step updated or blacklisted), "zeros" (elements FTRL-V2's l1 zeroed)}]}.
  Cached: every apply form of a (family, dim) runs the same trajectory."""
  key = (family, int(D), int(seed))
  if key not in _CACHE:
    _CACHE[key] = _oracle_trajectory(*key) if family in ORACLE_FAMILIES else _model_trajectory(*key)
  return _CACHE[key]


def _setup(family, D, seed):
  rng = np.random.default_rng([seed, D, FAMILIES.index(family)])
  batch = draw_batch(np.random.default_rng(seed))
  vinit, sinits = inits(family, D, rng)
  grads = [step_grads(rng, batch, D) for _ in range(STEPS)]
  return rng, batch, vinit, sinits, grads


def _dedup(ids, grad):
  from oracle import kv_oracle as ko
  u, s, _ = ko.dedup_segment_sum(ids, grad)
  return u, s


def _oracle_trajectory(family, D, seed):
  import _kv_model as M
  rng, batch, vinit, sinits, grads = _setup(family, D, seed)
  keys, ids = batch["keys"], batch["ids"]
  group = family in GROUP_FAMILIES
  l21s = []
  # the thresholds, one step after the other: the run up to step k with the thresholds found so far shows step k's norms
  for k in range(STEPS if group else 0):
    side = _OracleSide(family, D, seed, vinit, sinits)
    side.lookup(batch["pre"])
    for t in range(k + 1):
      side.lookup(ids)
      live = np.array([m["freq"] >= ENTER for m in side.metas(0, keys)])
      hp = _oracle_hp(family, t, l21s[t] if t < k else 0.0)
      side.apply(*_dedup(ids, grads[t]), hp)
    thr = M.lasso_threshold(_oracle_norms(family, side, keys[live], D, hp), rng)
    l21s.append(thr / float(np.sqrt(F(D))))
  side = _OracleSide(family, D, seed, vinit, sinits)
  side.lookup(batch["pre"])
  nk = keys.size
  rows = [side.rows(j, keys).astype(np.float64) for j in range(len(side.tables))]
  tol = [np.zeros_like(r) for r in rows]
  clear = np.ones(nk, bool)
  steps = []
  for t in range(STEPS):
    side.lookup(ids)
    live = np.array([m["freq"] >= ENTER for m in side.metas(0, keys)])
    before = [side.rows(j, keys) for j in range(len(side.tables))]
    for j in range(1, len(side.tables)):         # a slot row the step creates starts from the init rule's row (constant tables)
      missing = np.array([m is None for m in side.metas(j, keys)])
      before[j][missing] = sinits[j - 1][0]
    u, s = _dedup(ids, grads[t])
    gk = s[[int(np.flatnonzero(u == k)[0]) for k in keys]]
    hp = _oracle_hp(family, t, l21s[t] if group else 0.0)
    side.apply(u, s, hp)
    new = [side.rows(j, keys) for j in range(len(side.tables))]
    metas = [side.metas(j, keys) for j in range(len(side.tables))]
    av, aslots = ATOL[family]
    widen, ref_err, black = np.ones((nk, 1)), 0.0, np.zeros(nk, bool)
    for j in range(1, len(side.tables)):
      rows[j][live] = new[j][live]
      tol[j][live] = RTOL * np.abs(new[j][live]) + aslots[j - 1]
    if group:
      norm = _oracle_norms(family, side, keys, D, hp)
      thr = l21s[t] * float(np.sqrt(F(D)))
      with np.errstate(all="ignore"):
        scale = 1.0 - thr / np.maximum(norm, 1e-300)
      clear &= ~live | (np.abs(scale) > SKIP_BELOW)
      black = np.array([m["blacklist"] for m in metas[0]]) & live
      if family.startswith("group_adam"):
        x64, upd = group_adam64(before[0][live], before[1][live], gk[live], *hp)
      else:
        x64, upd = sparse_group_ftrl64(before[0][live], before[1][live], before[2][live], gk[live], *hp)
      bar = RTOL / np.maximum(scale[live], SKIP_BELOW)[:, None] * np.abs(x64) + av
      ok = clear[live]
      assert np.array_equal(upd[ok], ~black[live][ok]), (family, D, t)
      err = (np.abs(new[0][live].astype(np.float64) - x64) / bar).max(axis=1)      # per row, in units of its bar
      ref_err = float(err[ok].max())
      widen[live] = np.maximum(1.0, 4.0 * err)[:, None]
      rows[0][live], tol[0][live] = x64, bar
    else:
      rows[0][live] = new[0][live]
      tol[0][live] = RTOL * np.abs(new[0][live]) + av
    steps.append({"ids": ids, "grad": grads[t], "u": u, "s": s, "hp": hp, "clear": clear.copy(), "widen": widen,
                  "ref_err": ref_err, "black": black, "live": live, "zeros": None,
                  "tables": [{"rows": rows[j].copy(), "rows32": new[j].astype(np.float64), "tol": tol[j].copy(), "metas": metas[j],
                              "counters": side.counters(j)} for j in range(len(side.tables))]})
  return {"batch": batch, "vinit": vinit, "sinits": sinits, "steps": steps}


def _model_trajectory(family, D, seed):
  import _ftrl_ref as RF
  import _kv_model as M
  import _radam_ref as RR
  rng, batch, vinit, sinits, grads = _setup(family, D, seed)
  keys, ids = batch["keys"], batch["ids"]
  group = family in GROUP_FAMILIES
  side = _ModelSide(family, D, seed, vinit, sinits)
  var, slots = side.tables[0], side.tables[1:]
  side.lookup(batch["pre"])
  nk = keys.size
  pos = {int(k): i for i, k in enumerate(keys.tolist())}
  rows = [side.rows(j, keys).astype(np.float64) for j in range(len(side.tables))]
  clear = np.ones(nk, bool)
  steps = []
  for t in range(STEPS):
    side.lookup(ids)
    u, s = _dedup(ids, grads[t])
    b1p, b2p = beta_pows(t)
    seen = {}

    def hp_fn(x, srows, g):
      if family == "adam":
        return (0.05, b1p, b2p, 0.9, 0.999, 1e-8)
      if family == "ftrl_v2":      # l1 = the median |linear'|: about half of the elements are zeroed
        lr, _, _, two_l2s, lrp = RF._hp(0.1, 0.0, 1e-2, 1e-2, -0.5)
        z1 = RF._linear(x, srows[0], srows[1], g, lr, two_l2s, lrp)[1]
        return (0.1, float(np.median(np.abs(z1))), 1e-2, 1e-2, -0.5)
      if family == "group_ftrl_v2":
        hp0 = (0.1, 0.0, 1e-2, 1e-2, -0.5)
        return (0.1, M.lasso_threshold(M.linear_norms(family, x, srows, g, hp0)[0], rng)) + hp0[2:]
      tract, ams = [(False, False), (True, False), (True, True)][t]      # every branch of tests/_kv_model.py RADAM_BRANCHES
      hp0 = (0.1, b1p, b2p, 0.9, 0.999, 1e-7, 0.0, 1e-2, 0.0, 0.4, tract, ams, t == 1)
      l1 = float(np.median(np.abs(M.linear_norms(family, x, srows, g, hp0)[1])))
      hp1 = hp0[:6] + (l1,) + hp0[7:]
      return hp1[:8] + (M.lasso_threshold(RR.row_norms(x, srows[0], g, *hp1), rng) / float(np.sqrt(D)),) + hp1[9:]

    res = M.apply_step(family, var, slots, u, s, hp_fn, bar=group)
    hp = res["hp"]
    live = np.zeros(nk, bool)
    li = np.array([pos[k] for k in res["keys"]], np.int64)
    live[li] = True
    new = [side.rows(j, keys) for j in range(len(side.tables))]
    tol = [side.tables[j].tols(keys) for j in range(len(side.tables))]
    for j in range(len(side.tables)):
      rows[j] = new[j].astype(np.float64)
    widen, ref_err, black, zeros = np.ones((nk, 1)), 0.0, np.zeros(nk, bool), None
    if group:
      al = res["allow"]
      with np.errstate(all="ignore"):
        scale = 1.0 - 1.0 / res["ratio"]
      c = np.abs(scale) > SKIP_BELOW
      clear[li] &= c
      black[li] = ~res["updated"]
      if family == "group_ftrl_v2":
        x64, _, _, upd = RF.group_ftrl_v2(al["x"], al["srows"][0], al["srows"][1], al["g"], *hp, dtype=np.float64)
      else:
        x64, _, upd = RR.group_radam(al["x"], al["srows"][0], al["g"], *hp, dtype=np.float64)
      assert np.array_equal(upd[c], res["updated"][c]), (family, D, t)
      bar = al["tout"][0]
      e = np.abs(al["new"][0].astype(np.float64) - x64)
      ok = c & res["updated"]
      with np.errstate(all="ignore"):
        err = np.where(bar > 0, e / bar, 0.0).max(axis=1)      # per row, in units of its bar
      ref_err = float(err[ok].max())
      widen[li] = np.maximum(1.0, 4.0 * np.where(ok, err, 0.0))[:, None]
      rows[0][li] = np.where(res["updated"][:, None], x64, 0.0)
    else:
      av, aslots = ATOL[family]
      tol = [RTOL * np.abs(new[0]) + av] + [RTOL * np.abs(new[j]) + aslots[j - 1] for j in range(1, len(new))]
      for j in range(len(tol)):
        tol[j][~live] = 0.0 if t == 0 else np.maximum(steps[-1]["tables"][j]["tol"][~live], 0.0)
      if family == "ftrl_v2":
        zeros = (int((new[0][live] == 0).sum()), int(new[0][live].size))
    steps.append({"ids": ids, "grad": grads[t], "u": u, "s": s, "hp": hp, "clear": clear.copy(), "widen": widen,
                  "ref_err": ref_err, "black": black, "live": live, "zeros": zeros,
                  "tables": [{"rows": rows[j].copy(), "rows32": new[j].astype(np.float64), "tol": np.array(tol[j], np.float64),
                              "metas": side.metas(j, keys), "counters": side.counters(j)} for j in range(len(side.tables))]})
  return {"batch": batch, "vinit": vinit, "sinits": sinits, "steps": steps}
