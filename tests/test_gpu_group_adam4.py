"""Group AMSGrad / group AdaBelief (kvhip.h kv_apply_group_amsgrad / kv_apply_group_adabelief, optimizer code 9) against the
float64 restatement of tests/_group_adam4_ref.py, everything at the project's unique-id bar, rtol 1e-6 / atol 1e-7.  The float32
NumPy restatement, run on the CPU over _case() for every D of DIMS, both variants and all steps, lies within 0.68 (var), 0.06 (m),
0.01 (v), 0.67 (linear) and 0.21 (acc) of that bar, so no block needs more.  An MI355X measured 0.65 (var) and 0.67 (slot row)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_adam4_ref as R  # noqa: E402
import _ranks  # noqa: E402

F = np.float32
VARIANTS = ("amsgrad", "adabelief")
DIMS = (4, 7, 36, 256, 1024)   # one float4 lane; masked scalar class; K = 2; the largest entry-list dim; the sorted pipeline's largest
N, LR, TAIL = 300, 0.05, (0.9, 0.999, 1e-7, 1e-3, 0.01)        # ..., beta1, beta2, epsilon, l1, l2
FORMS = ("plain", "tok", "unique", "counted", "multi", "sparse")
gpu, both = pytest.mark.gpu, pytest.mark.parametrize("variant", VARIANTS)


def _hp(t, l21):
  return (LR, F(0.9) ** t, F(0.999) ** t) + TAIL + (l21,)


def _bar(w):
  return 1e-6 * np.abs(w) + 1e-7


def _clear(norm, hp, D):
  thr = float(F(hp[8])) * np.sqrt(D)
  return np.abs(norm - thr) > 1e-4 * thr


@functools.lru_cache(None)
def _case(variant, D):
  """-> the var's init row, N distinct ids, [(grad, hp)] of steps 1..3.  l21 of a step = the median of the reference's own
  row norms over sqrt(D), on the float32 restatement's trajectory: half the keys take each branch"""
  rng = np.random.default_rng(1000 + D)
  init, ids = rng.uniform(-0.5, 0.5, (1, D)).astype(F), rng.choice(10 ** 6, N, replace=False).astype(np.int64)
  x, s, steps = np.tile(init, (N, 1)), np.zeros((N, 4 * D), F), []
  for t in (1, 2, 3):
    g = (rng.normal(0, 0.05, (N, D)) * rng.lognormal(0, 1, (N, 1))).astype(F)
    hp = _hp(t, F(np.median(R.step(variant, x, s, g, _hp(t, 0.0), F)[3]) / np.sqrt(D)))
    x, s = [a.astype(F) for a in R.step(variant, x, s, g, hp, F)[:2]]
    steps.append((g, hp))
  return init, ids, steps


@pytest.mark.parametrize("D", DIMS)
@both
def test_chosen_seeds_take_both_branches_within_the_skip_cap(variant, D):
  """(CPU) the reference alone: every step updates some keys and blacklists others; at most 1 % lie at the threshold"""
  init, _, steps = _case(variant, D)
  x, s = np.tile(init, (N, 1)), np.zeros((N, 4 * D), F)
  for g, hp in steps:
    _, _, upd, norm = R.step(variant, x, s, g, hp)
    assert upd.any() and not upd.all() and _clear(norm, hp, D).mean() >= 0.99
    x, s = [a.astype(F) for a in R.step(variant, x, s, g, hp, F)[:2]]


@pytest.fixture(scope="module")
def ops():
  torch = pytest.importorskip("torch")
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _pair(ops, D, init, mult=4, cap=0):
  hs = [ops.kv_variable([D], capacity_hint=cap), ops.kv_variable([mult * D], capacity_hint=cap)]
  for h, t in zip(hs, (init, np.zeros((1, mult * D), F))):
    ops.init_kv_variable_v2(h, np.asarray(t, F))
  return hs


def _rows(ops, hs, keys):
  return [ops.kv_variable_gather_or_zeros_v2(h, np.asarray(keys, np.int64)).cpu().numpy() for h in hs]


def _op(ops, variant, multi=False):
  return getattr(ops, "kv_%s_group_sparse_apply_%s" % ("multi" if multi else "variable", variant))


def _flags(ops, h, keys):
  return [(m["blacklist"], m["under_threshold"]) for m in ops.kv_get_meta(h, keys)]


def _check(ops, hs, variant, ids, x0, s0, g, hp):
  """the pair after one step from rows x0 / s0 against the float64 step, var and all four slot blocks; both rows' flags exact;
  keys at the threshold skipped (<= 1 %).  -> the rows the next step starts from"""
  x64, s64, upd, norm = R.step(variant, x0, s0, g, hp)
  clear = _clear(norm, hp, x0.shape[1])
  assert clear.mean() >= 0.99 and upd.any() and not upd.all()
  got_x, got_s = _rows(ops, hs, ids)
  assert (np.abs(got_s - s64) <= _bar(s64)).all(), np.argwhere(np.abs(got_s - s64) > _bar(s64))[:5]
  assert (np.abs(got_x - x64) <= _bar(x64))[clear].all() and not got_x[clear & ~upd].any()
  small = lambda w: ~(np.abs(w) >= 1e-20).any(axis=1)            # UpdateUnderThreshold on the row written
  want = [(not u, bool(not u or b)) for u, b in zip(upd, small(x64))]
  assert [f for f, c in zip(_flags(ops, hs[0], ids), clear) if c] == [w for w, c in zip(want, clear) if c]
  assert _flags(ops, hs[1], ids) == [(False, bool(b)) for b in small(s64)]
  return got_x, got_s


@gpu
@pytest.mark.parametrize("D", DIMS)
@both
def test_three_steps_on_distinct_ids_every_form(ops, variant, D):
  import torch
  init, ids_np, steps = _case(variant, D)
  forms = FORMS if D in (4, 36, 256) else FORMS[:3]
  twins = {f: [_pair(ops, D, init) for _ in range(2 if f == "multi" else 1)] for f in forms}
  ids = torch.from_numpy(ids_np).cuda()
  state = {f: [(np.tile(init, (N, 1)), np.zeros((N, 4 * D), F))] * len(pairs) for f, pairs in twins.items()}
  for g_np, hp in steps:
    g = torch.from_numpy(g_np).cuda()
    for f, pairs in twins.items():
      for hs in pairs:
        ops.kv_variable_gather_or_insert_v2(hs[0], ids)           # (the lookup whose token _tok takes)
      hs = pairs[0]
      assert f != "tok" or ops._token_for(hs[0], ids) != 0
      if f == "multi":
        _op(ops, variant, True)([p[0] for p in pairs], [p[1] for p in pairs], [g, g], [ids.clone(), ids.clone()], *hp)
      elif f == "sparse":                                         # one-id segments: the segment gradients ARE the rows
        ops.kv_variable_apply_sparse("group_" + variant, hs, hp, g, ids.clone(), torch.arange(N, device="cuda"), None, N, "sum")
      else:
        kw = {"unique": {"unique_indices": True}, "counted": {"unique_count": torch.tensor([N], device="cuda")}}.get(f, {})
        _op(ops, variant)(hs[0], hs[1], g, ids if f == "tok" else ids.clone(), *hp, **kw)
      state[f] = [_check(ops, p, variant, ids_np, x0, s0, g_np, hp) for p, (x0, s0) in zip(pairs, state[f])]


@gpu
@pytest.mark.parametrize("det", [1, 0])
@both
def test_repeated_ids_equal_the_deduplicated_step(ops, variant, det):
  """One key 300 times among Zipf-like repeats, D = 32, l21 = 0 (no key at the threshold).  Deterministic mode: the bits of
  kv_dedup_segment_sum + _unique.  Default mode: the kernel's sum lies within dg = (cnt - 1) 2^-24 sum|g| of the exact one
  (tests/_reorder.py's interval), so var and slot may differ from the float64 step at the exact sum by the step's change over
  [gsum - dg, gsum + dg], doubled as _reorder does, plus the bar for the float32 evaluation."""
  rng = np.random.default_rng(7)
  D, hp = 32, _hp(1, 0.0)
  init = rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  ids = np.concatenate([np.full(300, 5), np.minimum(rng.zipf(1.2, 3000), 10 ** 6), np.arange(100, 1100)]).astype(np.int64)
  rng.shuffle(ids)
  g = rng.normal(0, 0.05, (ids.size, D)).astype(F)
  raw, ded = _pair(ops, D, init), _pair(ops, D, init)
  for hs in (raw, ded):
    ops.kv_set_deterministic(hs[0], det)
  _op(ops, variant)(raw[0], raw[1], g, ids, *hp)
  u, summed, _ = ops.kv_dedup_segment_sum(ded[0], ids, g)
  _op(ops, variant)(ded[0], ded[1], summed, u, *hp, unique_indices=True)
  keys, inv, cnt = np.unique(ids, return_inverse=True, return_counts=True)
  got = [np.concatenate(_rows(ops, hs, keys), axis=1) for hs in (raw, ded)]
  if det:
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    return
  gsum, gabs = np.zeros((keys.size, D)), np.zeros((keys.size, D))
  np.add.at(gsum, inv, g.astype(np.float64))
  np.add.at(gabs, inv, np.abs(g.astype(np.float64)))
  dg = (cnt[:, None] - 1) * 2.0 ** -24 * gabs
  f = lambda gs: np.concatenate(R.step(variant, np.tile(init, (keys.size, 1)), np.zeros((keys.size, 4 * D), F), gs, hp)[:2], axis=1)
  mid = f(gsum)
  bound = 2 * np.maximum(np.abs(f(gsum - dg) - mid), np.abs(f(gsum + dg) - mid)) + _bar(mid)
  assert all((np.abs(w - mid) <= bound).all() for w in got)


@gpu
def test_the_variant_flag_decides_and_amsgrad_keeps_the_maximum(ops):
  """A step with gradient 1.0, then one with 1e-3: g - m' != g and v / (1 - beta2_power) < acc.  The v and acc blocks differ
  between the variants, each matching its own reference; AMSGrad's acc stays bit for bit, AdaBelief's moves."""
  D, ids, got = 8, np.arange(10, 40, dtype=np.int64), {}
  for variant in VARIANTS:
    hs = _pair(ops, D, np.full((1, D), 0.25, F))
    for t, scale in ((1, 1.0), (2, 1e-3)):
      (x0, s0), g = _rows(ops, hs, ids), np.full((ids.size, D), scale, F) * np.linspace(1, 2, D, dtype=F)
      _op(ops, variant)(hs[0], hs[1], g, ids, *_hp(t, 0.0), unique_indices=True)
    got[variant] = (s0, _rows(ops, hs, ids)[1])
    want = R.step(variant, x0, s0, g, _hp(2, 0.0))[1]
    assert (np.abs(got[variant][1] - want) <= _bar(want)).all()
  for sl in (slice(D, 2 * D), slice(3 * D, 4 * D)):             # v: what the second moment squares; acc: the maximum
    assert (got["amsgrad"][1][:, sl] != got["adabelief"][1][:, sl]).all()
  acc = slice(3 * D, 4 * D)
  assert np.array_equal(got["amsgrad"][0][:, acc].view(np.uint32), got["amsgrad"][1][:, acc].view(np.uint32))
  assert (got["amsgrad"][0][:, acc] > 0).all() and (got["adabelief"][1][:, acc] < got["adabelief"][0][:, acc]).all()


@gpu
@both
def test_refusals_leave_the_tables_empty(ops, variant):
  import torch
  from tfplus_amd import _lib
  D, hp = 8, _hp(1, 0.01)
  hs, ids, g = _pair(ops, D, np.ones((1, D), F)), np.arange(3, dtype=np.int64), np.full((3, D), 0.1, F)
  bad = lambda i, v: hp[:i] + (v,) + hp[i + 1:]
  cases = [([hs[0], _pair(ops, D, np.ones((1, D), F), mult=3)[1]], hp, "opt must be 4x"),
           ([hs[0], _pair(ops, D, np.ones((1, D), F), mult=5)[1]], hp, "opt must be 4x"),
           ([hs[0], hs[0]], hp, "same table"), (hs, bad(0, 0.0), "lr"), (hs, bad(1, 1.0), "beta1_power")]
  for (tabs, h, word), kw in [(c, k) for c in cases for k in ({}, {"unique_indices": True})]:
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      _op(ops, variant)(tabs[0], tabs[1], g, ids, *h, **kw)
  gids, gd, n1 = torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), torch.tensor([3], device="cuda")
  for vec, word in ((hp, "optimizer 9 reads 10"), (hp + (2.0,), "variant")):         # the generic entry's own vector
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      _lib.check(_lib.lib().kv_apply_unique_counted(hs[0].ptr, 9, hs[1].ptr, None, ops._hp_array(vec, 9), ops._p(gd), ops._p(gids),
                                                    ops._TORCH_KEY[gids.dtype], 3, ops._p(n1), ops._stream(hs[0])))
  torch.cuda.synchronize()
  assert all(int(ops.kv_variable_shape_v2(h)[0]) == 0 and ops.kv_variable_frequency(h) == 0 for h in hs)


@gpu
@both
def test_sharded_apply_takes_code_9(ops, variant):
  """world 2 over staged communicators at D = 8 against one table, at tests/test_gpu_adam.py's tolerance for the same check"""
  import torch
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76)
  D, world, hp = 8, 2, _hp(1, 0.0)
  init = rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  ref, parts = _pair(ops, D, init), [_pair(ops, D, init) for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
  grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]

  def step(r, comm):
    shs[r].lookup(comm, torch.from_numpy(ids[r]).cuda())
    torch.cuda.synchronize()
    shs[r].apply(comm, ops.OPT_GROUP_ADAM4, [parts[r][1]], torch.from_numpy(grads[r]).cuda(),
                 [float(v) for v in hp] + [float(VARIANTS.index(variant))])
  ranks = _ranks.Ranks(ops, world)
  ranks.run(step)
  ranks.close()
  ops.kv_variable_gather_or_insert_v2(ref[0], np.concatenate(ids))
  _op(ops, variant)(ref[0], ref[1], np.concatenate(grads), np.concatenate(ids), *hp)
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r in range(world):
    for got, want in zip(_rows(ops, parts[r], u[own == r]), _rows(ops, ref, u[own == r])):
      np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)


@gpu
@both
def test_captured_lookup_and_apply_replay_on_fresh_ids(ops, variant):
  """kv_prepare_capture's contract: one call outside the capture first; two replays on fresh ids equal the eager twin's bits"""
  import torch
  dev = torch.device("cuda", 0)
  D, n, hp = 32, 2000, _hp(1, 0.01)
  gen = torch.Generator(device=dev).manual_seed(3)
  ids, grad = torch.randperm(4000, device=dev, generator=gen)[:n], torch.randn(n, D, device=dev, generator=gen) * 0.05
  cap, eag = [_pair(ops, D, np.full((1, D), 0.01, F), cap=8 * n) for _ in range(2)]

  def step(hs):
    ops.kv_variable_gather_or_insert_v2(hs[0], ids)
    _op(ops, variant)(hs[0], hs[1], grad, ids, *hp)
  step(cap), step(eag)
  torch.cuda.synchronize()
  for h in cap:
    ops.kv_prepare_capture(h, 3 * n)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    step(cap)
  seen = [ids.cpu().numpy()]
  for rep in range(2):
    ids.copy_(torch.randperm(4000, device=dev, generator=gen)[:n] + 1000 * rep)
    seen.append(ids.cpu().numpy())
    graph.replay()
    step(eag)
  torch.cuda.synchronize()
  keys = np.unique(np.concatenate(seen))
  for a, b, ha, hb in zip(_rows(ops, cap, keys), _rows(ops, eag, keys), cap, eag):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ops.kv_get_meta(ha, keys) == ops.kv_get_meta(hb, keys)


@gpu
@both
def test_optimizer_class_steps_as_the_op_called_directly(ops, variant):
  """two steps through the class — IndexedSlices, then a DeferredSparseGrad through _native_step and kv_multi_apply_sparse —
  against the op on a twin pair: a 4 D slot of zeros, the beta powers advanced per step, the same rows at the bar"""
  import torch
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import kv_variable_ops as kvo, variable_scope as vs
  vs.reset_default_store()
  kvo.set_training(True)
  D, n, rng = 16, 40, np.random.default_rng(3)
  kv = vs.get_kv_variable("ga4_" + variant, embedding_dim=D, initializer=vs.ones_initializer)
  opt = (training.GroupAMSGradOptimizer if variant == "amsgrad" else training.GroupAdaBeliefOptimizer)(
      LR, epsilon=1e-7, l1_regularization_strength=1e-3, l2_regularization_strength=0.01)
  twin, ids = _pair(ops, D, np.ones((1, D), F)), torch.from_numpy(rng.choice(60, n, replace=False).astype(np.int64)).cuda()
  powers = [F(0.9), F(0.999)]
  for t in (1, 2):
    g = torch.from_numpy(rng.normal(0, 0.1, (n, D)).astype(F)).cuda()
    grad = kvo.IndexedSlices(g, ids, None) if t == 1 else kvo.DeferredSparseGrad(g, ids, torch.arange(n, device="cuda"), None, n, "sum")
    opt.apply_gradients([(grad, kv)])
    _op(ops, variant)(twin[0], twin[1], g, ids.clone(), LR, *powers, *TAIL, 0.0)
    powers = [F(powers[0] * F(0.9)), F(powers[1] * F(0.999))]
  slot = opt.get_slot(kv, "opt").handle
  assert slot.dim == 4 * D and opt._native_step(kv)[0] == "group_" + variant and list(opt._get_beta_accumulators()) == powers
  for got, want in zip(_rows(ops, [kv.handle, slot], ids.cpu()), _rows(ops, twin, ids.cpu())):
    assert want.any() and (np.abs(got - want) <= _bar(want)).all()
