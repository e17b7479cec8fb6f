"""Group Momentum / group Adadelta (kvhip.h kv_apply_group_momentum / kv_apply_group_adadelta, optimizer code 11) against the
float64 restatement of tests/_group_acc3_ref.py.  The bar is the project's unique-id bar, rtol 1e-6 / atol 1e-7, per block
(accum, linear, m / accum_update, var).  The float32 restatement is run first, on the CPU, over every step of _case() with
NumPy's pairwise row sums and with running sums; a block whose worst error there exceeds the bar is held to twice that worst
(_scales(), computed from the cases, not written down), every other block to the bar itself.
The restatement's worst, pairwise / running sums, in units of the bar (test_restatement_ratios prints them):
  Momentum  accum 0.00 / 0.00, linear 0.26 / 0.26, m 0.24 / 0.24, var 0.10 / 0.23
  nesterov  accum 0.00 / 0.00, linear 0.48 / 0.48, m 0.38 / 0.38, var 0.15 / 0.41
  Adadelta  accum 0.10 / 0.10, linear 0.17 / 0.17, accum_update 0.00 / 0.00, var 0.47 / 2.18
so only Adadelta's var gets a wider bar, 4.36 (running sums at D = 1024: 1 - l21 sqrt(D) / norm cancels at the median threshold).
An MI355X measured, over all dims and forms: Momentum 0.00, 0.26, 0.24, 0.10; nesterov 0.00, 0.48, 0.38, 0.15; Adadelta 0.10,
0.17, 0.00, 0.46.  The issue's scalars are unchanged; adjusted on the CPU: Momentum's init row is drawn at amplitude 0.005, not 0.5 (_case)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_acc3_ref as R  # noqa: E402
import _ranks  # noqa: E402
import test_gpu_group_adam4 as A  # noqa: E402  (its helpers: _bar, _pair, _rows, _flags and the ops fixture)

F, N, FORMS, gpu, ops = np.float32, A.N, A.FORMS, pytest.mark.gpu, A.ops
DIMS = (4, 7, 36, 256, 1024)   # one float4 lane; masked scalar class; K = 2 with masked lanes; largest entry-list dim; sorted K = 4
LR, L1, L2, MOMENTUM, RHO, EPS = 0.05, 1e-3, 0.01, 0.9, 0.95, 1e-6
INIT = {"momentum": 0.005, "nesterov": 0.005, "adadelta": 0.5}   # the init row's amplitude (_case)
BLOCKS = ("accum", "linear", "third", "var")
each = pytest.mark.parametrize("variant", R.VARIANTS)


def _hp(variant, l21):
  """the reference's vector (R.HP_NAMES); Momentum's epsilon is never read"""
  return (LR, RHO if variant == "adadelta" else MOMENTUM, EPS, L1, L2, l21)


def _args(variant, hp):
  """-> the scalars of the named op, in its own order"""
  return hp if variant == "adadelta" else hp[:2] + hp[3:] + (variant == "nesterov",)


def _op(ops, variant, multi=False):
  return getattr(ops, "kv_%s_group_sparse_apply_%s" % ("multi" if multi else "variable", "adadelta" if variant == "adadelta" else "momentum"))


def _clear(norm, hp, D):
  thr = float(F(hp[5])) * np.sqrt(D)
  return np.abs(norm - thr) > 1e-4 * thr


@functools.lru_cache(None)
def _case(variant, D):
  """-> the var's init row, N distinct ids, [(x0, s0, grad, hp)] of steps 1..3 on the float32 restatement's trajectory.  l21 of
  a step = the median of the float32 restatement's row norms over sqrt(D): half the keys take each branch.  Every key starts from the
  SAME init row and Momentum's first linear is g - var / lr: with test_gpu_group_adam4.py's amplitude 0.5 the gradients
  (0.05 x a lognormal scale per key) lie far below |var| / lr = 10, all row norms crowd at one value and a tenth of the keys
  lies at the threshold (the CPU condition below failed), so Momentum's init row is drawn at INIT = 0.005"""
  rng = np.random.default_rng(1000 + D)
  init, ids = (2 * INIT[variant] * rng.uniform(-0.5, 0.5, (1, D))).astype(F), rng.choice(10 ** 6, N, replace=False).astype(np.int64)
  x, s, steps = np.tile(init, (N, 1)), np.zeros((N, 3 * D), F), []
  for t in (1, 2, 3):
    g = (rng.normal(0, 0.05, (N, D)) * rng.lognormal(0, 1, (N, 1))).astype(F)
    hp = _hp(variant, F(np.median(R.step(variant, x, s, g, _hp(variant, 0.0), F)[3]) / np.sqrt(D)))
    steps.append((x, s, g, hp))
    x, s = [a.astype(F) for a in R.step(variant, x, s, g, hp, F)[:2]]
  return init, ids, steps


def _units(got_x, got_s, x64, s64, clear):
  """-> the worst deviation from the float64 step in units of the project bar: BLOCKS' order (the var: clear keys only)"""
  D = x64.shape[1]
  return [float((np.abs(got_s - s64) / A._bar(s64))[:, b * D:(b + 1) * D].max()) for b in range(3)] + \
         [float((np.abs(got_x - x64) / A._bar(x64))[clear].max())]


@functools.lru_cache(None)
def _worst(variant):
  """-> the float32 restatement's worst over all dims and steps, per block, for (pairwise, running) row sums"""
  worst = np.zeros((2, 4))
  for D in DIMS:
    for x0, s0, g, hp in _case(variant, D)[2]:
      x64, s64, _, norm = R.step(variant, x0, s0, g, hp)
      for o, sequential in enumerate((False, True)):
        worst[o] = np.maximum(worst[o], _units(*R.step(variant, x0, s0, g, hp, F, sequential)[:2], x64, s64, _clear(norm, hp, D)))
  return worst


def _scales(variant):
  return [2 * w if w > 1 else 1.0 for w in _worst(variant).max(axis=0)]


@pytest.mark.parametrize("D", DIMS)
@each
def test_chosen_seeds_take_both_branches_within_the_skip_cap(variant, D):
  """(CPU) the reference alone: every step updates some keys and blacklists others; at most 1 % lie at the threshold"""
  for x0, s0, g, hp in _case(variant, D)[2]:
    _, _, upd, norm = R.step(variant, x0, s0, g, hp)
    assert upd.any() and not upd.all() and _clear(norm, hp, D).mean() >= 0.99


@each
def test_restatement_ratios(variant):
  """(CPU) prints the float32 restatement's worst per block in both summation orders and the bars that follow from them"""
  print("group_%s restatement, units of the project bar %s: pairwise %s running %s -> bars %s"
        % ((variant, BLOCKS) + tuple(np.round(w, 2).tolist() for w in _worst(variant)) + (np.round(_scales(variant), 2).tolist(),)))
  assert np.isfinite(_worst(variant)).all()


def _check(ops, hs, variant, ids, x0, s0, g, hp):
  """the pair after one step from rows x0 / s0 against the float64 step, var and all three slot blocks at _scales(); both rows'
  flags exact; keys at the threshold skipped (<= 1 %).  -> the rows the next step starts from"""
  x64, s64, upd, norm = R.step(variant, x0, s0, g, hp)
  clear = _clear(norm, hp, x0.shape[1])
  got_x, got_s = A._rows(ops, hs, ids)
  units = _units(got_x, got_s, x64, s64, clear)
  print("group_%s D %d: accum %.2f linear %.2f third %.2f var %.2f of the project bar" % ((variant, x0.shape[1]) + tuple(units)))
  assert all(u <= s for u, s in zip(units, _scales(variant))), (units, _scales(variant))
  assert not got_x[clear & ~upd].any()
  small = lambda w: ~(np.abs(w) >= 1e-20).any(axis=1)            # UpdateUnderThreshold on the row written
  want = [(not u, bool(not u or b)) for u, b in zip(upd, small(x64))]
  assert [f for f, c in zip(A._flags(ops, hs[0], ids), clear) if c] == [w for w, c in zip(want, clear) if c]
  assert A._flags(ops, hs[1], ids) == [(False, bool(b)) for b in small(s64)]
  return got_x, got_s


@gpu
@pytest.mark.parametrize("D", DIMS)
@each
def test_three_steps_on_distinct_ids_every_form(ops, variant, D):
  import torch
  init, ids_np, steps = _case(variant, D)
  forms = FORMS if D in (4, 36, 256) else FORMS[:3]
  twins = {f: [A._pair(ops, D, init, mult=3) for _ in range(2 if f == "multi" else 1)] for f in forms}
  ids = torch.from_numpy(ids_np).cuda()
  state = {f: [(np.tile(init, (N, 1)), np.zeros((N, 3 * D), F))] * len(pairs) for f, pairs in twins.items()}
  for _, _, g_np, hp in steps:
    g, sc = torch.from_numpy(g_np).cuda(), _args(variant, hp)
    for f, pairs in twins.items():
      for hs in pairs:
        ops.kv_variable_gather_or_insert_v2(hs[0], ids)           # (the lookup whose token _tok takes)
      hs = pairs[0]
      assert f != "tok" or ops._token_for(hs[0], ids) != 0
      if f == "multi":
        _op(ops, variant, True)([p[0] for p in pairs], [p[1] for p in pairs], [g, g], [ids.clone(), ids.clone()], *sc)
      elif f == "sparse":                                         # one-id segments: the segment gradients ARE the rows
        ops.kv_variable_apply_sparse("group_adadelta" if variant == "adadelta" else "group_momentum", hs, sc, g, ids.clone(),
                                     torch.arange(N, device="cuda"), None, N, "sum")
      else:
        kw = {"unique": {"unique_indices": True}, "counted": {"unique_count": torch.tensor([N], device="cuda")}}.get(f, {})
        _op(ops, variant)(hs[0], hs[1], g, ids if f == "tok" else ids.clone(), *sc, **kw)
      state[f] = [_check(ops, p, variant, ids_np, x0, s0, g_np, hp) for p, (x0, s0) in zip(pairs, state[f])]


@gpu
def test_a_step_from_sizeable_state_tells_the_variants_and_the_aliasing_readings(ops):
  """From zeros accum_update stays near epsilon, where atol hides its second term.  Here the var's init row is -0.25 (no sum
  in linear cancels), the slot's accum 0.3 | linear 0.1 | third 0.2 and the gradients lie in [1, 2], D = 8, one _unique step: every block at its bar against the
  reference, whose Adadelta divides by the twice-decayed accum — the once-decayed reading lies thousands of bars away — and
  whose nesterov m is the twice-updated one: not Momentum's"""
  D, ids, got = 8, np.arange(10, 40, dtype=np.int64), {}
  x0, s0 = np.full((ids.size, D), -0.25, F), np.tile(np.repeat(F([0.3, 0.1, 0.2]), D), (ids.size, 1))
  g = np.linspace(1, 2, ids.size * D, dtype=F).reshape(ids.size, D)
  for variant in R.VARIANTS:
    hs, hp = [ops.kv_variable([D]), ops.kv_variable([3 * D])], _hp(variant, 0.0)
    for h, row in zip(hs, (x0[:1], s0[:1])):
      ops.init_kv_variable_v2(h, row)
    _op(ops, variant)(hs[0], hs[1], g, ids, *_args(variant, hp), unique_indices=True)
    x64, s64, upd, _ = R.step(variant, x0, s0, g, hp)
    got[variant] = A._rows(ops, hs, ids)[1][:, 2 * D:]
    units = _units(*A._rows(ops, hs, ids), x64, s64, upd)
    print("group_%s from sizeable state: accum %.2f linear %.2f third %.2f var %.2f of the project bar" % ((variant,) + tuple(units)))
    assert upd.all() and all(u <= s for u, s in zip(units, _scales(variant))), units
  na = s0[:, :D] * RHO + (1 - RHO) * g.astype(np.float64) ** 2
  once = 0.2 * RHO + (1 - RHO) * (0.2 + EPS) * g ** 2 / (na + EPS)
  assert (np.abs(got["adadelta"] - once) > 1000 * A._bar(once)).all() and (got["nesterov"] != got["momentum"]).all()


@gpu
@pytest.mark.parametrize("det", [1, 0])
@each
def test_repeated_ids_equal_the_deduplicated_step(ops, variant, det):
  """One key 300 times among Zipf-like repeats, D = 32, l21 = 0 (no key at the threshold).  Deterministic mode: the bits of
  kv_dedup_segment_sum + _unique.  Default mode: tests/test_gpu_group_adam4.py's bound — the kernel's sum lies within
  dg = (cnt - 1) 2^-24 sum|g| of the exact one, so var and slot may differ from the float64 step at the exact sum by the
  step's change over [gsum - dg, gsum + dg], doubled, plus the bar for the float32 evaluation."""
  rng = np.random.default_rng(7)
  D, hp = 32, _hp(variant, 0.0)
  init = rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  ids = np.concatenate([np.full(300, 5), np.minimum(rng.zipf(1.2, 3000), 10 ** 6), np.arange(100, 1100)]).astype(np.int64)
  rng.shuffle(ids)
  g = rng.normal(0, 0.05, (ids.size, D)).astype(F)
  raw, ded = A._pair(ops, D, init, mult=3), A._pair(ops, D, init, mult=3)
  for hs in (raw, ded):
    ops.kv_set_deterministic(hs[0], det)
  _op(ops, variant)(raw[0], raw[1], g, ids, *_args(variant, hp))
  u, summed, _ = ops.kv_dedup_segment_sum(ded[0], ids, g)
  _op(ops, variant)(ded[0], ded[1], summed, u, *_args(variant, hp), unique_indices=True)
  keys, inv, cnt = np.unique(ids, return_inverse=True, return_counts=True)
  got = [np.concatenate(A._rows(ops, hs, keys), axis=1) for hs in (raw, ded)]
  if det:
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and got[0].any()
    return
  gsum, gabs = np.zeros((keys.size, D)), np.zeros((keys.size, D))
  np.add.at(gsum, inv, g.astype(np.float64))
  np.add.at(gabs, inv, np.abs(g.astype(np.float64)))
  dg = (cnt[:, None] - 1) * 2.0 ** -24 * gabs
  f = lambda gs: np.concatenate(R.step(variant, np.tile(init, (keys.size, 1)), np.zeros((keys.size, 3 * D), F), gs, hp)[:2], axis=1)
  mid = f(gsum)
  bound = 2 * np.maximum(np.abs(f(gsum - dg) - mid), np.abs(f(gsum + dg) - mid)) + A._bar(mid)
  assert all((np.abs(w - mid) <= bound).all() for w in got)


@gpu
def test_refusals_leave_the_tables_empty(ops):
  """every argument error by its word, through the named ops (both promise forms) and the generic entry"""
  import torch
  from tfplus_amd import _lib
  D = 8
  one = np.ones((1, D), F)
  hs, ids, g = A._pair(ops, D, one, mult=3), np.arange(3, dtype=np.int64), np.full((3, D), 0.1, F)
  bad = lambda hp, i, v: hp[:i] + (v,) + hp[i + 1:]
  mo, ad = _hp("momentum", 0.01), _hp("adadelta", 0.01)
  cases = [(v, [hs[0], A._pair(ops, D, one, mult=m)[1]], hp, "opt must be 3x") for v, hp in (("momentum", mo), ("adadelta", ad)) for m in (2, 4)]
  cases += [(v, [hs[0], hs[0]], hp, "same table") for v, hp in (("nesterov", mo), ("adadelta", ad))]
  cases += [(v, hs, bad(hp, i, w), word) for v, hp in (("momentum", mo), ("adadelta", ad))
            for i, w, word in ((0, 0.0, "lr"), (3, -1.0, "l1 "), (4, -1.0, "l2 "), (5, -1.0, "l21 "))]
  cases += [("momentum", hs, bad(mo, 1, 1.0), "momentum"), ("nesterov", hs, bad(mo, 1, -0.1), "momentum"),
            ("adadelta", hs, bad(ad, 1, 1.0), "rho"), ("adadelta", hs, bad(ad, 2, 0.0), "epsilon")]
  for (v, tabs, hp, word), kw in [(c, k) for c in cases for k in ({}, {"unique_indices": True})]:
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      _op(ops, v)(tabs[0], tabs[1], g, ids, *_args(v, hp), **kw)
  bare = ops.kv_variable([3 * D])                                 # never initialised
  with pytest.raises(_lib.FailedPreconditionError):
    _op(ops, "adadelta")(hs[0], bare, g, ids, *ad)
  gids, gd, n1 = torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), torch.tensor([3], device="cuda")
  with pytest.raises(_lib.InvalidArgumentError, match="0 or 1"):   # the wrapper passes a bool: the C entry itself
    _lib.check(_lib.lib().kv_apply_group_momentum_unique(hs[0].ptr, hs[1].ptr, ops._p(gd), ops._p(gids), 3, *mo[:2], *mo[3:], 2,
                                                         ops._stream(hs[0])))
  for vec, word in ((ad, "optimizer 11 reads 7"), (ad + (3.0,), "variant"), (bad(ad, 1, 1.0) + (2.0,), "rho")):
    with pytest.raises(_lib.InvalidArgumentError, match=word):    # the generic entry's own vector
      _lib.check(_lib.lib().kv_apply_unique_counted(hs[0].ptr, 11, hs[1].ptr, None, ops._hp_array(vec, 11), ops._p(gd), ops._p(gids),
                                                    ops._TORCH_KEY[gids.dtype], 3, ops._p(n1), ops._stream(hs[0])))
  torch.cuda.synchronize()
  assert all(int(ops.kv_variable_shape_v2(h)[0]) == 0 and ops.kv_variable_frequency(h) == 0 for h in hs)


@gpu
@each
def test_sharded_apply_takes_code_11(ops, variant):
  """world 2 over staged communicators at D = 8 against one table, at tests/test_gpu_group_adam4.py's tolerance for the same check"""
  import torch
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76)
  D, world, hp = 8, 2, _hp(variant, 0.0)
  init = rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  ref, parts = A._pair(ops, D, init, mult=3), [A._pair(ops, D, init, mult=3) for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
  grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]

  def step(r, comm):
    shs[r].lookup(comm, torch.from_numpy(ids[r]).cuda())
    torch.cuda.synchronize()
    shs[r].apply(comm, ops.OPT_GROUP_ACC3, [parts[r][1]], torch.from_numpy(grads[r]).cuda(),
                 [float(v) for v in hp] + [float(R.VARIANTS.index(variant))])
  ranks = _ranks.Ranks(ops, world)
  ranks.run(step)
  ranks.close()
  ops.kv_variable_gather_or_insert_v2(ref[0], np.concatenate(ids))
  _op(ops, variant)(ref[0], ref[1], np.concatenate(grads), np.concatenate(ids), *_args(variant, hp))
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r in range(world):
    for got, want in zip(A._rows(ops, parts[r], u[own == r]), A._rows(ops, ref, u[own == r])):
      assert want.any()
      np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)


@gpu
@each
def test_two_minimize_steps_of_the_optimizer_class_match_the_reference(ops, variant):
  """loss = sum(lookup(ids) w) twice through minimize() — the lookup's IndexedSlices, each id once — against the float64 step
  from the rows the tables held before it: a 3 D slot of zeros at first, the class's scalars those of the op"""
  import torch
  from tfplus_amd.kv_variable.python import training
  from tfplus_amd.kv_variable.python.ops import embedding_ops as eo, kv_variable_ops as kvo, variable_scope as vs
  vs.reset_default_store()
  kvo.set_training(True)
  D, n, rng = 16, 40, np.random.default_rng(3)
  kv = vs.get_kv_variable("acc3_" + variant, embedding_dim=D, initializer=vs.ones_initializer)
  reg = dict(l1_regularization_strength=L1, l2_regularization_strength=L2)
  opt = training.GroupAdadeltaOptimizer(LR, RHO, EPS, **reg) if variant == "adadelta" else \
      training.GroupMomentumOptimizer(LR, MOMENTUM, use_nesterov=variant == "nesterov", **reg)
  ids = torch.from_numpy(rng.choice(60, n, replace=False).astype(np.int64)).cuda()
  x0, s0, hp = np.ones((n, D), F), np.zeros((n, 3 * D), F), _hp(variant, 0.0)
  for t in (1, 2):
    w = rng.normal(0, 0.1, (n, D)).astype(F)
    opt.minimize((eo.embedding_lookup(kv, ids) * torch.from_numpy(w).cuda()).sum(), var_list=[kv])
    slot = opt.get_slot(kv, "opt").handle
    x64, s64, upd, _ = R.step(variant, x0, s0, w, hp)
    x0, s0 = A._rows(ops, [kv.handle, slot], ids.cpu())
    assert upd.all() and x64.any() and all(u <= s for u, s in zip(_units(x0, s0, x64, s64, upd), _scales(variant)))
  assert slot.dim == 3 * D and opt._native_step(kv)[0] == ("group_adadelta" if variant == "adadelta" else "group_momentum")
