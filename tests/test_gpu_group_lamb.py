"""Group LAMB (kvhip.h kv_apply_group_lamb, optimizer code 10) against the float64 restatement of tests/_group_lamb_ref.py.
m, v and accum depend on no sum: the project's unique-id bar, rtol 1e-6 / atol 1e-7.  linear and the var carry the trust ratio,
a quotient of two float32 sums of D squares, and the kernel sums in an order of its own (lane partials, then a butterfly).
Their bar comes from the restatement's own error: the float32 restatement, run over every step of _case() with NumPy's pairwise
sums and with running sums, lies within 0.48 / 0.96 (linear) and 1.01 / 1.88 (var) of the project bar; the third order gets twice
the worst, so linear is held to 1.91 and the var to 3.75 times the bar (_scales(), computed from the cases, not written down).
An MI355X measured at most 0.48 of the project bar on linear, 0.67 on the var and 0.14 on m, v and accum, over all dims and forms."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_lamb_ref as R  # noqa: E402
import _ranks  # noqa: E402
import test_gpu_group_adam4 as A  # noqa: E402  (its helpers: _hp, _bar, _clear, _pair, _rows, _flags and the ops fixture)

F, N, FORMS, gpu, ops = np.float32, A.N, A.FORMS, pytest.mark.gpu, A.ops
DIMS = (4, 7, 36, 256, 1024)   # one float4 lane; masked scalar class; K = 2 with masked lanes; largest entry-list dim; sorted K = 4


@functools.lru_cache(None)
def _case(D):
  """-> the var's init row, N distinct ids, [(x0, s0, grad, hp)] of steps 1..3 on the float32 restatement's trajectory.  l21 of
  a step = the median of the reference's own row norms over sqrt(D): half the keys take each branch"""
  rng = np.random.default_rng(1000 + D)
  init, ids = rng.uniform(-0.5, 0.5, (1, D)).astype(F), rng.choice(10 ** 6, N, replace=False).astype(np.int64)
  x, s, steps = np.tile(init, (N, 1)), np.zeros((N, 4 * D), F), []
  for t in (1, 2, 3):
    g = (rng.normal(0, 0.05, (N, D)) * rng.lognormal(0, 1, (N, 1))).astype(F)
    hp = A._hp(t, F(np.median(R.step(x, s, g, A._hp(t, 0.0), F)[3]) / np.sqrt(D)))
    steps.append((x, s, g, hp))
    x, s = [a.astype(F) for a in R.step(x, s, g, hp, F)[:2]]
  return init, ids, steps


def _units(got_x, got_s, x64, s64, clear):
  """-> the worst deviation from the float64 step in units of the project bar: [m, v, linear, accum, var (clear keys only)]"""
  D = x64.shape[1]
  return [float((np.abs(got_s - s64) / A._bar(s64))[:, b * D:(b + 1) * D].max()) for b in range(4)] + \
         [float((np.abs(got_x - x64) / A._bar(x64))[clear].max())]


@functools.lru_cache(None)
def _scales():
  """-> the bars of [m, v, linear, accum, var] in units of the project bar: 1, and for linear and the var twice the float32
  restatement's worst over both summation orders where that exceeds 1"""
  worst = np.zeros(5)
  for D in DIMS:
    for x0, s0, g, hp in _case(D)[2]:
      x64, s64, _, norm, _ = R.step(x0, s0, g, hp)
      for sequential in (False, True):
        worst = np.maximum(worst, _units(*R.step(x0, s0, g, hp, F, sequential)[:2], x64, s64, A._clear(norm, hp, D)))
  return [1.0, 1.0, max(1.0, 2 * worst[2]), 1.0, max(1.0, 2 * worst[4])]


@pytest.mark.parametrize("D", DIMS)
def test_chosen_seeds_reach_both_branches_and_the_unit_ratio(D):
  """(CPU) the reference alone: every step updates some keys and blacklists others, at most 1 % lie at the threshold, and
  from step 2 on rows blacklisted before enter as zeros and take ratio 1"""
  for t, (x0, s0, g, hp) in enumerate(_case(D)[2]):
    _, _, upd, norm, ratio = R.step(x0, s0, g, hp)
    assert upd.any() and not upd.all() and A._clear(norm, hp, D).mean() >= 0.99
    zero = ~x0.any(axis=1)
    assert (ratio[zero] == 1).all() and (ratio[~zero] != 1).all() and zero.any() == (t > 0)


def _check(ops, hs, ids, x0, s0, g, hp):
  """the pair after one step from rows x0 / s0 against the float64 step, var and all four slot blocks at _scales(); both rows'
  flags exact; keys at the threshold skipped (<= 1 %).  -> the rows the next step starts from"""
  x64, s64, upd, norm, _ = R.step(x0, s0, g, hp)
  clear = A._clear(norm, hp, x0.shape[1])
  got_x, got_s = A._rows(ops, hs, ids)
  units = _units(got_x, got_s, x64, s64, clear)
  print("group_lamb D %d: m %.2f v %.2f linear %.2f accum %.2f var %.2f of the project bar" % ((x0.shape[1],) + tuple(units)))
  assert all(u <= s for u, s in zip(units, _scales())), (units, _scales())
  assert not got_x[clear & ~upd].any()
  small = lambda w: ~(np.abs(w) >= 1e-20).any(axis=1)            # UpdateUnderThreshold on the row written
  want = [(not u, bool(not u or b)) for u, b in zip(upd, small(x64))]
  assert [f for f, c in zip(A._flags(ops, hs[0], ids), clear) if c] == [w for w, c in zip(want, clear) if c]
  assert A._flags(ops, hs[1], ids) == [(False, bool(b)) for b in small(s64)]
  return got_x, got_s


@gpu
@pytest.mark.parametrize("D", DIMS)
def test_three_steps_on_distinct_ids_every_form(ops, D):
  import torch
  init, ids_np, steps = _case(D)
  forms = FORMS if D in (4, 36, 256) else FORMS[:3]
  twins = {f: [A._pair(ops, D, init) for _ in range(2 if f == "multi" else 1)] for f in forms}
  ids = torch.from_numpy(ids_np).cuda()
  state = {f: [(np.tile(init, (N, 1)), np.zeros((N, 4 * D), F))] * len(pairs) for f, pairs in twins.items()}
  for _, _, g_np, hp in steps:
    g = torch.from_numpy(g_np).cuda()
    for f, pairs in twins.items():
      for hs in pairs:
        ops.kv_variable_gather_or_insert_v2(hs[0], ids)           # (the lookup whose token _tok takes)
      hs = pairs[0]
      assert f != "tok" or ops._token_for(hs[0], ids) != 0
      if f == "multi":
        ops.kv_multi_group_sparse_apply_lamb([p[0] for p in pairs], [p[1] for p in pairs], [g, g], [ids.clone(), ids.clone()], *hp)
      elif f == "sparse":                                         # one-id segments: the segment gradients ARE the rows
        ops.kv_variable_apply_sparse("group_lamb", hs, hp, g, ids.clone(), torch.arange(N, device="cuda"), None, N, "sum")
      else:
        kw = {"unique": {"unique_indices": True}, "counted": {"unique_count": torch.tensor([N], device="cuda")}}.get(f, {})
        ops.kv_variable_group_sparse_apply_lamb(hs[0], hs[1], g, ids if f == "tok" else ids.clone(), *hp, **kw)
      state[f] = [_check(ops, p, ids_np, x0, s0, g_np, hp) for p, (x0, s0) in zip(pairs, state[f])]


@gpu
@pytest.mark.parametrize("case", ["zero_var", "zero_grad", "both_norms"])
def test_the_ratio_takes_its_branch_exactly(ops, case):
  """D = 8.  A var row of zeros, or a zero gradient on zero m, gives ratio 1: no sum enters linear, which is then the float32
  restatement's bit for bit.  Both norms positive: the ratio is not 1 and linear holds its bar"""
  rng = np.random.default_rng(11)
  D, ids, hp = 8, np.arange(10, 40, dtype=np.int64), A._hp(1, 0.0)
  init = np.zeros((1, D), F) if case == "zero_var" else rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  g = np.zeros((ids.size, D), F) if case == "zero_grad" else rng.normal(0, 0.05, (ids.size, D)).astype(F)
  hs = A._pair(ops, D, init)
  x0, s0 = np.tile(init, (ids.size, 1)), np.zeros((ids.size, 4 * D), F)     # the rows the op inserts
  ops.kv_variable_group_sparse_apply_lamb(hs[0], hs[1], g, ids, *hp, unique_indices=True)
  lin = slice(2 * D, 3 * D)
  got, (_, s64, _, _, ratio), s32 = A._rows(ops, hs, ids)[1][:, lin], R.step(x0, s0, g, hp), R.step(x0, s0, g, hp, F)[1]
  assert (np.abs(got - s64[:, lin]) <= _scales()[2] * A._bar(s64[:, lin])).all()
  if case == "both_norms":
    assert (ratio != 1).all() and got.any()
  else:
    assert (ratio == 1).all() and np.array_equal(got.view(np.uint32), s32[:, lin].view(np.uint32)) and got.any() == (case == "zero_var")


@gpu
def test_repeated_ids_in_deterministic_mode_equal_the_deduplicated_step(ops):
  """One key 300 times among Zipf-like repeats, D = 32: the bits of kv_dedup_segment_sum + _unique on twin tables — code 9's
  test body, which names the op by its stem and, in deterministic mode, compares the twins and consults no reference"""
  A.test_repeated_ids_equal_the_deduplicated_step(ops, "lamb", 1)


@gpu
def test_refusals_leave_the_tables_empty(ops):
  import torch
  from tfplus_amd import _lib
  D, hp = 8, A._hp(1, 0.01)
  hs, ids, g = A._pair(ops, D, np.ones((1, D), F)), np.arange(3, dtype=np.int64), np.full((3, D), 0.1, F)
  bad = lambda i, v: hp[:i] + (v,) + hp[i + 1:]
  cases = [([hs[0], A._pair(ops, D, np.ones((1, D), F), mult=3)[1]], hp, "opt must be 4x"),
           ([hs[0], A._pair(ops, D, np.ones((1, D), F), mult=5)[1]], hp, "opt must be 4x"),
           ([hs[0], hs[0]], hp, "same table"), (hs, bad(0, 0.0), "lr"), (hs, bad(1, 1.0), "beta1_power")]
  for (tabs, h, word), kw in [(c, k) for c in cases for k in ({}, {"unique_indices": True})]:
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      ops.kv_variable_group_sparse_apply_lamb(tabs[0], tabs[1], g, ids, *h, **kw)
  gids, gd, n1 = torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda(), torch.tensor([3], device="cuda")
  for code, vec, word in ((9, hp, "optimizer 9 reads 10"), (10, hp[:8], "optimizer 10 reads 9")):   # the generic entry's own vector
    with pytest.raises(_lib.InvalidArgumentError, match=word):
      _lib.check(_lib.lib().kv_apply_unique_counted(hs[0].ptr, code, hs[1].ptr, None, ops._hp_array(vec, code), ops._p(gd),
                                                    ops._p(gids), ops._TORCH_KEY[gids.dtype], 3, ops._p(n1), ops._stream(hs[0])))
  torch.cuda.synchronize()
  assert all(int(ops.kv_variable_shape_v2(h)[0]) == 0 and ops.kv_variable_frequency(h) == 0 for h in hs)


@gpu
def test_sharded_apply_takes_code_10(ops):
  """world 2 over staged communicators at D = 8 against one table, at tests/test_gpu_group_adam4.py's tolerance for the same check"""
  import torch
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(76)
  D, world, hp = 8, 2, A._hp(1, 0.0)
  init = rng.uniform(-0.5, 0.5, (1, D)).astype(F)
  ref, parts = A._pair(ops, D, init), [A._pair(ops, D, init) for _ in range(world)]
  shs = [ops.KvShard(parts[r][0], world, r, ops.KV_OWNER_HASH, max_ids=1 << 14) for r in range(world)]
  ids = [rng.integers(-100, 1500, 700 + 50 * r).astype(np.int64) for r in range(world)]
  grads = [rng.normal(0, 1e-2, (i.size, D)).astype(F) for i in ids]

  def step(r, comm):
    shs[r].lookup(comm, torch.from_numpy(ids[r]).cuda())
    torch.cuda.synchronize()
    shs[r].apply(comm, ops.OPT_GROUP_LAMB, [parts[r][1]], torch.from_numpy(grads[r]).cuda(), [float(v) for v in hp])
  ranks = _ranks.Ranks(ops, world)
  ranks.run(step)
  ranks.close()
  ops.kv_variable_gather_or_insert_v2(ref[0], np.concatenate(ids))
  ops.kv_variable_group_sparse_apply_lamb(ref[0], ref[1], np.concatenate(grads), np.concatenate(ids), *hp)
  u = np.unique(np.concatenate(ids))
  own = sharded.owner_of(torch.from_numpy(u), world, "hash").numpy()
  for r in range(world):
    for got, want in zip(A._rows(ops, parts[r], u[own == r]), A._rows(ops, ref, u[own == r])):
      assert want.any()
      np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
