"""kv_lookup_sparse_clip, kv_lookup_sparse_clip_grad, kv_lookup_sparse_zeros_clip (include/kvhip.h) against the chain itself
in torch float64 on the CPU, on the float32 inputs: rows -> x c / max(|x|, c) -> weights -> segment combine; the backward is
torch.autograd through that expression.  Rows are inserted, so their norms are known: 0.25 c .. 4 c, and one zero row.

Forward bound, to first order in u = 2^-24:  |out[s,e] - ref| <= K u sum_j |w_j s_j x_je| / den_s,  K = 2 len_s + D/2 + 8:
any order of the D squares puts D u on q; the square root halves that and adds u (D/2 + 1 on s_j); the division, the factor
multiply and a position's multiply add u each, the accumulator's additions len_s u (D/2 + 4 + len_s); the denominator's sum,
square root and division add len_s + 2; the + 2 covers the second-order terms.
Backward bound:  |values[j,e] - ref| <= (2 D + 10) u |scale_j s_j| (|g_e| + |x_e| sum_k |x_k g_k| / q).  x . g and q are D
terms each in any order (2 D u on their quotient, + u for the division); the product with x_e, the subtraction, the factor
scale_j * s_j and the final multiply add u each: 2 D + 5.  That is NOT the whole first-order worst case: s_j carries its own
D/2 + 2 and, in a weighted mean / sqrtn, scale_j's denominator up to len_s + 2, about 2.5 D + len_s + 9 in all.  The constant
2 D + 10 is the specified one and is kept; it is NOT proven — the test passes because rounding errors do not all line up (a
float32 emulation of the kernel's arithmetic on these inputs stays under a fifth of it).  The Jacobian jumps where |x| = c:
no inserted row sits within c 2^-10 of it (asserted).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tfplus_amd import _lib  # noqa: E402

C, K, U = 1.0, 40, 2.0 ** -24   # max_norm; keys 0 .. K-1 carry the norms, key K is the zero row, key 999 is never inserted
LENS = [0, 1, 3, 4, 5, 0, 70, 2]   # empty, around the 4 rows a lane keeps in flight, one longer than the serving kernel's lane group
CASES = [(D, "mean", True, np.int64) for D in (64, 4, 8, 12, 256, 7, 260, 1024)] + [   # one pass over each axis; 7, 260, 1024: serving only
    (64, "sum", True, np.int64), (64, "sqrtn", True, np.int64), (64, "mean", False, np.int64), (64, "mean", True, np.int32)]


@pytest.fixture(scope="module")
def ops():
  if not torch.cuda.is_available():
    pytest.skip("needs a GPU")
  from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as g
  return g


def _rows(D):
  x = np.random.default_rng(D).standard_normal((K, D))
  x *= (C * 2.0 ** np.linspace(-2, 2, K) / np.linalg.norm(x, axis=1))[:, None]
  rows = np.concatenate([x, np.zeros((1, D))]).astype(np.float32)
  assert (np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - C) > C * 2.0 ** -10).all()
  return rows


def _table(ops, rows):
  h = ops.kv_variable([rows.shape[1]])
  ops.init_kv_variable_v2(h, np.zeros((4, rows.shape[1]), np.float32))
  ops.kv_variable_insert_v2(h, np.arange(K + 1), rows)
  return h


def _case(missing, seed=0):
  rng = np.random.default_rng(seed)
  seg = np.repeat(np.arange(len(LENS)), LENS)
  ids = rng.integers(0, K + 1, seg.size)
  ids[1:5] = [3, K - 2, 3, K]        # a key repeated in a segment, an unclipped and a clipped row side by side, the zero row
  ids[5] = 999 if missing else K - 1
  return ids, seg, rng.uniform(0.1, 2.0, seg.size).astype(np.float32), len(LENS), rng.standard_normal((len(LENS), 1024)).astype(np.float32)


def _ref(rows, ids, seg, w, nseg, combiner, g):
  """float64: out and its bound, values and their bound (docstring above); an empty segment's 0/0 is NaN and is not compared"""
  f64, D = (lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))), rows.shape[1]
  x = f64(rows)[torch.as_tensor(np.where(ids <= K, ids, K))].requires_grad_()   # a key the table lacks reads zeros
  wt, sg = (torch.ones(len(ids), 1, dtype=torch.float64) if w is None else f64(w)[:, None]), torch.as_tensor(seg.astype(np.int64))
  add = lambda v: torch.zeros((nseg, v.shape[1]), dtype=torch.float64).index_add(0, sg, v)
  den = {"sum": torch.ones(nseg, 1, dtype=torch.float64), "mean": add(wt), "sqrtn": add(wt * wt).sqrt()}[combiner]
  y = x * C / torch.clamp(x.norm(dim=1, keepdim=True), min=C) * wt
  out = add(y) / den
  out.backward(f64(g))
  xd, gp, q = x.detach(), f64(g)[sg], (x.detach() ** 2).sum(1, keepdim=True)
  vbound = (wt / den[sg] * C / torch.clamp(q.sqrt(), min=C)).abs() * (gp.abs() + xd.abs() * (xd * gp).abs().sum(1, keepdim=True) / q.clamp(min=1e-300))
  return out.detach(), (2 * f64(LENS)[:, None] + D / 2 + 8) * U * add(y.detach().abs()) / den, x.grad, (2 * D + 10) * U * vbound


def _inside(got, want, bound):
  err, m = (got.detach().cpu().double() - want).abs(), torch.isfinite(want)
  assert bool((err[m] <= bound[m]).all()), float((err[m] / bound[m].clamp(min=1e-300)).max())


@pytest.mark.parametrize("D,combiner,weighted,segdt", CASES)
def test_against_float64(ops, D, combiner, weighted, segdt):
  rows = _rows(D)
  h = _table(ops, rows)
  for training in (False, True)[:1 + (D % 4 == 0 and D <= 256)]:   # serving: a key never inserted; training: every norm is known
    ids, seg, w, nseg, g = _case(not training)
    seg, w, g = seg.astype(segdt), w if weighted else None, g[:, :D]
    out, obound, vals, vbound = _ref(rows, ids, seg, w, nseg, combiner, g)
    got, saved = (ops.kv_variable_lookup_sparse_clip(h, ids, seg, w, nseg, combiner, False, C) if training else
                  (ops.kv_variable_lookup_sparse_zeros_clip(h, ids, seg, w, nseg, combiner, C), None))
    _inside(got, out, obound)
    if training:
      _inside(ops.kv_variable_lookup_sparse_clip_grad(h, g, seg, w, saved, nseg, combiner, C), vals, vbound)


@pytest.mark.parametrize("D,max_norm", [(D, np.inf) for D in (4, 8, 12, 64, 128, 256, 7, 1024)] + [(64, 8 * C), (260, 8 * C)])
def test_nothing_clips_gives_the_unclipped_bits(ops, D, max_norm):
  ha, hb = (_table(ops, _rows(D) / 2) for _ in range(2))   # twins; norms up to 2 c
  ids, seg, w, nseg, g = _case(True)
  bits = lambda t: t.view(torch.int32)
  assert torch.equal(bits(ops.kv_variable_lookup_sparse_zeros_clip(ha, ids, seg, w, nseg, "mean", max_norm)),
                     bits(ops.kv_variable_lookup_sparse_zeros(hb, ids, seg, w, nseg, "mean")))
  if D % 4 == 0 and D <= 256:
    got, saved = ops.kv_variable_lookup_sparse_clip(ha, ids, seg, w, nseg, "mean", True, max_norm)   # (inserts key 999 in both)
    assert torch.equal(bits(got), bits(ops.kv_variable_lookup_sparse(hb, ids, seg, w, nseg, "mean", True)))
    assert torch.equal(bits(ops.kv_variable_lookup_sparse_clip_grad(ha, g[:, :D], seg, w, saved, nseg, "mean", max_norm)),
                       bits(ops.kv_variable_lookup_sparse_grad(hb, g[:, :D], seg, w, nseg, "mean")))
    keys = np.append(np.arange(K + 1), 999)
    assert ops.kv_get_meta(ha, keys) == ops.kv_get_meta(hb, keys) and None not in ops.kv_get_meta(ha, keys)   # frequency words, flags
    assert ops.kv_variable_size_v2(ha) == ops.kv_variable_size_v2(hb) == K + 2


def test_refusals(ops):
  h, h260 = _table(ops, _rows(64)), _table(ops, _rows(260))
  ids, seg, w, nseg, g = _case(False)
  saved, keys = torch.zeros((ids.size, 2), dtype=torch.int32, device="cuda"), np.arange(K + 1)
  before = ops.kv_get_meta(h, keys)
  calls = lambda t, c: (lambda: ops.kv_variable_lookup_sparse_clip(t, ids, seg, w, nseg, "mean", False, c),
                        lambda: ops.kv_variable_lookup_sparse_clip_grad(t, g[:, :t.dim], seg, w, saved, nseg, "mean", c),
                        lambda: ops.kv_variable_lookup_sparse_zeros_clip(t, ids, seg, w, nseg, "mean", c))
  refused = [(_lib.InvalidArgumentError, calls(h, bad)) for bad in (0.0, -1.0, float("nan"))] + [(_lib.UnimplementedError, calls(h260, C)[:2])]
  for err, call in ((e, c) for e, cs in refused for c in cs):
    with pytest.raises(err):
      call()
  assert ops.kv_get_meta(h, keys) == before and ops.kv_variable_size_v2(h) == ops.kv_variable_size_v2(h260) == K + 1
  assert torch.equal(ops.kv_variable_lookup_sparse_clip(h, ids[:0], seg[:0], None, 3, "mean", False, C)[0], torch.zeros(3, 64, device="cuda"))
  got, saved = ops.kv_variable_lookup_sparse_clip(h, ids, seg, w, nseg, "sum", False, C)
  assert torch.equal(ops.kv_variable_lookup_sparse_clip(h, ids, seg, w, nseg, "sum", False, C, save=False)[0], got)   # saved == NULL


def test_python_surface(ops, monkeypatch):
  from tfplus_amd.kv_variable.python.ops import embedding_ops as eo, kv_variable_ops as kvo, variable_scope as vs
  D, (ids, seg, w, nseg, g) = 64, _case(False)
  rows, keys, g = _rows(D), np.arange(K + 1), g[:, :D]
  sparse = lambda v: eo.SparseTensor(np.stack([seg, np.zeros_like(seg)], 1), v, None)
  lookup = lambda v, fused, comb="mean": eo.embedding_lookup_sparse(v, sparse(ids), sparse(w), combiner=comb, max_norm=C, fused_max_norm=fused)
  out, obound, vals, vbound = _ref(rows, ids, seg, w, nseg, "mean", g)
  dense = lambda i, v: torch.zeros(K + 1, D, dtype=torch.float64).index_add(0, torch.as_tensor(i).cpu().reshape(-1), v.detach().cpu().double())
  def step(fused):   # lookup and backward on a fresh variable: the variable, the output, the gradient filed on it per key
    v = kvo.KvVariable(np.zeros((4, D), np.float32), name="clip_%d" % fused)
    ops.kv_variable_insert_v2(v.handle, keys, rows)
    o = lookup(v, fused)
    o.backward(torch.as_tensor(g).to(o.device))
    return v, o.detach().cpu().double(), dense(v._pending_grads[0].indices, v._pending_grads[0].values)
  (vf, of, gf), (vc, oc, gc) = step(True), step(False)
  _inside(of, torch.where(torch.isfinite(out), oc, out), obound)   # against the chain, on a twin variable
  _inside(gf, gc, dense(ids, vbound))
  assert ops.kv_get_meta(vf.handle, keys) == ops.kv_get_meta(vc.handle, keys) and vf.total_count == vc.total_count
  # a table in occurrence-order mode (refused by the op), a dim the training op does not serve and a partitioned variable keep the chain
  vo = kvo.KvVariable(np.ones((4, D), np.float32), name="clip_occ")
  ops.kv_set_deterministic(vo.handle, ops.KV_ORDER_OCCURRENCE)
  torch.testing.assert_close(lookup(vo, True, "sum"), lookup(vo, False, "sum"))
  monkeypatch.setattr(ops, "kv_variable_lookup_sparse_clip", None)
  part = vs.get_kv_variable("clip_part", embedding_dim=16, initializer=vs.ones_initializer(), partitioner=vs.fixed_size_partitioner(2))
  for v in (kvo.KvVariable(np.ones((4, 260), np.float32), name="clip_260"), part):
    torch.testing.assert_close(lookup(v, True, "sum"), lookup(v, False, "sum"))
  monkeypatch.setattr(kvo, "IS_TRAINING", False)   # inference mode: one read-only fused call — no gather-or-zeros, nothing inserted
  monkeypatch.setattr(ops, "kv_variable_gather_or_zeros_v2", None)
  ids[5] = 999
  o = lookup(vf, True)
  _inside(o, *_ref(rows, ids, seg, w, nseg, "mean", g)[:2])
  assert o.grad_fn is None and vf.total_count == vc.total_count and ops.kv_get_meta(vf.handle, [999]) == [None]
