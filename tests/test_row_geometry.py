"""The row-geometry restatement (tests/_row_geometry.py) against the sources, on the CPU: class_of agrees, for every dim,
with what the one dispatch table (tfplus_amd/csrc/kv_row_geom.h) selects — printed by a stand-alone program that includes
the header alone — and every launcher goes through that table; DIMS reaches every class of every pipeline at its edges,
draw_batch meets its occurrence plan for the seeds the GPU module uses, and the LDS a k_apply_fin block needs is within
what its launcher provides at every dim.  A later change to a table fails here until the restatement and the dim list follow."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _row_geometry as G  # noqa: E402

CSRC = os.path.join(HERE, "..", "tfplus_amd", "csrc")
SUPPORTED = [D for D in range(1, 1025) if G.dim_supported(D)]


def _src(name):
  with open(os.path.join(CSRC, name)) as f:
    return f.read()


def _const(text, name):
  m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
  assert m, name
  return int(m.group(1))


def _function(text, head):
  """The definition that starts with `head`, up to its closing brace in column 0."""
  at = text.index(head)
  return text[at:text.index("\n}\n", at) + 3]


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
  """{D: what kv_row_geom.h selects for dim D}, D in 0..1028, as tests/c_abi/row_geom_check.cc prints it: the program
  includes the header alone, is built with the host compiler under AddressSanitizer and UBSan and run directly (no GPU,
  nothing loaded into Python).  "sorted" / "entry": the (V, LPR, K) with_row_geom hands the launcher's lambda, or None."""
  src = os.path.join(HERE, "c_abi", "row_geom_check.cc")
  exe = str(tmp_path_factory.mktemp("row_geom") / "row_geom_check")
  if shutil.which("g++"):
    cmd = ["g++", "-std=c++17", "-fsanitize=address,undefined"]
  else:   # the compiler the library itself needs
    cmd = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined"]
  subprocess.check_call(cmd + ["-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
  r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
  assert r.returncode == 0, r.stdout + r.stderr
  lines = r.stdout.strip().split("\n")
  assert lines[-1] == "ok" and len(lines) == 1030, r.stdout[-2000:] + r.stderr
  cls = lambda w: None if w == "-" else tuple(int(x) for x in w.split(","))
  out = {}
  for D, line in enumerate(lines[:-1]):
    w = line.split()
    assert int(w[0]) == D and len(w) == 9, line
    out[D] = dict(sorted=cls(w[1]), entry=cls(w[2]), fused_ok=bool(int(w[3])), row_lanes=int(w[4]), lanes=int(w[5]),
                  lanes256=int(w[6]), pow2_64=int(w[7]), pow2_256=int(w[8]))
  return out


def test_constants_match_the_headers():
  dev, ker = _src("kv_device.h"), _src("kv_kernels.h")
  assert (_const(dev, "LCOLD"), _const(dev, "HC"), _const(dev, "IPT")) == (G.LCOLD, G.HC, G.IPT)
  assert int(re.search(r"#define KV_TBT (\d+)", dev).group(1)) == G.TBT
  assert re.search(r"constexpr int TILE = TBT \* IPT;", dev)
  assert _const(ker, "TBF") == G.TBF
  assert re.search(r"bool dim_supported\(int D\) \{ return \(D & 3\) == 0 \? D <= 1024 : D <= 256; \}", _src("kvhip.hip"))
  assert all(G.dim_supported(D) for D in G.DIMS) and not any(G.dim_supported(D) for D in G.REFUSED)


def test_class_of_matches_the_sorted_apply_table(selected):
  for D in range(1, 1025):
    assert G.class_of("sorted", D) == selected[D]["sorted"], D
    assert (selected[D]["sorted"] is not None) == G.dim_supported(D), D
  for D in SUPPORTED:
    if selected[D]["sorted"]:
      v, lpr, k = selected[D]["sorted"]
      assert D <= v * lpr * k, D          # the class holds the whole row
  assert all(selected[D]["sorted"] is None for D in (0, 257, 258, 1025, 1028))
  body = _function(_src("kv_kernels.h"), "int launch_apply_t(")
  assert re.search(r"return with_row_geom<SORTED_MAX_Q, true>\(D, \[&\]\(auto g\) -> int \{", body)
  geom = _src("kv_row_geom.h")
  assert _const(geom, "SORTED_MAX_Q") == G._F4[-1][0] and _const(geom, "SCALAR_MAX_D") == G._SC[-1][0]
  # apply_lanes (the cold batch the partition pass forms) states the same lane counts: restated for the device, and held
  # against the table by the compiler
  assert re.search(r"return q <= 1 \? 1 : q <= 2 \? 2 : q <= 4 \? 4 : q <= 16 \? 8 : q <= 32 \? 16 : 64;", geom)
  assert re.search(r"if \(!row_class\(D\)\.none\(\) && apply_lanes\(D\) != row_class\(D\)\.LPR\) return false;", geom)
  assert re.search(r"static_assert\(apply_lanes_match_the_ladders\(\),", geom)
  assert "apply_lanes(a.tv.dim)" in _src("kv_kernels.h")


ENTRY_LAUNCHERS = [("kv_papply.h", "int launch_papply_t("), ("kv_uapply.h", "int launch_uapply_t("),
                   ("kv_sums.hip", "int launch_tsum("), ("kv_sums.hip", "static int launch_ltsum_t("),
                   ("kv_sums.hip", "int launch_papply_ud(")]


@pytest.mark.parametrize("name,head", ENTRY_LAUNCHERS, ids=[h.split()[-1][:-1] for _, h in ENTRY_LAUNCHERS])
def test_class_of_matches_the_entry_list_tables(name, head, selected):
  body = _function(_src(name), head)
  calls = re.findall(r"with_row_geom<([^>]*)>\(", body)
  assert calls == ["ENTRY_MAX_Q"], (head, calls)
  assert _const(_src("kv_row_geom.h"), "ENTRY_MAX_Q") == G._ENTRY_Q
  assert "constexpr bool fused_ok(int D) { return !row_class(D, ENTRY_MAX_Q, false).none(); }" in _src("kv_row_geom.h")
  for D in range(1, 1025):
    assert G.class_of("entry", D) == selected[D]["entry"], D
    assert selected[D]["fused_ok"] == (selected[D]["entry"] is not None) == (D % 4 == 0 and D // 4 <= G._ENTRY_Q), D
    if selected[D]["entry"]:
      assert selected[D]["entry"] == selected[D]["sorted"], D      # one table: the entry family is its float4 rungs to q = 64


def test_no_hand_written_ladder_remains():
  """The table is stated once: no `if (q <= N) KV_XX(V, LPR, K);` ladder, no per-expansion tag struct, no rung outside
  kv_row_geom.h; every rung of the restatement is there once."""
  for name in sorted(os.listdir(CSRC)):
    if not name.endswith((".h", ".hip")):
      continue
    text = _src(name)
    assert not re.search(r"if \((?:q|D) <= \d+\) KV_\w+\(", text), name      # (nc: the occ-sum table, another rule)
    assert not re.search(r"struct \w*Tag \{\}", text), name
    assert ("Rung<" in text) == (name == "kv_row_geom.h"), name
  rungs = [(int(t), (int(v), int(l), int(k)))
           for t, v, l, k in re.findall(r"\bRung<(\d+), (\d+), (\d+), (\d+)>", _src("kv_row_geom.h"))]
  assert rungs == G._F4 + G._SC


def test_class_of_matches_the_row_copy_lanes(selected):
  for D in range(1, 1025):
    q = D // 4
    assert selected[D]["row_lanes"] == G._pow2ceil(max(1, q)), D
    assert selected[D]["lanes"] == min(64, selected[D]["row_lanes"]) and selected[D]["lanes256"] == min(256, selected[D]["row_lanes"]), D
    if D % 4 == 0:
      assert G.class_of("row_copy", D) == selected[D]["lanes"], D
  assert sorted({G.class_of("row_copy", D) for D in SUPPORTED if D % 4 == 0}) == [1, 2, 4, 8, 16, 32, 64]
  # dim 36: 16 lanes in the row copies, 8 lanes x 2 vectors in the apply
  assert G.class_of("row_copy", 36) == 16 and G.class_of("entry", 36) == (4, 8, 2)
  # the default cap adds no instantiation to the callers that name none
  assert re.search(r"template <int CAP = 64, int L = 1, class F>\s*auto with_lanes\(int lanes, F&& f\)", _src("kv_row_geom.h"))
  for name in ("kvhip.hip", "kv_ops.hip", "kv_shard.hip"):
    assert set(re.findall(r"\bwith_lanes(<\w+>)?\(", _src(name))) <= ({"", "<TB>"} if name == "kvhip.hip" else {""}), name


def test_class_of_matches_the_gather_tables(selected):
  hip, ops = _src("kvhip.hip"), _src("kv_ops.hip")
  body = _function(hip, "void launch_gather(")
  assert "const int q = pow2_vectors(D, TB);" in body and _const(_src("kv_device.h"), "TB") == 256
  # a power-of-two q takes its own VQ, every other dim the generic body <0>
  assert re.search(r"if \(q\) with_lanes<TB>\(q, launch\);\s*else launch\(std::integral_constant<int, 0>\{\}\);", body)
  assert "static int sparse_zeros_lanes(int D) { return pow2_vectors(D, 64); }" in ops
  gz = _function(ops, "int kv_gather_or_zeros(")
  assert "const int q = pow2_vectors(t->dim, 64);" in gz
  assert re.search(r"if \(q\)\s*with_lanes\(q, \[&\]\(auto vq\) \{ k_gather_or_zeros_w<", gz)
  for D in range(1, 1025):
    assert G.class_of("gather", D) == selected[D]["pow2_256"], D
    if selected[D]["pow2_256"]:
      assert selected[D]["lanes256"] == selected[D]["pow2_256"], D       # with_lanes<256> hands q itself over
    for p in ("gather_zeros", "sparse_zeros"):
      assert G.class_of(p, D) == selected[D]["pow2_64"], (p, D)
    if selected[D]["pow2_64"]:
      assert selected[D]["lanes"] == selected[D]["pow2_64"], D
  assert sorted({G.class_of("gather", D) for D in SUPPORTED}) == [0, 1, 2, 4, 8, 16, 32, 64, 128, 256]
  for p in ("gather_zeros", "sparse_zeros"):
    assert sorted({G.class_of(p, D) for D in SUPPORTED}) == [0, 1, 2, 4, 8, 16, 32, 64]


def test_class_of_matches_the_occ_sum_table():
  hip = _src("kvhip.hip")
  body = hip[hip.index("int launch_occ_sum("):hip.index("#undef KV_OCC")]
  assert "const int nc = (D + 63) / 64;" in body
  tops = [(int(a), int(b)) for a, b in re.findall(r"if \(nc <= (\d+)\) KV_OCC\((\d+)\);", body)]
  last = int(re.search(r"else KV_OCC\((\d+)\);", body).group(1))
  assert [b for _, b in tops] + [last] == G._OCC and all(a == b for a, b in tops)
  assert 64 * last >= 1024


@pytest.mark.parametrize("pipeline", G.PIPELINES)
def test_dims_reach_every_class_at_its_edges(pipeline):
  members = {}
  for D in SUPPORTED:
    members.setdefault(G.class_of(pipeline, D), []).append(D)
  members.pop(None, None)
  assert len(members) > 1
  for cls, ds in members.items():
    assert ds[0] in G.DIMS and ds[-1] in G.DIMS, (pipeline, cls, ds[0], ds[-1])
    if any(G.masked(pipeline, D) for D in ds):
      assert any(G.masked(pipeline, D) for D in ds if D in G.DIMS), (pipeline, cls)
    if any(not G.masked(pipeline, D) for D in ds) and G.width_of(pipeline, ds[0]) is not None:
      assert any(not G.masked(pipeline, D) for D in ds if D in G.DIMS), (pipeline, cls)      # ... and a full row


def test_dims_list():
  assert G.DIMS == sorted(set(G.DIMS)) and 35 <= len(G.DIMS) <= 40
  assert 572 in G.DIMS and 576 in G.DIMS          # either side of the LDS a launch gets without asking


@pytest.mark.parametrize("seed", G.SEEDS)
@pytest.mark.parametrize("kd", [np.int64, np.int32])
def test_batch_meets_its_occurrence_plan(seed, kd):
  b = G.draw_batch(np.random.default_rng(seed), kd)
  ids, keys, counts = b["ids"], b["keys"], b["counts"]
  assert ids.dtype == kd and G.TILE < ids.size <= G.TILE + 256 and 140 <= keys.size <= 160
  u, c = np.unique(ids, return_counts=True)
  assert np.array_equal(u, np.sort(keys)) and np.array_equal(c, counts[np.argsort(keys)])
  have = set(c.tolist())
  assert {1, 2, 3, 4, G.LCOLD, G.LCOLD + 1, G.HC, G.HC + 1, 300} <= have      # cold lists, hot in one chunk, in several
  assert sum(1 for x in c if x > G.HC) >= 2
  at = np.flatnonzero(ids == b["span"])
  assert at[0] < G.TILE <= at[-1]                                              # one key in both tiles
  assert any((np.flatnonzero(ids == k) >= G.TILE).all() for k in u)            # ... and one in the second tile alone
  assert (keys < 0).any() and (keys > 0).any()
  if kd == np.int64:
    assert (np.abs(keys.astype(np.int64)) > 1 << 32).sum() >= keys.size // 8
  pu, pc = np.unique(b["pre"], return_counts=True)
  assert set(pu.tolist()) | set(b["new"].tolist()) == set(keys.tolist()) and not set(pu.tolist()) & set(b["new"].tolist())
  assert abs(pu.size - b["new"].size) <= 1 and (pc == 1).any() and (pc == 2).any()   # enter_threshold 2: below and at it


@pytest.mark.parametrize("seed", G.SEEDS)
def test_repeated_ids_sum_exactly_in_every_order(seed):
  rng = np.random.default_rng(seed)
  b = G.draw_batch(rng)
  g = G.draw_grads(rng, b, 5)
  for k, c in zip(b["keys"], b["counts"]):
    rows = g[b["ids"] == k]
    if c == 1:
      continue
    fwd = np.zeros(5, np.float32)
    for r in rows:
      fwd = fwd + r
    assert np.array_equal(fwd, rows.astype(np.float64).sum(0).astype(np.float32))
    assert np.array_equal(rows[::-1].cumsum(0, dtype=np.float32)[-1], fwd)
  once = g[np.isin(b["ids"], b["keys"][b["counts"] == 1])]
  assert (np.frexp(once)[0] * 2.0 ** 24 % 2 != 0).mean() > 0.3                 # full mantissas


def test_apply_fin_lds_fits_at_every_dim():
  """k_apply_fin's block: static lkeys[TBF][7] + lnk, dynamic lsum[TBF / 64][D].  Within LDS_NO_ASK a launch just gets it;
  above (dims 576..1024) launch_apply_t asks for the dynamic part before the launch, and the sum stays within a CU's LDS."""
  ker = _src("kv_kernels.h")
  assert re.search(r"__shared__ unsigned lkeys\[TBF\]\[7\];", ker) and re.search(r"__shared__ unsigned lnk;", ker)
  assert "constexpr size_t FIN_STATIC_LDS = (size_t)TBF * 7 * 4 + 16;" in ker
  assert "constexpr size_t LDS_NO_ASK = 64 * 1024;" in ker
  assert "inline size_t fin_dyn_lds(int D) { return (size_t)(TBF / 64) * D * 4 + 16; }" in ker
  body = ker[ker.index("int launch_apply_t("):]
  assert "const size_t sh = span == 1 ? fin_dyn_lds(D) : 0;" in body
  ask = re.search(r"if \(span == 1 && sh \+ FIN_STATIC_LDS > LDS_NO_ASK\) \{.*?hipFuncSetAttribute\(fin_kernel<MODE, OPT, V, LPR, K>"
                  r"\(md != nullptr\), hipFuncAttributeMaxDynamicSharedMemorySize,\s*\\?\s*\(int\)sh\) != hipSuccess\)", body, re.S)
  assert ask, "launch_apply_t no longer asks for k_apply_fin's LDS"
  asked = []
  for D in G.DIMS:
    st, dyn = G.fin_lds_bytes(D)
    assert st >= G.TBF * 7 * 4 + 4
    assert st + dyn <= G.LDS_PER_CU, D
    if st + dyn > G.LDS_NO_ASK:
      asked.append(D)
  assert asked == [576, 1020, 1024]
  assert sum(G.fin_lds_bytes(572)) <= G.LDS_NO_ASK < sum(G.fin_lds_bytes(576))


# ---- the optimizer cases' reference trajectories (tests/_row_geometry.py trajectory), on the reference alone ----------------
@pytest.mark.parametrize("family", G.GROUP_FAMILIES + ("ftrl_v2",))
def test_reference_trajectories_meet_their_conditions(family):
  """For every dim: the regularizers put some rows on either side of the decision at every step, at least 99 % of the keys
  are compared (no row's scale within 1e-4 of the threshold), some keys stay below the enter threshold at the first step,
  and the float32 reference's own distance from the float64 step — what a widened bar rests on — is printed per dim."""
  line = []
  for D in G.DIMS:
    tr = G.trajectory(family, D)
    worst = 0.0
    for t, st in enumerate(tr["steps"]):
      n_live = int(st["live"].sum())
      assert st["clear"].mean() >= 0.99, (family, D, t)
      if family in G.GROUP_FAMILIES:
        assert 0 < int(st["black"].sum()) < n_live, (family, D, t)
      else:
        assert 0 < st["zeros"][0] < st["zeros"][1], (family, D, t)
      assert (n_live < st["live"].size) == (t == 0), (family, D, t)
      assert np.isfinite(st["ref_err"]) and (st["widen"] >= 1.0).all() and st["widen"].shape == (st["live"].size, 1)
      assert st["widen"][st["clear"]].max() == max(1.0, 4.0 * st["ref_err"])
      for tb in st["tables"]:
        assert np.isfinite(tb["rows"]).all() and np.isfinite(tb["tol"]).all() and (tb["tol"] >= 0).all()
      worst = max(worst, st["ref_err"])
    line.append("%d: %.3g" % (D, worst))
  print("%s ref_err per dim (units of the bar): %s" % (family, ", ".join(line)))
