"""The read-only sharded lookup against the training one and against the plain gather, at world 1 (a communicator of one rank
without RCCL: every phase but the wire), one filled table of dim 32, a Zipf(1.2) batch of 1 M ids.  Times, per step:
  (a) kv_shard_lookup_zeros             route -> [records] -> k_shard_serve_zeros -> [rows] -> finish
  (b) kv_shard_lookup                   the training lookup, on a second, identical shard (its serve: tile pass + partition pass)
  (c) kv_gather_or_zeros                over the same ids on the local table: the bytes reference (it writes the [n, dim] rows)
and for (a) and (b) the serve phase alone, through the phase calls and event pairs around it (route and exchange run once per
sample, outside the events; the training serve defers its partition pass to the table's next op, here the next sample's
serve, so that pass is inside the events too, one sample late).  Expectation, checked at the end: (a)'s serve is below (b)'s — one probe-and-copy launch over the
distinct records against a tile pass plus a partition pass.  python tools/shard_zeros_time.py [other.so]"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfplus_amd import _lib
if len(sys.argv) > 1:
  _lib.SO_PATH = os.path.abspath(sys.argv[1])
import bench
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)
KEYS, N, D = 2_000_000, 1 << 20, 32

init = torch.randn(256, D, device=dev, generator=g)


def make():
  h = ops.kv_variable([D], capacity_hint=KEYS + 1024)
  ops.kv_set_seed(h, 3)
  ops.init_kv_variable_v2(h, init)
  for j in range(0, KEYS, 1 << 20):
    ops.kv_variable_gather_or_insert_v2(h, torch.arange(j, min(j + (1 << 20), KEYS), device=dev))
  return h, ops.KvShard(h, 1, 0, max_ids=N)


def timed(fn, reps):
  for _ in range(3): fn()
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(reps): fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e6


def serve_alone(sh, serve, reps):
  """the serve phase between event pairs; its route and the exchange of the records run outside them"""
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
  for k in range(-3, reps):
    sh.lookup_route(ids)
    ops.kv_shard_exchange_local([sh], 0)
    if k >= 0: ev[k][0].record()
    serve()
    if k >= 0: ev[k][1].record()
  torch.cuda.synchronize()
  ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
  return ts[len(ts) // 2], ts[0]


(ha, sa), (hb, sb) = make(), make()
comm = ops.KvComm(1, 0, None)
ids = bench.Zipf(KEYS, 1.2, dev).sample(N, g) - 1
uniq = int(torch.unique(ids).numel())
# the three paths return the same rows (every id is held: the training lookup inserts nothing)
want = ops.kv_variable_gather_or_zeros_v2(ha, ids)
assert torch.equal(sa.lookup_zeros(comm, ids), want) and torch.equal(sb.lookup(comm, ids), want)
print("world 1, no RCCL; one table of %d keys, dim %d; %d ids, Zipf(1.2): %d distinct (the serve's live records); peer capacity %d"
      % (KEYS, D, N, uniq, sa.peer_capacity))
runs = (("(a) kv_shard_lookup_zeros", lambda: sa.lookup_zeros(comm, ids)),
        ("(b) kv_shard_lookup (training)", lambda: sb.lookup(comm, ids)),
        ("(c) kv_gather_or_zeros", lambda: ops.kv_variable_gather_or_zeros_v2(ha, ids)))
best = {}
for rnd in range(3):                                     # the paths alternate: three rounds each
  for name, fn in runs:
    t = timed(fn, 50)
    best[name] = min(best.get(name, t), t)
    print("  round %d  %-32s %9.1f us per step" % (rnd, name, t))
serves = {}
for rnd in range(3):
  for name, sh, serve in (("(a) serve: k_shard_serve_zeros", sa, sa.lookup_serve_zeros), ("(b) serve: training lookup", sb, sb.lookup_serve)):
    med, lo = serve_alone(sh, serve, 30)
    serves[name] = min(serves.get(name, med), med)
    print("  round %d  %-32s %9.1f us median of 30 (least %.1f), events around the phase" % (rnd, name, med, lo))
ta, tb, tc = (best[r[0]] for r in runs)
va, vb = serves["(a) serve: k_shard_serve_zeros"], serves["(b) serve: training lookup"]
print("  best of 3: (a) %.1f us, (b) %.1f us, (c) %.1f us per step; serve alone (a) %.1f us, (b) %.1f us, (b) / (a) = %.2fx"
      % (ta, tb, tc, va, vb, vb / va))
print("expectation ((a)'s serve below (b)'s serve): %s" % ("MET" if va < vb else "NOT MET"))
del comm
sys.exit(0 if va < vb else 1)
