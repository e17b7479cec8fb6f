"""Times what an unchanged reference graph runs per step — complete lookup (no batch token), TF-core's de-duplication
(kv_dedup_segment_sum), the optimizer op on unique ids (GroupAdam V4) — in its two forms, in one process:

  sync     kv_dedup_segment_sum returns the count to the host (one stream drain per step) + kv_apply_group_adam_unique
  counted  kv_dedup_segment_sum_dev leaves the count on the device + kv_apply_unique_counted reads it there

at bench.py's `unchanged_graph` shape (1 M Zipf(1.2) ids over 50 M keys, dim 32), each form on its own pre-sized table
pair.  The forms alternate block by block (a block = `--block` steps issued back to back, one synchronisation at its end)
so that clocks and cache state are shared; a form's figure is the median over the blocks of the block's time per step.  The
spread of the sync form between its own blocks is printed with it: a difference between the forms inside it says nothing.
Host time per step is the time the host spends inside the three calls (for the sync form that includes the drain).

  python tools/unchanged_chain.py [--blocks 15] [--block 20] [--warmup 3] [--keys 50000000] [--batch 1000000] [--dim 32]
                                  [--capacity 33554432]

The counted form advances the host's row bounds by the batch length per call (kvhip.h): --capacity is what keeps the count
refreshes (one synchronisation each) rare.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import Zipf  # noqa: E402
from tfplus_amd import _lib  # noqa: E402
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--blocks", type=int, default=15)
  ap.add_argument("--block", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--keys", type=int, default=50_000_000)
  ap.add_argument("--batch", type=int, default=1_000_000)
  ap.add_argument("--dim", type=int, default=32)
  ap.add_argument("--capacity", type=int, default=1 << 25)
  args = ap.parse_args()
  dev = torch.device("cuda", 0)
  D, N = args.dim, args.batch
  L = _lib.lib()
  gen = torch.Generator(device=dev).manual_seed(11)
  z = Zipf(args.keys, 1.2, dev)
  pool = [(z.sample(N, gen), torch.randn(N, D, device=dev, generator=gen) * 1e-2) for _ in range(4)]
  uniq = float(np.mean([int(torch.unique(p[0]).numel()) for p in pool]))
  out = torch.empty((N, D), dtype=torch.float32, device=dev)
  adam = (1e-3, 0.9, 0.999, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)

  def pair():
    hs = [ops.kv_variable([D], capacity_hint=args.capacity), ops.kv_variable([3 * D], capacity_hint=args.capacity)]
    ops.init_kv_variable_v2(hs[0], torch.randn(64, D, device=dev, generator=gen) * 0.05)
    ops.init_kv_variable_v2(hs[1], torch.zeros(16, 3 * D, device=dev))
    return hs

  def lookup(hs, ids):   # the complete lookup: no token is asked for
    _lib.check(L.kv_gather_or_insert_tok(hs[0].ptr, ids.data_ptr(), None, ids.numel(), out.data_ptr(), None,
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

  def sync_step(hs, ids, grad):
    lookup(hs, ids)
    u, s, _ = ops.kv_dedup_segment_sum(hs[0], ids, grad)
    ops.kv_variable_group_sparse_apply_adam_v4(hs[0], hs[1], s, u, *adam, unique_indices=True)

  def counted_step(hs, ids, grad):
    lookup(hs, ids)
    u, s, _, nu = ops.kv_dedup_segment_sum(hs[0], ids, grad, sync=False)
    ops.kv_variable_group_sparse_apply_adam_v4(hs[0], hs[1], s, u, *adam, unique_count=nu)

  forms = {"sync": (pair(), sync_step), "counted": (pair(), counted_step)}
  ms = {k: [] for k in forms}
  host = {k: [] for k in forms}
  k = 0
  for b in range(args.warmup + args.blocks):
    for name, (hs, step) in forms.items():
      torch.cuda.synchronize()
      spent = 0.0
      t0 = time.perf_counter()
      for i in range(args.block):
        ids, grad = pool[(k + i) % len(pool)]
        h0 = time.perf_counter()
        step(hs, ids, grad)
        spent += time.perf_counter() - h0
      torch.cuda.synchronize()
      if b >= args.warmup:
        ms[name].append((time.perf_counter() - t0) / args.block * 1e3)
        host[name].append(spent / args.block * 1e3)
    k += args.block
  med = {n: float(np.median(v)) for n, v in ms.items()}
  res = {"batch": N, "dim": D, "keys": args.keys, "zipf": 1.2, "unique_ids_mean": uniq, "blocks": args.blocks,
         "steps_per_block": args.block, "capacity": args.capacity,
         "ms_per_step_median": med,
         "ms_per_step_min_max": {n: [float(np.min(v)), float(np.max(v))] for n, v in ms.items()},
         "sync_spread_ms": float(np.max(ms["sync"]) - np.min(ms["sync"])),
         "sync_p10_p90_ms": [float(np.percentile(ms["sync"], 10)), float(np.percentile(ms["sync"], 90))],
         "host_ms_per_step_median": {n: float(np.median(v)) for n, v in host.items()},
         "counted_over_sync": med["counted"] / med["sync"]}
  print(json.dumps(res))


if __name__ == "__main__":
  main()
