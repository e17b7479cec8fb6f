"""Times one training step — lookup (kv_gather_or_insert_tok) + optimizer apply (_tok) — of FTRL-V2, group FTRL-V2 and
SparseGroupFtrl in one process, the three alternating step by step so that clocks and cache state are shared.  The
batch is configs[1]'s: 1 M Zipf(1.2) ids over 50 M keys, dim 32; the tables are pre-sized and filled by the warm-up, so
the working set lives in HBM (the three move the same bytes per unique key).

  python tools/ftrl_step.py [--steps 20] [--warmup 5] [--keys 50000000] [--batch 1000000] [--dim 32]

Prints one JSON line: median / p90 milliseconds per step of each optimizer and their ratios to SparseGroupFtrl."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import Zipf  # noqa: E402
from tfplus_amd.kv_variable.python.ops import gen_kv_variable_ops as ops  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--keys", type=int, default=50_000_000)
  ap.add_argument("--batch", type=int, default=1_000_000)
  ap.add_argument("--dim", type=int, default=32)
  args = ap.parse_args()
  dev = torch.device("cuda", 0)
  D, N = args.dim, args.batch
  gen = torch.Generator(device=dev).manual_seed(11)
  z = Zipf(args.keys, 1.2, dev)
  pool = [z.sample(N, gen) for _ in range(4)]
  grads = [torch.randn(N, D, device=dev, generator=gen) * 1e-2 for _ in range(4)]
  cap = 4 * N + (1 << 20)

  def triple():
    hs = [ops.kv_variable([D], capacity_hint=cap) for _ in range(3)]
    ops.init_kv_variable_v2(hs[0], torch.randn(64, D, device=dev, generator=gen) * 0.05)
    ops.init_kv_variable_v2(hs[1], torch.full((16, D), 0.1, device=dev))
    ops.init_kv_variable_v2(hs[2], torch.zeros(16, D, device=dev))
    return hs

  hp = (0.05, 1e-3, 1e-2, 1e-2, -0.5)
  runs = {
      "ftrl_v2_tok": (triple(), lambda hs, g, i: ops.kv_variable_sparse_apply_ftrl_v2(*hs, g, i, *hp)),
      "group_ftrl_v2_tok": (triple(), lambda hs, g, i: ops.kv_variable_group_sparse_apply_ftrl_v2(*hs, g, i, *hp)),
      "sparse_group_ftrl_tok": (triple(), lambda hs, g, i: ops.kv_variable_sparse_group_sparse_apply_ftrl_v2(
          *hs, g, i, hp[0], hp[1], hp[2], 1e-3, hp[3], hp[4])),
  }
  times = {k: [] for k in runs}
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  for step in range(args.warmup + args.steps):
    for name, (hs, fn) in runs.items():
      ids, g = pool[step % 4], grads[step % 4]
      ev[0].record()
      ops.kv_variable_gather_or_insert_v2(hs[0], ids)          # the token goes with `ids` to the apply
      fn(hs, g, ids)
      ev[1].record()
      ev[1].synchronize()
      if step >= args.warmup:
        times[name].append(ev[0].elapsed_time(ev[1]))
  med = {k: float(np.median(v)) for k, v in times.items()}
  out = {"batch": N, "dim": D, "keys": args.keys, "zipf": 1.2, "steps": args.steps,
         "ms_median": med, "ms_p90": {k: float(np.percentile(v, 90)) for k, v in times.items()},
         "ratio_to_sparse_group_ftrl": {k: med[k] / med["sparse_group_ftrl_tok"] for k in med}}
  print(json.dumps(out))


if __name__ == "__main__":
  main()
