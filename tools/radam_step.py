"""Times one training step — lookup (kv_gather_or_insert_tok) + optimizer apply (_tok) — of group RectifiedAdam beside
GroupAdam V3 in one process, the two alternating step by step on the same ids so that clocks and cache state are shared.
The batch is configs[1]'s: 1 M Zipf(1.2) ids over 50 M keys, dim 32; the tables are pre-sized and filled by the warm-up,
so the working set lives in HBM.  Algorithmic bytes of the token apply: GroupAdam's with the slot terms at
5 D instead of 3 D, N (8 + 4 D) + U (16 + 6 * 4 D) + U * 6 * 4 D; GroupAdam V3: N (8 + 4 D) + U (16 + 4 * 4 D) + U * 4 * 4 D.

  python tools/radam_step.py [--steps 20] [--warmup 5] [--keys 50000000] [--batch 1000000] [--dim 32]

Prints one JSON line: median / p90 milliseconds per step (lookup + apply) and per apply of each optimizer, the apply's
algorithmic bytes and bytes / s, and the ratio of the steps."""
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
  uniq = float(np.mean([int(torch.unique(p).numel()) for p in pool]))
  cap = 4 * N + (1 << 20)

  def pair(mult):
    hs = [ops.kv_variable([D], capacity_hint=cap), ops.kv_variable([mult * D], capacity_hint=cap)]
    ops.init_kv_variable_v2(hs[0], torch.randn(64, D, device=dev, generator=gen) * 0.05)
    ops.init_kv_variable_v2(hs[1], torch.zeros(16, mult * D, device=dev))
    return hs

  adam = (0.01, 0.9, 0.999, 0.9, 0.999, 1e-8, 1e-4, 1e-3, 1e-4)
  radam = (0.01, 0.9, 0.999, 0.9, 0.999, 1e-7, 1e-4, 1e-3, 1e-4, 0.4, True, True, False)
  runs = {
      "group_radam_tok": (pair(5), lambda hs, g, i: ops.kv_variable_group_sparse_apply_rectified_adam(*hs, g, i, *radam)),
      "group_adam_v3_tok": (pair(3), lambda hs, g, i: ops.kv_variable_group_sparse_apply_adam_v3(*hs, g, i, *adam)),
  }
  blocks = {"group_radam_tok": 6, "group_adam_v3_tok": 4}          # rows of D floats read (and written) per unique key
  step_ms = {k: [] for k in runs}
  apply_ms = {k: [] for k in runs}
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  for step in range(args.warmup + args.steps):
    for name, (hs, fn) in runs.items():
      ids, g = pool[step % 4], grads[step % 4]
      ev[0].record()
      ops.kv_variable_gather_or_insert_v2(hs[0], ids)          # the token goes with `ids` to the apply
      ev[1].record()
      fn(hs, g, ids)
      ev[2].record()
      ev[2].synchronize()
      if step >= args.warmup:
        step_ms[name].append(ev[0].elapsed_time(ev[2]))
        apply_ms[name].append(ev[1].elapsed_time(ev[2]))
  med = {k: float(np.median(v)) for k, v in step_ms.items()}
  amed = {k: float(np.median(v)) for k, v in apply_ms.items()}
  nbytes = {k: N * (8 + 4 * D) + uniq * (16 + b * 4 * D) + uniq * b * 4 * D for k, b in blocks.items()}
  out = {"batch": N, "dim": D, "keys": args.keys, "zipf": 1.2, "steps": args.steps, "unique_ids_mean": uniq,
         "ms_per_step_median": med, "ms_per_step_p90": {k: float(np.percentile(v, 90)) for k, v in step_ms.items()},
         "ms_per_apply_median": amed, "apply_algorithmic_bytes": nbytes,
         "apply_bytes_per_s": {k: nbytes[k] / (amed[k] * 1e-3) for k in amed},
         "step_ratio_to_group_adam_v3": med["group_radam_tok"] / med["group_adam_v3_tok"]}
  print(json.dumps(out))


if __name__ == "__main__":
  main()
