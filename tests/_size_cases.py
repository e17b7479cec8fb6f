"""The size boundaries of the table ops restated, and the inputs of the tests that sit on them (test_size_cases.py checks
this file on the CPU, test_gpu_size_limits.py runs the cases).

Limits: how many ids one index pass takes, where the chunk loops of kv_ops.hip cut a longer call, the longest lookup.
source_limits() reads the same values out of the sources, so a changed limit fails on the CPU instead of moving a
boundary away from the GPU cases.

key_row: a row that is an exact fp32 function of its key — small integers, never all zero, distinct for distinct keys
in [0, 2^52) — in torch on whatever device the keys are on, so a wide expectation never exists on the host.
straddle_ids: a batch that crosses a chunk boundary with every kind of key the boundary can treat differently.
Gradients are integer-valued with |g| <= 3 (draw_int_rows): every per-key sum stays below 2^24 and is exact in any order.
adagrad_ref: the Adagrad step in float64."""
import os
import re

import numpy as np

FUSED_MAX_N = 1 << 23        # ids of one index pass at the dims of the entry-list kernels (multiples of 4 up to 256)
OTHER_DIM_MAX_N = 1 << 21    # ... at every other dim
SCATTER_CHUNK = 1 << 21      # scatter_like (insert, assign, import stages) and the folding kv_scatter_update cut here
LOOKUP_MAX_N = 1 << 30       # the longest kv_gather_or_insert
TILE = 2048                  # ids per tile of the tile pass
MAX_KEYS = 300_000           # distinct keys of an oracle-backed case
FREQ_MAX = 65535             # where a key's frequency saturates

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tfplus_amd", "csrc")


def _src(name):
  with open(os.path.join(CSRC, name)) as f:
    return f.read()


def _function(text, head):
  """The definition that starts with `head`, up to its closing brace in column 0."""
  at = text.index(head)
  return text[at:text.index("\n}\n", at) + 3]


def _shift(text, pattern):
  """The value of the one `1ll << K` the pattern's group captures; the pattern must occur exactly once."""
  found = re.findall(pattern, text)
  assert len(found) == 1, (pattern, found)
  return 1 << int(found[0])


def source_limits():
  """{name: value} of the limits above as kv_host.h, kv_ops.hip and kv_device.h state them."""
  host, ops, dev = _src("kv_host.h"), _src("kv_ops.hip"), _src("kv_device.h")
  goi = _function(ops, "int gather_or_insert_impl(")
  scat = _function(ops, "static int scatter_like(")
  upd = _function(ops, "int kv_scatter_update(")
  out = {"FUSED_MAX_N": _shift(host, r"constexpr long long FUSED_MAX_N = 1ll << (\d+);")}
  out["OTHER_DIM_MAX_N"] = _shift(goi, r"const long long CHK = fused_tab\(t\) \? FUSED_MAX_N : \(1ll << (\d+)\);")
  out["LOOKUP_MAX_N"] = _shift(goi, r"if \(n < 0 \|\| n > \(1ll << (\d+)\)\) return fail\(KV_INVALID_ARGUMENT")
  out["SCATTER_CHUNK"] = _shift(scat, r"const long long CH = 1ll << (\d+);")
  out["FOLD_CHUNK"] = _shift(upd, r"const long long CHK = 1ll << (\d+);")
  # every loop steps by the constant it names
  assert len(re.findall(r"for \(long long off = 0; off < n; off \+= CHK\)", goi)) == 1
  assert len(re.findall(r"for \(long long off = 0; off < n; off \+= CH\)", scat)) == 1
  assert len(re.findall(r"for \(long long off = 0; off < n; off \+= CHK\)", upd)) == 1
  tbt = int(re.search(r"#define KV_TBT (\d+)", dev).group(1))
  ipt = int(re.search(r"constexpr int IPT = (\d+);", dev).group(1))
  assert re.search(r"constexpr int TILE = TBT \* IPT;", dev) and re.search(r"constexpr int TBT = KV_TBT;", dev)
  out["TILE"] = tbt * ipt
  return out


# ---- rows ------------------------------------------------------------------------------------------------------------------
_MIX = -7046029254386353131          # 0x9E3779B97F4A7C15 as int64: odd, so key -> key * _MIX is a bijection on any low 2^k bits
_LOW52 = (1 << 52) - 1
ROW_CHUNK = 1 << 18                  # key_row fills a wide output this many rows at a time


def key_row(keys, D, out=None):
  """[len(keys), D] fp32 rows, on the keys' device.  y = key * _MIX mod 2^52 (a bijection of [0, 2^52)); its four 13-bit
  digits are elements 0..3, so distinct keys in [0, 2^52) have distinct rows at every D >= 4; element e >= 4 is digit
  (e + e // 4) mod 4 plus 977 (e // 4), mod 8192.  Every element minus 4095: integers in [-4095, 4096], exact in fp32."""
  import torch
  keys = torch.as_tensor(keys).reshape(-1)
  n = keys.numel()
  if out is None:
    out = torch.empty((n, D), dtype=torch.float32, device=keys.device)
  e = torch.arange(D, device=keys.device)
  col = (e + e // 4) % 4
  add = ((e // 4) * 977).to(torch.int32)
  shifts = torch.tensor([0, 13, 26, 39], device=keys.device)
  for i in range(0, n, ROW_CHUNK):
    y = (keys[i:i + ROW_CHUNK].to(torch.int64) * _MIX) & _LOW52
    dig = ((y.unsqueeze(1) >> shifts) & 8191).to(torch.int32)            # [m, 4]
    out[i:i + ROW_CHUNK] = ((dig[:, col] + add) & 8191) - 4095
  return out


def draw_keys(rng, count, bits=40):
  """`count` distinct keys in [1, 2^bits), in random order."""
  assert count < (1 << bits) // 4
  k = np.unique(rng.integers(1, 1 << bits, int(count * 1.1) + 16, dtype=np.int64))
  assert k.size >= count
  return rng.permutation(k)[:count]


def draw_int_rows(n, D, gen, device, values=(-3, -2, -1, 1, 2, 3), out=None):
  """[n, D] fp32 rows drawn from `values` (torch, on `device`; into out[:n] when given)."""
  import torch
  v = torch.tensor(values, dtype=torch.float32, device=device)
  if out is None:
    out = torch.empty((n, D), dtype=torch.float32, device=device)
  for i in range(0, n, ROW_CHUNK):       # (the index tensor is int64: a wide draw goes chunk by chunk)
    m = min(ROW_CHUNK, n - i)
    out[i:i + m] = v[torch.randint(0, len(values), (m, D), generator=gen, device=device)]
  return out


# ---- ids across a chunk boundary ---------------------------------------------------------------------------------------
def straddle_ids(chunk, tail, rng, keys=MAX_KEYS, bits=40):
  """chunk + tail ids over at most `keys` distinct keys, as a dict:
    ids   int64 [chunk + tail]
    a     keys that occur in the first `chunk` positions only
    b     keys that occur on both sides of the boundary (besides d)
    c     keys that occur only in the `tail` positions
    d     one key with FREQ_MAX - 1 occurrences before the boundary and two after it: FREQ_MAX + 1 in all, so its
          frequency saturates only if the second pass continues the count of the first
    e     (ids[chunk - 1], ids[chunk]): an `a` key and a `c` key, either side of the boundary
  A tail of 3 holds one c key and d twice; a longer one as many b and c keys as fit.  Positions beyond one per key are
  filled Zipf(1.2) over the side's keys (the hottest ones saturate inside one pass, and the oracle stays in its caches)."""
  assert tail >= 3 and keys >= 8
  n_side = max(1, min((keys - 1) // 3, (chunk - (FREQ_MAX - 1)) // 4))
  n_c = max(1, min(n_side, (tail - 2) // 2))
  n_b = max(0, min(n_side, tail - 2 - n_c))
  pool = draw_keys(rng, 2 * n_side + n_c + 1, bits)
  a, b_all, c, d = pool[:n_side], pool[n_side:2 * n_side], pool[2 * n_side:2 * n_side + n_c], pool[-1]
  b = b_all[:n_b]
  first_pool = np.concatenate([a, b]) if n_b else a
  fill = chunk - (FREQ_MAX - 1) - first_pool.size
  assert fill >= 0, "chunk too short for its keys"
  first = np.concatenate([np.full(FREQ_MAX - 1, d), first_pool, first_pool[rng.zipf(1.2, fill) % first_pool.size]])
  rng.shuffle(first)
  at = np.flatnonzero(first == a[0])[0]                 # the last position before the boundary: an `a` key
  first[at], first[-1] = first[-1], first[at]
  tail_pool = np.concatenate([c, b]) if n_b else c
  fill = tail - 2 - tail_pool.size
  assert fill >= 0
  last = np.concatenate([np.full(2, d), tail_pool, tail_pool[rng.zipf(1.2, fill) % tail_pool.size]])
  rng.shuffle(last)
  at = np.flatnonzero(last == c[0])[0]                  # the first position after it: a `c` key
  last[at], last[0] = last[0], last[at]
  ids = np.concatenate([first, last]).astype(np.int64)
  return dict(ids=ids, a=a, b=b, c=c, d=np.int64(d), e=(ids[chunk - 1], ids[chunk]), chunk=chunk)


def class_keys(s):
  """The keys a case reads frequency and day stamp of: every key of a, b and c, then d and the two of e; with them the
  class of every position of the list, for the message of a mismatch."""
  keys = np.concatenate([s["a"], s["b"], s["c"], [s["d"]], list(s["e"])]).astype(np.int64)
  names = np.array(["a"] * s["a"].size + ["b"] * s["b"].size + ["c"] * s["c"].size + ["d", "e[0]", "e[1]"])
  return keys, names


def distinct_keys(n, device=None, start=1):
  """n distinct keys in torch: (start + i) * 1000003, far below 2^52 for every n a case uses."""
  import torch
  return (torch.arange(start, start + n, dtype=torch.int64, device=device)) * 1000003


# what the GPU cases use, by name: (chunk, tail, key bits)
SEED = 20251020
STRADDLES = {
    "fused+3": (FUSED_MAX_N, 3, 40),                 # one pass and a tail of three ids
    "fused-int32+3": (FUSED_MAX_N, 3, 31),           # ... with keys an int32 table takes
    "fused-x2": (FUSED_MAX_N, FUSED_MAX_N, 40),      # an exact multiple: no short last pass
    "other+3": (OTHER_DIM_MAX_N, 3, 40),             # the sorted-position pipeline's pass, and the scatter chunk
}
assert OTHER_DIM_MAX_N == SCATTER_CHUNK
NONFUSED_DIM = 257     # the smallest dim outside the entry-list kernels whose lookups take the 2^21-id pass; a scalar row copy
NONFUSED_DIM4 = 260    # ... and the smallest one the optimizer ops serve too (float4 rows)
WIDE_DIM = 1024
WIDE_N = (1 << 21) + 4096          # x 1024: the last two tiles lie wholly beyond element 2^31
WIDE_KEYS = 65536
WIDE_TAIL = 4096                   # the last positions of a wide batch: keys that occur nowhere else
WIDE_TAIL_KEYS = 512


def straddle_case(name):
  chunk, tail, bits = STRADDLES[name]
  rng = np.random.default_rng([SEED, sorted(STRADDLES).index(name)])
  return straddle_ids(chunk, tail, rng, bits=bits)


# ---- Adagrad -----------------------------------------------------------------------------------------------------------
def adagrad_ref(x, acc, gsum, lr):
  """(x', acc') of KvVariableSparseApplyAdagrad with update_slots, in float64: acc' = acc + g^2, x' = x - lr g / sqrt(acc').
  numpy arrays or torch tensors; lr is rounded to fp32 first, as the op receives it."""
  lr = float(np.float32(lr))
  if isinstance(x, np.ndarray):
    x, acc, g = x.astype(np.float64), np.asarray(acc, np.float64), np.asarray(gsum, np.float64)
    acc2 = acc + g * g
    return x - lr * g / np.sqrt(acc2), acc2
  x, acc, g = x.double(), acc.double(), gsum.double()
  acc2 = acc + g * g
  return x - lr * g / acc2.sqrt(), acc2
