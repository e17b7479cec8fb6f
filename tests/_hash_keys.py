"""Keys crafted against the library's hash (NumPy only, no GPU).

Every kernel places a key by fixed bit fields of mix64(key) (csrc/kv_device.h), murmur3's 64-bit finaliser.  It is a
bijection: its inverse is the three xor-shifts undone and two multiplications by the constants' inverses mod 2^64.  So a
test chooses the HASH it wants (which partition, which LDS slot, which home slot, which owner) and gets the key.

  bits of mix64(key)         decides
  low log2(cap)              home slot of the table index (linear probe, `& mask`)
  8 .. 17/18                 slot of the partition block's LDS key hash (lds_key_slot<HSK>, HSK 1024 / 2048)
  20 ..                      sub-hash class (in_round) when a partition holds more keys than that hash
  40 .. 51                   slot of the tile pass's LDS hash (LS = 4096)
  (hash >> 32) % world       owner shard
  top log2(P), P <= 2048     hash partition (part_of)

keys_with(n, rng, **fields) is the generator; the named families below are what tests/test_gpu_adversarial_keys.py feeds
(tests/test_hash_keys.py asserts every family's fields for the seeds used there)."""
import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
EDGE_KEYS = (INT64_MIN, INT64_MAX, 0, -1)                   # INT64_MIN is the index's EMPTY_KEY (its own slot, stored as 0)
EDGE_KEYS32 = (-(1 << 31), (1 << 31) - 1, 0, -1)


# ---- the hash and its inverse: Python ints (unsigned 64-bit values) ------------------------------------------------
def mix64(x):
  x &= M64
  x ^= x >> 33; x = (x * C1) & M64
  x ^= x >> 33; x = (x * C2) & M64
  x ^= x >> 33
  return x


def unmix64(h):
  # y = x ^ (x >> 33) is its own inverse on 64 bits (33 * 2 >= 64: the shifted-in part is x's untouched top bits)
  h &= M64
  h ^= h >> 33; h = (h * C2_INV) & M64
  h ^= h >> 33; h = (h * C1_INV) & M64
  h ^= h >> 33
  return h


def to_key(u):
  """unsigned 64-bit value -> the int64 key with those bits"""
  return u - (1 << 64) if u >= (1 << 63) else u


def hash_of(key):
  """mix64 of an int64 key (Python int)"""
  return mix64(key & M64)


# ---- vectorised (uint64 arrays; the products wrap) -----------------------------------------------------------------
def mix64_np(x):
  x = np.asarray(x).astype(np.uint64, copy=True)
  with np.errstate(over="ignore"):
    x ^= x >> np.uint64(33); x *= np.uint64(C1)
    x ^= x >> np.uint64(33); x *= np.uint64(C2)
    x ^= x >> np.uint64(33)
  return x


def unmix64_np(h):
  h = np.asarray(h).astype(np.uint64, copy=True)
  with np.errstate(over="ignore"):
    h ^= h >> np.uint64(33); h *= np.uint64(C2_INV)
    h ^= h >> np.uint64(33); h *= np.uint64(C1_INV)
    h ^= h >> np.uint64(33)
  return h


def hashes(keys):
  """mix64 of int64 (or int32: sign-extended, as the kernels widen them) keys -> uint64"""
  return mix64_np(np.asarray(keys).astype(np.int64).view(np.uint64))


def field(h, lo, width):
  """bits lo .. lo+width-1 of the uint64 hashes h"""
  return (np.asarray(h, np.uint64) >> np.uint64(lo)) & np.uint64((1 << width) - 1)


# ---- the fields, by name: (lowest bit, width) ---------------------------------------------------------------------
FIELDS = {
    "part": (53, 11),    # top 11 bits: the partition for every P <= 2048
    "sub": (20, 24),     # sub-hash classes (in_round)
    "lds": (8, 11),      # partition LDS hash, HSK 2048 (HSK 1024: its low 10 bits)
    "tile": (40, 12),    # tile LDS hash
    "home": (0, 24),     # home slot for every index of up to 2^24 entries
}
SENT_HASH = mix64(INT64_MIN & M64)                        # 0x8f780810af31a493
SENT_PART = SENT_HASH >> 53                               # 1147
SENT_SUB = (SENT_HASH >> 20) & 0xFFFFFF                   # 0x810af3


def keys_with(n, rng, bits=(), owner=None, **fields):
  """n distinct int64 keys (none of EDGE_KEYS) whose hash has the given fields fixed and every other bit drawn from rng.
  fields: name=value for the names of FIELDS; bits: further (lo, width, value) triples; owner=(world, r): also
  (hash >> 32) % world == r (by rejection).  Distinct hashes are distinct keys: mix64 is a bijection."""
  fixed = [FIELDS[k] + (v,) for k, v in fields.items()] + [tuple(b) for b in bits]
  keep, val = M64, 0
  for lo, width, v in fixed:
    assert 0 <= v < (1 << width) and lo + width <= 64, (lo, width, v)
    m = ((1 << width) - 1) << lo
    assert (~keep & m) == 0 or ((val >> lo) & ((1 << width) - 1)) == v, "overlapping fields disagree"
    keep &= ~m
    val |= v << lo
  edge_h = np.array([hash_of(k) for k in EDGE_KEYS], np.uint64)
  got = np.empty(0, np.uint64)
  while got.size < n:
    h = rng.integers(0, 1 << 64, 2 * (n - got.size) + 16, dtype=np.uint64, endpoint=False)
    h = (h & np.uint64(keep)) | np.uint64(val)
    if owner is not None:
      h = h[(h >> np.uint64(32)) % np.uint64(owner[0]) == np.uint64(owner[1])]
    h = h[~np.isin(h, edge_h)]
    _, first = np.unique(np.concatenate([got, h]), return_index=True)
    got = np.concatenate([got, h])[np.sort(first)]           # arrival order kept: the result depends on rng alone
  return unmix64_np(got[:n]).view(np.int64)


def _with_edge(keys, edge, edge_keys=EDGE_KEYS):
  if not edge:
    return keys
  return np.concatenate([keys, np.array(edge_keys, keys.dtype)])


# ---- the named families (edge=True appends INT64_MIN, INT64_MAX, 0, -1: n + 4 keys) ---------------------------------
def one_partition(n, rng, edge=False):
  """the sentinel key's partition for every P <= 2048, everything else random"""
  return _with_edge(keys_with(n, rng, part=SENT_PART), edge)


def one_class(n, k, value, rng, edge=False):
  """one_partition, and hash bits 20 .. 20+k-1 equal to `value`: the first k splits of the partition leave the keys together"""
  return _with_edge(keys_with(n, rng, part=SENT_PART, bits=[(20, k, value)]), edge)


def deep_split(n, k, rng, edge=False):
  """one_class with the sentinel's own bits: the first k splits of the partition put every key and the sentinel into one
  class and leave its sibling empty"""
  return one_class(n, k, SENT_SUB & ((1 << k) - 1), rng, edge)


def final_classes(keys, ucapk):
  """The partition pass's split of one partition's keys, restated: a class of at least `ucapk` distinct keys is halved by
  the next sub-hash bit (in_round: (hash >> 20) & (R - 1) == round).  Returns {(R, round): keys} of the classes that are
  processed.  (No stack bound here: for key sets that are not refused.)"""
  sub = hashes(keys) >> np.uint64(20)
  out, todo = {}, [(1, 0)]
  while todo:
    R, r = todo.pop()
    sel = (sub & np.uint64(R - 1)) == np.uint64(r)
    if int(sel.sum()) >= ucapk:
      todo += [(2 * R, r), (2 * R, r + R)]
    else:
      out[(R, r)] = np.asarray(keys)[sel]
  return out


def inseparable(n, rng, sub=0xFFFFFF, edge=False):
  """one_partition, and hash bits 20 .. 43 all `sub`: no sub-hash class of those 24 bits separates the keys.  The default,
  all ones, is the pattern the partition pass REFUSES (every split leaves the empty sibling on its 24-deep stack);
  sub=SENT_SUB puts the sentinel key among them (a pattern that is split 24 times and then separates on bits 44 ..)."""
  return _with_edge(keys_with(n, rng, part=SENT_PART, sub=sub), edge)


def one_lds_slot(n, rng, edge=False):
  """one_partition, and bits 8 .. 18 all ones: every key homes at the LAST slot of the partition LDS hash (HSK 1024 and
  2048 alike), so the probe wraps"""
  return _with_edge(keys_with(n, rng, part=SENT_PART, lds=(1 << 11) - 1), edge)


def one_tile_slot(n, rng, edge=False):
  """bits 40 .. 51 all ones: every key homes at the last slot of the tile pass's LDS hash"""
  return _with_edge(keys_with(n, rng, tile=(1 << 12) - 1), edge)


def last_home(n, rng, edge=False):
  """low 24 bits all ones: the home is slot `mask` of every index of up to 2^24 entries; the chain wraps to slot 0"""
  return _with_edge(keys_with(n, rng, home=(1 << 24) - 1), edge)


def one_owner(n, world, r, rng, edge=False):
  """(hash >> 32) % world == r: rank r owns every key"""
  return _with_edge(keys_with(n, rng, owner=(world, r)), edge)


def int32_one_partition(n, rng, edge=False):
  """int32 keys of [-2^21, 2^21) whose top 6 hash bits are the sentinel's (65 538 of them): one partition whenever
  P <= 64.  edge=True appends INT32_MIN, INT32_MAX, 0, -1 (wherever they hash to)."""
  cand = np.arange(-(1 << 21), 1 << 21, dtype=np.int64)
  cand = cand[(hashes(cand) >> np.uint64(58)) == np.uint64(SENT_HASH >> 58)]
  cand = cand[~np.isin(cand, EDGE_KEYS32)]
  assert cand.size >= n
  return _with_edge(rng.permutation(cand)[:n].astype(np.int32), edge, EDGE_KEYS32)


# ---- the draws the GPU tests use: name -> (family, arguments, seed, the hash fields that must hold) ----------------------
# tests/test_hash_keys.py asserts the fields of exactly these draws; the GPU files call case(name) and nothing else.
_PART = (53, 11, SENT_PART)
GPU_CASES = {
    "A1": (one_partition, (3000,), dict(edge=True), 11, [_PART], 3004),
    "A2_k3": (deep_split, (3000, 3), dict(edge=True), 12, [_PART, (20, 3, SENT_SUB & 7)], 3004),
    "A2_k8": (deep_split, (3000, 8), dict(edge=True), 13, [_PART, (20, 8, SENT_SUB & 255)], 3004),
    "A3_lds": (one_lds_slot, (700,), {}, 14, [_PART, (8, 11, 2047), (8, 10, 1023)], 700),
    "A3_tile": (one_tile_slot, (2048,), {}, 15, [(40, 12, 4095)], 2048),
    "A4": (one_partition, (1980,), {}, 16, [_PART], 1980),
    "A4_hot": (one_class, (20, 3, 5), {}, 26, [_PART, (20, 3, 5)], 20),   # the hot keys: one class as deep as R = 8
    "A5": (one_partition, (60000,), {}, 17, [_PART], 60000),
    "A6": (int32_one_partition, (3000,), {}, 18, [(58, 6, SENT_HASH >> 58)], 3000),
    "A7": (inseparable, (1100,), dict(sub=SENT_SUB, edge=True), 19, [_PART, (20, 24, SENT_SUB)], 1104),
    "B1": (one_partition, (66000,), {}, 21, [_PART], 66000),
    "B2": (inseparable, (1100,), {}, 22, [_PART, (20, 24, 0xFFFFFF)], 1100),
    "B3": (one_partition, (300,), {}, 23, [_PART], 300),
    "C": (last_home, (500,), dict(edge=True), 31, [(0, 24, 0xFFFFFF)], 504),
    "D_w2": (one_owner, (1500, 2, 1), dict(edge=True), 42, [], 1504),
    "D_w3": (one_owner, (1500, 3, 2), dict(edge=True), 43, [], 1504),
    "D_w4": (one_owner, (1500, 4, 3), dict(edge=True), 44, [], 1504),
}
N_EDGE = {name: (4 if c[2].get("edge") else 0) for name, c in GPU_CASES.items()}


def case(name):
  """the keys of GPU_CASES[name] (the crafted ones first, the edge keys last)"""
  fam, args, kw, seed, _, _ = GPU_CASES[name]
  return fam(*args, rng=np.random.default_rng(seed), **kw)
