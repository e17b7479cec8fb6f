"""The crafted-key generator of tests/_hash_keys.py, checked on the CPU: the inverse of mix64, the Python statement of the
hash against the project's other one (ops/sharded.py), and, for every draw tests/test_gpu_adversarial_keys.py and
tests/test_gpu_sharded_two_ranks.py feed the kernels, that the keys are distinct, as many as asked, and that the hash
fields the family promises hold bit for bit.  (What tests/test_kv_model.py is to the fuzz's generator.)"""
import numpy as np
import pytest

import _hash_keys as hk

EDGE_H = [0, 1, hk.M64, 1 << 63, (1 << 63) - 1, 1 << 33, (1 << 33) - 1, 0x8f780810af31a493]


def test_unmix64_inverts_mix64_both_ways():
  rng = np.random.default_rng(0)
  h = rng.integers(0, 1 << 64, 100_000, dtype=np.uint64, endpoint=False)
  assert np.array_equal(hk.mix64_np(hk.unmix64_np(h)), h)
  assert np.array_equal(hk.unmix64_np(hk.mix64_np(h)), h)
  for v in EDGE_H + [int(x) for x in h[:200]]:
    assert hk.mix64(hk.unmix64(v)) == v and hk.unmix64(hk.mix64(v)) == v
    assert int(hk.mix64_np(np.array([v], np.uint64))[0]) == hk.mix64(v)        # the two forms agree
    assert int(hk.unmix64_np(np.array([v], np.uint64))[0]) == hk.unmix64(v)


def test_known_values():
  assert hk.mix64(0) == 0                                   # key 0 homes at slot 0 of every index
  assert hk.SENT_HASH == 0x8f780810af31a493 and hk.SENT_PART == 1147 and hk.SENT_SUB == 0x810af3
  assert hk.to_key(hk.unmix64(hk.SENT_HASH)) == hk.INT64_MIN
  assert (hk.C1 * hk.C1_INV) & hk.M64 == 1 and (hk.C2 * hk.C2_INV) & hk.M64 == 1


def test_matches_the_sharded_module():
  torch = pytest.importorskip("torch")
  from tfplus_amd.kv_variable.python.ops import sharded
  rng = np.random.default_rng(1)
  ids = np.concatenate([rng.integers(-(1 << 63), (1 << 63) - 1, 10_000, endpoint=True), np.array(hk.EDGE_KEYS, np.int64)])
  h = hk.hashes(ids)
  assert np.array_equal(sharded._mix64(torch.from_numpy(ids)).numpy().view(np.uint64), h)
  for world in (2, 3, 4, 8):
    assert np.array_equal(sharded.owner_of(torch.from_numpy(ids), world).numpy(), ((h >> np.uint64(32)) % np.uint64(world)).astype(np.int64))


def test_keys_with_leaves_the_other_bits_random():
  k = hk.keys_with(4096, np.random.default_rng(2), part=hk.SENT_PART, sub=5)
  h = hk.hashes(k)
  assert np.unique(k).size == 4096 and np.all(hk.field(h, 53, 11) == hk.SENT_PART) and np.all(hk.field(h, 20, 24) == 5)
  for lo, width in ((0, 20), (44, 9)):                       # the free bits: every bit is set in 40 .. 60 % of the keys
    for b in range(lo, lo + width):
      assert 0.4 < float(np.mean(hk.field(h, b, 1))) < 0.6, b
  with pytest.raises(AssertionError):
    hk.keys_with(4, np.random.default_rng(2), part=1, bits=[(53, 11, 2)])


@pytest.mark.parametrize("name", sorted(hk.GPU_CASES))
def test_every_draw_the_gpu_tests_use(name):
  fam, args, kw, seed, fields, count = hk.GPU_CASES[name]
  keys = hk.case(name)
  assert np.array_equal(keys, hk.case(name))                # a draw is a function of its seed
  assert keys.size == count == args[0] + hk.N_EDGE[name] and np.unique(keys).size == count
  ne = hk.N_EDGE[name]
  crafted = keys[:count - ne]
  assert keys.dtype == (np.int32 if fam is hk.int32_one_partition else np.int64)
  if ne:
    assert keys[count - ne:].tolist() == list(hk.EDGE_KEYS)
  assert not np.isin(crafted, hk.EDGE_KEYS).any()
  h = hk.hashes(crafted)
  for lo, width, value in fields:
    assert np.all(hk.field(h, lo, width) == np.uint64(value)), (name, lo, width)
  if fam is hk.one_owner:
    world, r = args[1], args[2]
    assert r == world - 1 and np.all((h >> np.uint64(32)) % np.uint64(world) == r)
  if fam is hk.int32_one_partition:
    assert crafted.min() >= -(1 << 21) and crafted.max() < (1 << 21)
  if fields and fields[0] == hk._PART:                      # the sentinel's partition for every P the library picks
    for P in (64, 128, 256, 512, 1024, 2048):
      sh = np.uint64(64 - P.bit_length() + 1)
      assert np.all((h >> sh) == np.uint64(hk.SENT_HASH >> int(sh)))


def test_int32_candidates_are_as_many_as_the_issue_counted():
  cand = np.arange(-(1 << 21), 1 << 21, dtype=np.int64)
  h = hk.hashes(cand)
  assert int(np.sum((h >> np.uint64(58)) == np.uint64(hk.SENT_HASH >> 58))) == 65538
  assert int(np.sum((h >> np.uint64(54)) == np.uint64(hk.SENT_HASH >> 54))) == 3997


def test_A4_hot_keys_share_the_class_that_is_processed():
  """A4 at D = 6 is written for the branch that takes more than 16 keys of more than 16 chunks in ONE class (lnbig is
  counted per class): for either size of the partition blocks' key table (768, 1023) the split of the 2000 keys ends at
  R <= 8 and one processed class holds all 20 hot keys; 2101 occurrences are 17 chunks of HC = 128 rows"""
  cold, hot = hk.case("A4"), hk.case("A4_hot")
  keys = np.concatenate([cold, hot])
  assert np.unique(keys).size == 2000
  assert (2101 + 127) // 128 == 17
  for ucapk in (768, 1023):
    cls = hk.final_classes(keys, ucapk)
    assert sum(v.size for v in cls.values()) == 2000 and max(R for R, _ in cls) <= 8
    assert len(cls) > 1                                        # the partition does split
    assert sorted(int(np.isin(hot, v).sum()) for v in cls.values())[-1] == 20
