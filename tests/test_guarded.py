"""tests/_guarded.py held against faults planted by hand, on CPU tensors: every kind of error the guarded buffers exist
to catch is reported, with the offset it happened at, and what is not an error passes."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _guarded as G  # noqa: E402
from _guarded import Guarded, frozen  # noqa: E402

N, D = 5, 7


def _written(g):
  """what a correct op leaves: every element of the buffer"""
  g.t.copy_(torch.arange(g.t.numel(), dtype=torch.float32).view(g.t.shape).to(g.t.dtype))
  return g


def _poke(g, element, value=1.0):
  """one element written at `element` relative to the buffer's start, through the allocation (what a stray store does)"""
  at = g.begin + element * g.item
  g.raw[at:at + g.item].view(g.dtype).fill_(value)


def _fails(call, text):
  with pytest.raises(AssertionError) as e:
    call()
  assert re.search(text, str(e.value)), str(e.value)


def test_layout():
  for d in (1, 3, 7, 100, 1024):
    g = Guarded((N, d))
    assert g.t.shape == (N, d) and g.t.is_contiguous() and g.t.data_ptr() % 16 == 0, d
    rows_front, rows_back = (g.begin - g.front) // (4 * d), (g.back - g.end) // (4 * d)
    assert rows_front >= 8 and rows_front % 4 == 0 and g.begin - g.front >= 8192
    assert rows_back >= 8 and g.back - g.end >= 8192
    assert bool((g.raw[g.front:g.back].view(torch.int32) == G.SENT_F32).all())
  for dt in (torch.uint8, torch.int32, torch.int64):
    g = Guarded(N, dt)
    assert g.t.shape == (N,) and g.t.data_ptr() % 16 == 0 and g.begin - g.front >= 8192
    assert bool((g.raw == G.SENT_BYTE).all())
  assert np.isnan(np.array([G.SENT_F32], np.uint32).view(np.float32)[0])


@pytest.mark.parametrize("d", [1, 3, 7, 100])
def test_base_is_16_byte_aligned(d):
  for g in Guarded.many([((3, d), torch.float32), ((1, d), torch.float32), (5, torch.uint8), ((2, d), torch.float32)]):
    assert g.t.data_ptr() % 16 == 0


def test_clean_run_passes():
  _written(Guarded((N, D))).check(N)
  g = Guarded((N, D))
  g.t[:3] = 2.0
  g.check(3, rest_untouched=True)
  g.check(slice(0, 3))
  g.check(torch.tensor([True, True, True, False, False]))
  Guarded((0, D)).check(0, rest_untouched=True)
  Guarded((N, D)).check(0, rest_untouched=True)
  for dt in (torch.uint8, torch.int32, torch.int64):
    g = Guarded(N, dt)
    g.t.fill_(3)
    g.check(N)


def test_another_nan_passes():
  g = _written(Guarded((N, D)))
  g.t[2, 3] = float("nan")
  g.t.view(torch.int32)[4, 0] = 0x7FE5A5A5      # the sentinel quieted: still another pattern
  g.check(N)


def test_one_element_before():
  g = _written(Guarded((N, D), name="rows"))
  _poke(g, -1)
  _fails(lambda: g.check(N), r"rows: front guard, written at element -1 \(row -1\)")


def test_one_element_after():
  g = _written(Guarded((N, D), name="rows"))
  _poke(g, N * D)
  _fails(lambda: g.check(N), r"rows: back guard, written at element %d \(row %d\)" % (N * D, N))


def test_far_ends_of_the_guards():
  g = _written(Guarded((N, D), name="rows"))
  first = -(g.begin - g.front) // 4
  _poke(g, first)
  _fails(lambda: g.check(N), r"front guard, written at element %d \(row %d\)" % (first, first // D))
  g = _written(Guarded((N, D)))
  last = (g.back - g.begin) // 4 - 1
  _poke(g, last)
  _fails(lambda: g.check(N), r"back guard, written at element %d \(row %d\)" % (last, last // D))


def test_a_zero_written_into_a_guard_is_seen():
  g = _written(Guarded(N, torch.int64, name="keys"))
  _poke(g, N, 0)
  _fails(lambda: g.check(N), r"keys: back guard, written at element %d" % N)


def test_row_left_unwritten():
  g = Guarded((N, D), name="rows")
  g.t[:3] = 1.0
  g.t[4] = 1.0
  _fails(lambda: g.check(N), r"rows: buffer, not written at element %d \(row 3\)" % (3 * D))


def test_element_left_unwritten():
  g = _written(Guarded((N, D), name="rows"))
  g.t.view(torch.int32)[2, 5] = G.SENT_F32
  _fails(lambda: g.check(N), r"rows: buffer, not written at element %d \(row 2\)" % (2 * D + 5))
  g = Guarded(N, torch.uint8, name="flags")
  g.t[:4] = 1
  _fails(lambda: g.check(N), r"flags: buffer, not written at element 4 \(row 4\)")


def test_written_outside_the_defined_rows():
  g = Guarded((N, D), name="rows")
  g.t[:2] = 1.0
  g.t[3, 1] = 0.0
  _fails(lambda: g.check(2, rest_untouched=True), r"rows: buffer, written outside the defined extent at element %d \(row 3\)" % (3 * D + 1))


def test_stray_write_between_two_buffers():
  a, b, c = Guarded.many([((N, D), torch.float32, "a"), ((0, D), torch.float32, "empty"), ((N, 3), torch.float32, "c")])
  assert a.raw is b.raw is c.raw and a.back == b.front and b.back == c.front
  _written(a), _written(c)
  for g, n in ((a, N), (b, 0), (c, N)):
    g.check(n)
  _poke(a, N * D)                                 # a's lane one past its last row
  _fails(lambda: a.check(N), r"a: back guard, written at element %d \(row %d\)" % (N * D, N))
  b.check(0), c.check(N)
  _poke(c, -2)
  _fails(lambda: c.check(N), r"c: front guard, written at element -2 \(row -1\)")
  # a buffer of no rows: anything the op writes for it lands in its guards
  a, b = Guarded.many([((0, D), torch.float32, "none"), ((N, D), torch.float32, "b")])
  _poke(a, 0)
  _fails(lambda: a.check(0), r"none: back guard, written at element 0 \(row 0\)")


def test_frozen_inputs():
  ids = torch.arange(100, dtype=torch.int64)
  grad = torch.ones(100, D)
  with frozen(ids, grad=grad):
    pass
  with pytest.raises(AssertionError, match=r"input\[0\]: input changed at element 41 \(row 41\)"):
    with frozen(ids, grad=grad):
      ids[41] += 1
  ids[41] -= 1
  f = frozen(ids=ids, grad=grad, weights=None)
  grad.view(torch.int32)[9, 2] ^= 1               # one bit of one gradient element
  _fails(f.verify, r"grad: input changed at element %d \(row 9\)" % (9 * D + 2))
  # -0.0 for +0.0 compares equal as floats, not as bytes
  z = torch.zeros(4)
  f = frozen(z=z)
  z[3] = -0.0
  _fails(f.verify, r"z: input changed at element 3")


def test_same_bits():
  a = np.arange(12, dtype=np.float32).reshape(3, 4)
  G.same_bits(torch.from_numpy(a.copy()), a)
  b = a.copy()
  b[2, 1] = np.nextafter(b[2, 1], np.float32(100))
  _fails(lambda: G.same_bits(b, a, "rows"), r"rows: 1 of 12 elements differ, first at element 9 \(row 2\)")
  _fails(lambda: G.same_bits(np.float32([-0.0]), np.float32([0.0])), "differ")
  # an expected NaN (0/0) is met by any NaN, and by nothing else
  nan = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
  G.same_bits(nan, nan[::-1].copy())
  _fails(lambda: G.same_bits(np.float32([1.0, 2.0]), nan), r"2 of 2 elements differ")
  _fails(lambda: G.same_bits(nan, np.float32([1.0, 2.0])), r"2 of 2 elements differ")
