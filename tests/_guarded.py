"""Caller buffers for tests that ask where an op wrote, not only what (test_guarded.py checks this file on the CPU,
test_gpu_buffer_extents.py uses it on every op that writes a caller's buffer).

  Guarded(shape, dtype, device)   front guard | buffer | back guard in ONE allocation, all prefilled with a sentinel; `.t`
                                  is the buffer, a contiguous view.  A guard is at least 8 rows and at least 8 KiB (the widest
                                  row class spans 1024 floats = 4 KiB: a one-row overrun at any dim lands inside it) and a
                                  multiple of 4 rows, so the buffer's base is 16-byte aligned at every dim, odd ones included.
  Guarded.many([(shape, dtype)])  several outputs of one call in one allocation, guards between neighbours: an overrun from
                                  one output towards the next is caught.
  g.check(defined)                both guards still hold the sentinel in every byte; no element of the `defined` extent (a
                                  row count, a slice of rows, a mask over rows or elements) holds it — a skipped store reads
                                  as the sentinel, whatever the allocator handed out.  rest_untouched=True: every element
                                  outside `defined` still holds it.
  frozen(*tensors, **named)       context manager (or .verify()): the inputs are byte-identical afterwards.
  same_bits(got, want, name)      two buffers bit for bit, the first difference by element and row.

The float sentinel is ONE NaN bit pattern, 0x7FA5A5A5: no op produces that payload from finite inputs, and a NaN an op does
produce (0/0 of an empty weighted segment) has another.  Integer buffers are filled with the byte 0xA5.  Every comparison
is on bits (int32 / uint8 views), never a float ==.  Plain torch: works on CPU tensors too."""
import math

import numpy as np
import torch

SENT_F32 = 0x7FA5A5A5
SENT_BYTE = 0xA5
GUARD_ROWS = 8
GUARD_BYTES = 8192


def _sent_bytes(dtype):
  """the sentinel of one element of `dtype`, as its bytes in memory"""
  size = torch.empty((), dtype=dtype).element_size()
  if dtype == torch.float32:
    return np.array([SENT_F32], np.uint32).view(np.uint8).copy()
  return np.full(size, SENT_BYTE, np.uint8)


def _fill(raw, dtype):
  """raw: uint8 [k * itemsize], 4-byte aligned"""
  if raw.numel() == 0:
    return
  if dtype == torch.float32:
    raw.view(torch.int32).fill_(SENT_F32)
  else:
    raw.fill_(SENT_BYTE)


def _is_sentinel(raw, dtype):
  """uint8 [k * itemsize] -> bool [k]: the element holds the sentinel's bits"""
  if dtype == torch.float32:
    return raw.view(torch.int32) == SENT_F32
  size = torch.empty((), dtype=dtype).element_size()
  return (raw.view(-1, size) == SENT_BYTE).all(dim=1)


def guard_rows(row_bytes):
  """rows of one guard: >= 8 rows, >= 8 KiB, a multiple of 4 rows and of 16 bytes"""
  step = 4 * (16 // math.gcd(16, 4 * row_bytes))
  rows = max(GUARD_ROWS, -(-GUARD_BYTES // row_bytes))
  return -(-rows // step) * step


def _layout(specs):
  """byte offsets of front guard | buffer | back guard for each spec, one after the other -> (plans, total bytes)"""
  plans, at = [], 0
  for i, spec in enumerate(specs):
    shape, dtype = spec[0], spec[1]
    name = spec[2] if len(spec) > 2 else "out[%d]" % i
    shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    row_len = int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 1
    row_bytes = max(1, row_len) * item
    g = guard_rows(row_bytes) * row_bytes
    assert at % 16 == 0 and g % 16 == 0
    begin, end = at + g, at + g + int(np.prod(shape, dtype=np.int64)) * item
    back = end + g
    back += -back % 16                       # the next buffer's guard starts on 16 bytes; the padding belongs to this guard
    plans.append((name, shape, dtype, item, max(1, row_len), at, begin, end, back))
    at = back
  return plans, at


def _allocate(total, device):
  raw = torch.empty(total, dtype=torch.uint8, device=device)
  assert raw.data_ptr() % 16 == 0
  return raw


class Guarded:
  def __init__(self, shape, dtype=torch.float32, device="cpu", name="out"):
    plans, total = _layout([(shape, dtype, name)])
    self._attach(_allocate(total, device), plans[0])

  @staticmethod
  def many(specs, device="cpu"):
    """specs: (shape, dtype) or (shape, dtype, name) per buffer -> one Guarded each, neighbours in one allocation"""
    plans, total = _layout(specs)
    raw = _allocate(total, device)
    out = []
    for plan in plans:
      g = Guarded.__new__(Guarded)
      g._attach(raw, plan)
      out.append(g)
    return out

  def _attach(self, raw, plan):
    """this buffer's place in the allocation `raw`: guards and buffer prefilled, `.t` the view"""
    self.name, self.shape, self.dtype, self.item, self.row_len, self.front, self.begin, self.end, self.back = plan
    self.raw = raw
    _fill(raw[self.front:self.back], self.dtype)
    self.t = raw[self.begin:self.end].view(self.dtype).view(self.shape)

  # ---- checks -------------------------------------------------------------------------------------------------------------
  def ptr(self):
    return self.t.data_ptr() if self.t.numel() else self.raw.data_ptr() + self.begin

  def _fail(self, side, what, offset):
    raise AssertionError("%s: %s, %s at element %d (row %d)" % (self.name, side, what, offset, offset // self.row_len))

  def check_guards(self):
    n = (self.end - self.begin) // self.item
    for side, a, b in (("front guard", self.front, self.begin), ("back guard", self.end, self.back)):
      bad = ~_is_sentinel(self.raw[a:b], self.dtype)
      if bool(bad.any()):
        first = int(bad.nonzero()[0])
        self._fail(side, "written", first - (self.begin - a) // self.item if side[0] == "f" else n + first)

  def _element_mask(self, defined):
    n = self.t.numel()
    rows = self.shape[0] if self.shape else 1
    m = torch.zeros(n, dtype=torch.bool, device=self.raw.device)
    if isinstance(defined, (int, np.integer)):
      assert 0 <= defined <= rows
      m[:int(defined) * self.row_len] = True
    elif isinstance(defined, slice):
      m.view(rows, -1)[defined] = True
    else:
      d = torch.as_tensor(defined, dtype=torch.bool).to(self.raw.device)
      if d.numel() == rows and d.dim() == 1:
        m.view(rows, -1)[d] = True
      else:
        assert d.numel() == n, "a mask covers the rows or the elements"
        m = d.reshape(-1).clone()
    return m

  def check(self, defined, rest_untouched=False):
    self.check_guards()
    if self.t.numel() == 0:
      return
    sent = _is_sentinel(self.raw[self.begin:self.end], self.dtype)
    m = self._element_mask(defined)
    bad = sent & m
    if bool(bad.any()):
      self._fail("buffer", "not written", int(bad.nonzero()[0]))
    if rest_untouched:
      bad = ~sent & ~m
      if bool(bad.any()):
        self._fail("buffer", "written outside the defined extent", int(bad.nonzero()[0]))


def check_all(guarded, defined, rest_untouched=False):
  for g, d in zip(guarded, defined):
    g.check(d, rest_untouched)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _bytes(t):
  return t.reshape(-1).view(torch.uint8)


class frozen:
  """with frozen(ids, grad=g): op(...)   — or   f = frozen(...); op(...); f.verify()"""

  def __init__(self, *tensors, **named):
    self.items = [("input[%d]" % i, t) for i, t in enumerate(tensors)] + list(named.items())
    self.items = [(k, t) for k, t in self.items if t is not None]
    for k, t in self.items:
      assert t.is_contiguous(), k
    self.snap = [_bytes(t).clone() for _, t in self.items]

  def verify(self):
    for (name, t), was in zip(self.items, self.snap):
      if t.is_cuda:
        torch.cuda.synchronize(t.device)
      bad = _bytes(t) != was
      if bool(bad.any()):
        at = int(bad.nonzero()[0]) // t.element_size()
        row_len = int(np.prod(t.shape[1:], dtype=np.int64)) if t.dim() > 1 else 1
        raise AssertionError("%s: input changed at element %d (row %d)" % (name, at, at // max(1, row_len)))

  def __enter__(self):
    return self

  def __exit__(self, kind, value, tb):
    if kind is None:
      self.verify()
    return False


# ---- values ----------------------------------------------------------------------------------------------------------------
def bits(x):
  """a tensor or array as a numpy array of unsigned integers of the element's width"""
  a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
  return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, name="out"):
  """bit for bit; where `want` is a float NaN (0/0: IEEE leaves sign and payload open), any NaN"""
  g, w = bits(got), bits(want)
  assert g.shape == w.shape, "%s: shape %s, expected %s" % (name, g.shape, w.shape)
  differ = g.reshape(-1) != w.reshape(-1)
  if isinstance(want, np.ndarray) and want.dtype == np.float32:
    differ &= ~(np.isnan(want).reshape(-1) & np.isnan(g.view(np.float32)).reshape(-1))
  bad = np.flatnonzero(differ)
  if bad.size:
    at = int(bad[0])
    row_len = int(np.prod(g.shape[1:], dtype=np.int64)) if g.ndim > 1 else 1
    raise AssertionError("%s: %d of %d elements differ, first at element %d (row %d): 0x%x, expected 0x%x" %
                         (name, bad.size, g.size, at, at // max(1, row_len), int(g.reshape(-1)[at]), int(w.reshape(-1)[at])))
