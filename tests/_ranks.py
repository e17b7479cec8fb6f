"""Ranks as threads of one process: the transport of the sharded whole ops in the GPU tests (tests/test_gpu_shard_lookup_zeros.py,
tests/test_gpu_fuzz_sharded.py).  Every rank has a KvCommStaged whose callbacks move the segments between the ranks' buffers
on the one device; a barrier with a timeout keeps a rank that failed from leaving the others waiting.

Destructors.  A staged communicator sits in reference cycles (the communicator, its ctypes callbacks, the closures, this
object), so only the cyclic collector would free it: at a time and on a thread nobody chooses — also on a rank thread, inside
an exchange callback, while the other ranks are inside library calls — and what then runs is kv_comm_destroy (a stream
synchronisation, every live table's lock, the staging slots).  Neither happens here: run() keeps the collector off while the
rank threads live, and close() destroys the communicators on the caller's thread and breaks the cycles."""
import gc
import threading

import torch


class Ranks(object):
  """`world` staged communicators whose callbacks move the segments between the ranks' buffers on the device (the transport
  of test_whole_ops_with_ranks_as_threads_match_one_unsharded_table: a rank's own segment is never delivered)."""

  def __init__(self, ops, world, timeout=60):
    self.ops, self.world = ops, world
    self.bar = threading.Barrier(world, timeout=timeout)
    sent, vals, dev = [None] * world, [0] * world, torch.device("cuda", 0)

    def make(r):
      def exchange(send, recv, per_peer):
        n = per_peer * world
        sent[r] = ops.KvCommStaged.raw(send, n, dev)
        torch.cuda.synchronize()
        self.bar.wait()
        dst = ops.KvCommStaged.raw(recv, n, dev)
        for p in range(world):
          if p == r and per_peer != 32:
            dst[p * per_peer:(p + 1) * per_peer].fill_(0xA5)
          else:
            dst[p * per_peer:(p + 1) * per_peer].copy_(sent[p][r * per_peer:(r + 1) * per_peer])
        torch.cuda.synchronize()
        self.bar.wait()

      def max_u32(v):
        vals[r] = v
        self.bar.wait()
        m = max(vals)
        self.bar.wait()
        return m
      return ops.KvCommStaged(0, world=world, rank=r, exchange=exchange, max_u32=max_u32)
    self.comms = [make(r) for r in range(world)]

  def run(self, fn):
    """fn(rank, comm) on every rank at once; the results by rank"""
    outs, errs = [None] * self.world, []

    def body(r):
      try:
        torch.cuda.set_device(0)
        outs[r] = fn(r, self.comms[r])
        torch.cuda.synchronize()
      except Exception as e:   # a rank that fails breaks the barrier: the others fail too instead of waiting
        errs.append((r, repr(e)))
        self.bar.abort()
    ts = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
    collecting = gc.isenabled()
    gc.disable()                 # no destructor of anybody's garbage on a rank thread in the middle of an op
    try:
      for t in ts:
        t.start()
      for t in ts:
        t.join()
    finally:
      if collecting:
        gc.enable()
    assert not errs, errs
    self.bar.reset()
    return outs

  def close(self):
    """destroys the communicators now, on this thread, and breaks their reference cycles (nothing may be in flight)"""
    torch.cuda.synchronize()
    for c in self.comms:
      c.__del__()                # kv_comm_destroy; the handle is cleared, so the collector's own call is a no-op
      c._cb = None
    self.comms = []
