// kv_mirror_epoch.h — the epoch of a (var, slot) pair's slot mirrors: which generation the copies in the var's rows belong
// to, whether a lean apply has written any since the last write-back, and how many epochs have ended.  Plain C++: a host
// compiler builds it alone (tests/c_abi/mirror_epoch_check.cc).  The pair's own mutex guards the record (kv_host.h
// MirrorPair); nothing here launches: end() says what the caller has to launch.
#pragma once

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// Invariants (every write is one of the two transitions, the members are private):
//   - the epoch is a number in 1 .. 0xFFFF, the 16 bits a copy on the device is stamped with; 0 is never an epoch (the
//     rows' mirror units start as zero bytes).
//   - a number that copies were stamped with (lean_apply returned it) is never handed out again before a clear_all: end()
//     moves on to a number no copy carries, and where it passes 0xFFFF it restarts at 1 and tells the caller to clear every
//     copy (clear_all).
//   - dirty <=> a lean apply has run since the last end(): the dirty copies all carry the CURRENT epoch, and that number —
//     captured before the bump — is the End::flush_epoch16 of the end() that reports them.
//   - after end() the record is clean.
class MirrorEpoch {
 public:
  // what the caller of end() launches: the write-back of the dirty copies stamped flush_epoch16 (flush), then the clearing
  // of every copy (clear_all: the number wrapped)
  struct End {
    bool flush;
    unsigned flush_epoch16;
    bool clear_all;
  };

  // a record whose first epoch is first_epoch16 (0: 1), ended_before epochs already counted: a var that leaves one pair and
  // joins another goes on where it stopped — its rows' mirror units still hold the old pair's copies, and only a number they
  // do not carry makes them void
  explicit MirrorEpoch(unsigned first_epoch16 = 1u, long long ended_before = 0)
      : epoch_((first_epoch16 & 0xFFFFu) ? (first_epoch16 & 0xFFFFu) : 1u), ended_(ended_before) {}

  // ---- transitions ----
  // a lean apply is about to be launched: its copies carry the returned epoch, some of them will be dirty
  unsigned lean_apply() { dirty_ = true; return epoch_; }
  // the epoch ends: every copy is void from here on (after the write-back the caller launches)
  End end() {
    End e{dirty_, epoch_, false};
    dirty_ = false;
    ++ended_;
    if (++epoch_ > 0xFFFFu) { epoch_ = 1u; e.clear_all = true; }
    return e;
  }

  // ---- reads ----
  unsigned epoch16() const { return epoch_; }
  bool dirty() const { return dirty_; }
  long long ended() const { return ended_; }

 private:
  unsigned epoch_;
  long long ended_;
  bool dirty_ = false;
};

}  // namespace kvhip_internal
