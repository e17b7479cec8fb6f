// Walks MirrorEpoch (tfplus_amd/csrc/kv_mirror_epoch.h) through its transitions and checks what end() reports after each:
// built by tests/test_mirror_epoch.py with the host compiler and its sanitizers, the header alone.  Exit status: the number
// of failed checks; one line per failure.
#include "kv_mirror_epoch.h"

#include <cstdio>

using kvhip_internal::MirrorEpoch;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// `steps` epoch ends from `m` on, a lean apply in front of every third: clear_all exactly on the bump that passes 0xFFFF,
// where the counter restarts at 1; no flush_epoch16 is 0; consecutive epochs differ modulo 2^16; a flush carries the
// number the lean apply was given.  Returns how many wraps it saw.
static int walk(MirrorEpoch& m, long steps) {
  int wraps = 0;
  for (long k = 0; k < steps; ++k) {
    const unsigned before = m.epoch16();
    const long long ended = m.ended();
    const bool apply = k % 3 == 0;
    unsigned stamped = 0u;
    if (apply) {
      stamped = m.lean_apply();
      CHECK(stamped == before);
      CHECK(m.dirty());
    }
    const MirrorEpoch::End e = m.end();
    CHECK(e.flush == apply);
    CHECK(e.flush_epoch16 == before);
    CHECK(e.flush_epoch16 != 0u && e.flush_epoch16 <= 0xFFFFu);
    if (apply) CHECK(e.flush_epoch16 == stamped);
    CHECK(e.clear_all == (before == 0xFFFFu));
    if (e.clear_all) { CHECK(m.epoch16() == 1u); ++wraps; }
    else CHECK(m.epoch16() == before + 1u);
    CHECK((m.epoch16() & 0xFFFFu) != (before & 0xFFFFu));
    CHECK(m.epoch16() != 0u && m.epoch16() <= 0xFFFFu);
    CHECK(!m.dirty());
    CHECK(m.ended() == ended + 1);
  }
  return wraps;
}

int main() {
  {  // 1. the plain cycle
    MirrorEpoch m;
    CHECK(!m.dirty());
    CHECK(m.epoch16() == 1u);
    CHECK(m.ended() == 0);
    const unsigned e0 = m.lean_apply();
    CHECK(e0 == m.epoch16());
    CHECK(m.dirty());
    CHECK(m.lean_apply() == e0);   // (a second lean apply of the same epoch: the same stamp)
    const MirrorEpoch::End e = m.end();
    CHECK(e.flush);
    CHECK(e.flush_epoch16 == e0);
    CHECK(!e.clear_all);
    CHECK(!m.dirty());
    CHECK(m.epoch16() != e0);
    CHECK(m.ended() == 1);
  }
  {  // 2. end() on a clean record: no flush, the epoch still advances, ended() counts it
    MirrorEpoch m;
    const unsigned e0 = m.epoch16();
    const MirrorEpoch::End e = m.end();
    CHECK(!e.flush);
    CHECK(!e.clear_all);
    CHECK(m.epoch16() != e0);
    CHECK(m.ended() == 1);
    CHECK(!m.dirty());
  }
  {  // 3. two end() calls back to back (the two sides of a pair, serialised): exactly one reports the flush, with the
     //    number the copies carry
    MirrorEpoch m;
    m.end();
    const unsigned stamped = m.lean_apply();
    const MirrorEpoch::End a = m.end(), b = m.end();
    CHECK(a.flush != b.flush);
    CHECK(a.flush && a.flush_epoch16 == stamped);
    CHECK(b.flush_epoch16 != stamped);
    CHECK(m.ended() == 3);
  }
  {  // 4. the wrap, from near the top ...
    MirrorEpoch m(0xFFFAu);
    CHECK(m.epoch16() == 0xFFFAu);
    CHECK(walk(m, 12) == 1);
    CHECK(m.epoch16() == 7u);
    CHECK(m.ended() == 12);
    // ... a first epoch of 0xFFFF wraps at its first end; 0 is no epoch
    MirrorEpoch top(0xFFFFu);
    top.lean_apply();
    const MirrorEpoch::End e = top.end();
    CHECK(e.flush && e.flush_epoch16 == 0xFFFFu && e.clear_all);
    CHECK(top.epoch16() == 1u);
    CHECK(MirrorEpoch(0u).epoch16() == 1u);
    // ... and one full walk: 65 535 ends from 1 pass 0xFFFF exactly once and arrive at 1 again
    MirrorEpoch full;
    CHECK(walk(full, 65535) == 1);
    CHECK(full.epoch16() == 1u);
    CHECK(full.ended() == 65535);
  }
  {  // 5. continuation: a record started at another record's next epoch goes on with its numbering (and its count)
    MirrorEpoch a;
    a.end();
    const unsigned stamped = a.lean_apply();
    a.end();   // (the var leaves its pair: the epoch ends)
    MirrorEpoch b(a.epoch16(), a.ended());
    CHECK(!b.dirty());
    CHECK(b.epoch16() == a.epoch16());
    CHECK(b.epoch16() != stamped);
    CHECK(b.ended() == 2);
    CHECK(b.lean_apply() != stamped);
    const MirrorEpoch::End e = b.end();
    CHECK(e.flush && e.flush_epoch16 == a.epoch16());
    CHECK(b.epoch16() == a.epoch16() + 1u);
    CHECK(b.ended() == 3);
  }
  if (failures == 0) std::printf("ok\n");
  return failures;
}
