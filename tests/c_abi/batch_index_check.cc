// Walks BatchIndex (tfplus_amd/csrc/kv_batch_index.h) through its transitions and checks plan() and holds() after each:
// built by tests/test_batch_index.py with the host compiler and its sanitizers, the header alone.  Exit status: the number
// of failed checks; one line per failure.
#include "kv_batch_index.h"

#include <cstdio>
#include <initializer_list>

using kvhip_internal::BatchIndex;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// every (token, n, dim) combination asks for a rebuild
static void check_all_rebuild(const BatchIndex& b, uint64_t token, long long n) {
  for (uint64_t t : {uint64_t(0), token, token + 1})
    for (long long m : {0ll, n, n + 1})
      for (bool dim : {false, true}) {
        CHECK(b.plan(t, m, dim) == BatchIndex::REBUILD);
        CHECK(!b.holds(t, m));
      }
}

int main() {
  const long long n = 3000;
  {  // 1. a fresh record
    BatchIndex b;
    check_all_rebuild(b, 7, n);
    CHECK(!b.part_pending());
    CHECK(b.P() == 0u);
    CHECK(!b.names(0));
  }
  BatchIndex b;
  // 2. publish entry-list, then defer: the pass is pending
  const uint64_t tok = b.publish(7, n, BatchIndex::ENTRIES, 128);
  CHECK(tok == 7);
  CHECK(b.holds(tok, n));
  CHECK(b.P() == 128u);
  CHECK(b.plan(tok, n, true) == BatchIndex::TAKE_DONE);   // (not deferred yet)
  b.defer_part();
  CHECK(b.part_pending());
  CHECK(b.plan(tok, n, true) == BatchIndex::TAKE_PENDING);
  CHECK(BatchIndex::takes_entries(b.plan(tok, n, true)));
  // 5. a wrong token   6. a right token with the wrong n   7. token 0 — all while the pass is pending
  CHECK(b.plan(tok + 1, n, true) == BatchIndex::REBUILD);
  CHECK(!b.holds(tok + 1, n));
  CHECK(b.plan(tok, n - 1, true) == BatchIndex::REBUILD);
  CHECK(!b.holds(tok, n - 1));
  CHECK(b.names(tok));   // (the serial alone still matches)
  CHECK(b.plan(0, n, true) == BatchIndex::REBUILD);
  CHECK(!b.holds(0, n));
  CHECK(!b.names(0));
  // (tiles' entries are of use only to the entry-list kernels)
  CHECK(b.plan(tok, n, false) == BatchIndex::REBUILD);
  // 3. after part_flushed: the pass is done, the index stays
  b.part_flushed();
  CHECK(!b.part_pending());
  CHECK(b.plan(tok, n, true) == BatchIndex::TAKE_DONE);
  CHECK(b.holds(tok, n));
  CHECK(b.P() == 128u);
  // 4. after part_taken: likewise
  b.defer_part();
  CHECK(b.plan(tok, n, true) == BatchIndex::TAKE_PENDING);
  b.part_taken();
  CHECK(!b.part_pending());
  CHECK(b.plan(tok, n, true) == BatchIndex::TAKE_DONE);
  CHECK(b.plan(tok + 1, n, true) == BatchIndex::REBUILD);
  CHECK(b.plan(tok, n + 1, true) == BatchIndex::REBUILD);
  CHECK(b.plan(0, n, true) == BatchIndex::REBUILD);
  // 10. a second publish makes the first token stale
  const uint64_t tok2 = b.publish(9, n, BatchIndex::ENTRIES, 256);
  CHECK(tok2 == 9);
  CHECK(!b.holds(tok, n));
  CHECK(b.plan(tok, n, true) == BatchIndex::REBUILD);
  CHECK(b.plan(tok2, n, true) == BatchIndex::TAKE_DONE);
  CHECK(b.P() == 256u);
  // 8. publish sorted-position: the positions are taken whatever the dim, and P reads 0
  const uint64_t tok3 = b.publish(11, n, BatchIndex::SORTED, 512);
  CHECK(b.plan(tok3, n, false) == BatchIndex::TAKE_SORTED);
  CHECK(b.plan(tok3, n, true) == BatchIndex::TAKE_SORTED);
  CHECK(!BatchIndex::takes_entries(b.plan(tok3, n, true)));
  CHECK(b.holds(tok3, n));
  CHECK(b.P() == 0u);
  CHECK(b.plan(tok2, n, true) == BatchIndex::REBUILD);
  CHECK(b.plan(tok3, n + 1, false) == BatchIndex::REBUILD);
  CHECK(b.plan(0, n, false) == BatchIndex::REBUILD);
  // 9. after drop(): everything gives rebuild — from a sorted-position index and from an entry-list one
  b.drop();
  check_all_rebuild(b, tok3, n);
  CHECK(b.P() == 0u);
  b.publish(13, n, BatchIndex::ENTRIES, 64);
  b.drop();
  check_all_rebuild(b, 13, n);
  CHECK(b.P() == 0u);
  if (failures == 0) std::printf("ok\n");
  return failures;
}
