// Walks ShardBatch (tfplus_amd/csrc/kv_shard_batch.h) through its transitions, next to the two BatchIndex records its tokens
// come from (the route table's and the owner table's), and checks its reads after each: built by tests/test_shard_batch.py with
// the host compiler and its sanitizers, the two headers alone.  Exit status: the number of failed checks; one line per failure.
#include "kv_shard_batch.h"
#include "kv_batch_index.h"

#include <cstdio>
#include <initializer_list>

using kvhip_internal::BatchIndex;
using kvhip_internal::ShardBatch;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

int main() {
  const long long n = 300, nrec = 2 * (64 + 1);   // a batch's ids; the records of the owner's receive buffer
  uint64_t serial = 6;                            // the library's ++g_serial
  BatchIndex route, owner;                        // the route table's record and the owner table's
  {  // 1. a fresh record holds nothing and refuses no apply
    ShardBatch b;
    CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
    CHECK(b.n() == 0 && b.route_token() == 0 && b.serve_token() == 0);
    CHECK(b.may_apply());
    CHECK(!b.own_segment_stays());
    route.publish(++serial, 0, BatchIndex::ENTRIES, 64);   // (no index of another shard's batch is taken for its own)
    CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
  }
  ShardBatch b;
  // 2. route of n > 0: nothing holds until the index is published, then both do — until another op republishes the record
  b.begin_route(n);
  CHECK(b.n() == n && b.route_token() == 0);
  CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
  b.route_published(route.publish(++serial, n, BatchIndex::ENTRIES, 128));
  CHECK(b.route_token() == serial);
  CHECK(b.route_holds(route) && b.route_holds_ids(route));
  route.publish(++serial, n, BatchIndex::ENTRIES, 128);   // another route of as many ids on the same route table
  CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
  route.drop();
  CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
  // 3. routed-empty: the finish that writes segments may follow, the ones that need ids may not
  b.begin_route(0);
  b.route_voided();
  b.routed_empty();
  CHECK(b.n() == 0 && b.route_token() == 0);
  CHECK(b.route_holds(route) && !b.route_holds_ids(route));
  // 4. voided but not empty-routed (a failed or refused route of n ids): neither — and a later empty route is told apart
  b.begin_route(n);
  b.route_voided();
  CHECK(b.n() == 0 && b.route_token() == 0);
  CHECK(!b.route_holds(route) && !b.route_holds_ids(route));
  b.begin_route(0);
  b.route_voided();
  b.routed_empty();
  CHECK(b.route_holds(route));
  b.begin_route(n);   // (a new route ends the empty one)
  CHECK(!b.route_holds(route));
  b.route_published(route.publish(++serial, n, BatchIndex::ENTRIES, 128));
  CHECK(b.route_holds(route) && b.route_holds_ids(route));
  // 5. a read-only serve: no serve token and no apply, whatever else happens, until the next route
  b.serve_begins();
  b.served(owner.publish(++serial, nrec, BatchIndex::ENTRIES, 64));
  CHECK(b.may_apply() && b.serve_token() == serial);
  b.served_read_only();
  CHECK(!b.may_apply() && b.serve_token() == 0);
  CHECK(b.route_holds_ids(route));   // (the route index is the read-only batch's own)
  b.serve_begins();
  CHECK(!b.may_apply());
  b.served(0);
  b.route_published(b.route_token());
  b.exchanged_by_library(true);
  b.exchanged_by_caller();
  CHECK(!b.may_apply());
  b.begin_route(n);
  CHECK(b.may_apply());
  b.served_read_only();
  CHECK(!b.may_apply());
  b.route_voided();   // (the void route of a failed training route is a new route too)
  CHECK(b.may_apply());
  // 6. the serve token is the owner table's: it names the batch until the owner table's serial moves
  b.begin_route(n);
  b.route_published(route.publish(++serial, n, BatchIndex::ENTRIES, 128));
  b.serve_begins();
  CHECK(b.serve_token() == 0 && !owner.holds(b.serve_token(), nrec));
  const uint64_t t = owner.publish(++serial, nrec, BatchIndex::ENTRIES, 64);
  b.served(t);
  CHECK(b.serve_token() == t && owner.holds(b.serve_token(), nrec));
  b.begin_route(n);   // the next batch: its route leaves the serve token, its serve republishes the owner's record
  b.route_published(route.publish(++serial, n, BatchIndex::ENTRIES, 128));
  CHECK(b.serve_token() == t);
  owner.publish(++serial, nrec, BatchIndex::ENTRIES, 64);
  CHECK(!owner.holds(b.serve_token(), nrec));   // stale: the serial moved
  CHECK(owner.plan(b.serve_token(), nrec, true) == BatchIndex::REBUILD);
  b.serve_begins();
  CHECK(b.serve_token() == 0);
  // 7. the caller's exchange clears own_segment_stays whatever it was
  for (bool before : {false, true}) {
    b.exchanged_by_library(before);
    CHECK(b.own_segment_stays() == before);
    b.exchanged_by_caller();
    CHECK(!b.own_segment_stays());
  }
  if (failures == 0) std::printf("ok\n");
  return failures;
}
