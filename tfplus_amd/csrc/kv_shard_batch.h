// kv_shard_batch.h — what a shard remembers of the batch it last routed and served, so that the finish, the gradient pre-sum
// and the owner's apply of that batch find the indexes its route and its serve left behind.  Plain C++: a host compiler builds
// it alone (tests/c_abi/shard_batch_check.cc).  The caller orders a shard's phases; nothing here locks.
#pragma once
#include "kv_batch_index.h"

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// Invariants (between two phases of the shard; every write is one of the transitions, the members are private):
//   - n: the ids of the batch last routed; a voided route (failed, refused or empty) leaves n == 0.
//   - route token != 0  =>  n > 0: the token the ROUTE table's BatchIndex published that batch's index under.  Whether the
//     index is still there is the BatchIndex's to say (another route republishes it): route_holds, route_holds_ids.
//   - empty_routed: the last route was of an EMPTY batch the caller asked for, not a voided one — a finish with segments to
//     write may follow it.  Exclusive with a route token: it implies n == 0 and token == 0.
//   - read_only_last: the last served batch was a read-only one, whose route overwrote the route index of the training batch
//     before it: no apply may follow.  Cleared only by a new route (begin_route, route_voided).
//   - The serve token is valid only for the batch the route token names: the OWNER table's BatchIndex published it in that
//     batch's serve.  A new route leaves it; the next serve voids it first, and until then the owner table's serial decides.
//   - own_segment_stays (this rank's own segments are read from the send buffers, no copy in the exchange) may change only
//     before a batch's first exchange — or after a lossless grow, before the batch is routed again.
class ShardBatch {
 public:
  // ---- transitions ----
  // a new batch of n ids is being routed: whoever serves it says what it is
  void begin_route(long long n) { n_ = n; route_token_ = 0; empty_routed_ = false; read_only_last_ = false; }
  void route_voided() { begin_route(0); }         // nothing to send (failed, refused or empty): void headers went out
  void routed_empty() { empty_routed_ = true; }   // ... and the caller's batch WAS empty
  void route_published(uint64_t token) { route_token_ = token; }
  void serve_begins() { serve_token_ = 0; }       // the owner's serve: what it fails to publish is not there
  void served(uint64_t token) { serve_token_ = token; }
  void served_read_only() { serve_token_ = 0; read_only_last_ = true; }   // marked whatever happens to the serve
  void exchanged_by_caller() { own_stays_ = false; }   // the phase calls: every segment arrives in the receive buffers
  void exchanged_by_library(bool can_stay) { own_stays_ = can_stay; }   // the whole ops
  // ---- reads ----
  long long n() const { return n_; }
  uint64_t route_token() const { return route_token_; }
  uint64_t serve_token() const { return serve_token_; }
  bool own_segment_stays() const { return own_stays_; }
  bool may_apply() const { return !read_only_last_; }
  // route: the ROUTE table's record.  It holds the index of the batch last routed, ids and all; or that batch was empty
  bool route_holds_ids(const BatchIndex& route) const { return n_ > 0 && route.holds(route_token_, n_); }
  bool route_holds(const BatchIndex& route) const { return n_ > 0 ? route_holds_ids(route) : empty_routed_; }
 private:
  long long n_ = 0;
  uint64_t route_token_ = 0, serve_token_ = 0;
  bool empty_routed_ = false, read_only_last_ = false, own_stays_ = false;
};

}  // namespace kvhip_internal
