// kv_batch_index.h — what a table remembers of its last batch's index, so that the optimizer apply of the same ids (the one
// handed the batch's token) takes the index over instead of building it again.  Plain C++: a host compiler builds it alone
// (tests/c_abi/batch_index_check.cc).  The table's mutex guards the record like the rest of kv_table.
#pragma once

#include <cstdint>

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// Invariants (between two ops of the table; every write is one of the transitions, the members are private):
//   - serial == 0  <=>  the workspace holds no batch index: no token is valid, n, kind and P say nothing (drop zeroes them).
//     A table whose rows were released, whose workspace moved or whose pipeline changed holds none.
//   - serial != 0: the workspace holds the index of exactly the batch of n ids that `serial` names, of one kind: the tiles'
//     entries (ENTRIES: kv_fused.h, an apply of that batch goes through k_papply) or a sorted position list (SORTED:
//     kv_kernels.h).  A token that is not the serial is stale.
//   - P != 0 only while an ENTRIES index is held: the partitions its apply must use.
//   - A pending partition pass belongs to a held ENTRIES index: it is the bookkeeping of the lookup that published it.
//     Nothing here launches, so the ops keep that: an op drops only a table it entered with settle (or after
//     settle_pending), and a lookup that defers its pass publishes in the same op.  (The report of a deferred device error
//     drops before it settles: the pass then stays pending for the table's next op, which no token reaches any more —
//     except the report of a refused batch, code 2, which launches the pass before it sweeps: kvhip.hip rollback_refused.)
class BatchIndex {
 public:
  enum Kind : unsigned char { ENTRIES, SORTED };
  // how the apply handed (token, n) gets its index
  enum Plan {
    REBUILD,        // no valid token: the apply indexes the ids itself
    TAKE_PENDING,   // the held entries, and the lookup's partition pass with them (k_papply PA_LOOKUP)
    TAKE_DONE,      // the held entries, their bookkeeping is done (PA_NONE)
    TAKE_SORTED,    // the held sorted positions
  };

  // ---- transitions ----
  // the workspace holds no batch index, every token is stale
  void drop() { serial_ = 0; n_ = 0; P_ = 0; }
  // the workspace now holds the index of exactly this batch (serial: the caller's ++g_serial); returns the serial, the
  // batch's token.  P: the partitions of an ENTRIES index.
  uint64_t publish(uint64_t serial, long long n, Kind kind, unsigned P) {
    serial_ = serial; n_ = n; kind_ = kind; P_ = kind == ENTRIES ? P : 0u;
    return serial;
  }
  void defer_part() { pending_ = true; }     // the lookup's partition pass waits for the table's next op
  void part_taken() { pending_ = false; }    // the apply of that batch completes it inside k_papply
  void part_flushed() { pending_ = false; }  // it has been launched

  // ---- reads ----
  bool names(uint64_t token) const { return token != 0 && token == serial_; }
  bool holds(uint64_t token, long long n) const { return names(token) && n == n_; }
  bool part_pending() const { return pending_; }
  unsigned P() const { return P_; }
  // entry_list_dim: the entry-list kernels serve the table (fused_tab / fused_ok) — tiles' entries are of use to no other
  Plan plan(uint64_t token, long long n, bool entry_list_dim) const {
    if (!holds(token, n)) return REBUILD;
    if (kind_ == SORTED) return TAKE_SORTED;
    if (!entry_list_dim) return REBUILD;
    return pending_ ? TAKE_PENDING : TAKE_DONE;
  }
  static bool takes_entries(Plan p) { return p == TAKE_PENDING || p == TAKE_DONE; }

 private:
  uint64_t serial_ = 0;
  long long n_ = 0;
  unsigned P_ = 0;
  Kind kind_ = SORTED;
  bool pending_ = false;
};

}  // namespace kvhip_internal
