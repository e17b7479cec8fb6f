// kv_types.h — the types libkvhip's translation units hand each other: the kernels' arguments and the launchers' parameters
// (kv_launch.h).  One definition in a named namespace, so that every unit sees the same types and the compiler checks the
// calls between units; hidden, so that none of it is exported.  The kernels and their device helpers stay in each unit's
// anonymous namespace (kv_device.h and the kernel headers).
#pragma once

#include <hip/hip_runtime.h>

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// index-pass modes (k_part_keys) and fold modes (k_apply_sorted)
enum Mode { MODE_LOOKUP = 0, MODE_APPLY = 1, MODE_DEDUP = 2, MODE_SCATTER = 3, MODE_MARK = 4, MODE_UNIQUE = 5,
            MODE_APPLYIDX = 6 };
enum Opt { OPT_ADAM_V4 = 0, OPT_ADAM_V3 = 1, OPT_ADAGRAD = 2, OPT_FTRL = 3, OPT_FTRL_V2 = 4, OPT_GROUP_FTRL_V2 = 5,
           OPT_GROUP_RADAM = 6, OPT_ADAM = 7 };
// What the pipelines ask of an optimizer, in one place (a new OPT_* must answer each of them):
// GroupAdam: one slot table of three dim-wide blocks (m | v | z)
constexpr bool group_adam(int opt) { return opt == OPT_ADAM_V4 || opt == OPT_ADAM_V3; }
// a second slot table (accum + linear): rows probed and inserted in ts1, no slot-mirror lean path (the mirror stands for
// ONE slot record)
constexpr bool two_slots(int opt) { return opt == OPT_FTRL || opt == OPT_FTRL_V2 || opt == OPT_GROUP_FTRL_V2; }
// no CoverUpdate of the var: its flags are read (blacklist lifted by RemoveBlacklistUnsafe) and left to a later lookup
constexpr bool keeps_var_flags(int opt) { return opt == OPT_ADAGRAD || opt == OPT_FTRL_V2; }
// plain Adam: the bookkeeping of the generic ops its reference composes (python/training/adam.py:93-163), GatherOrInsert
// and ScatterUpdate on the slot row, ScatterSub on the var (kv_variable.h:263-380, 616-734), not a training op's.  The var
// has no frequency filter and no CoverUpdate: a blacklisted row stays blacklisted and unwritten, any other row's flags are
// recomputed from the row written.  A slot row inserted now carries the day stamp (insert_func); a blacklisted one reads
// as zeros and is left unwritten
constexpr bool scatter_chain(int opt) { return opt == OPT_ADAM; }
// dim-wide blocks of the first slot row (group RectifiedAdam: m | v | linear | vhat | vamsgrad; Adam: m | v)
constexpr int slot0_blocks(int opt) { return opt == OPT_GROUP_RADAM ? 5 : group_adam(opt) ? 3 : opt == OPT_ADAM ? 2 : 1; }
// one wide slot table whose dim is a multiple of the var's (what the ops' initialisation and shape checks ask)
constexpr bool wide_slot(int opt) { return slot0_blocks(opt) > 1; }
// dim-wide blocks of optimizer state a key's update holds besides the var row: the first slot row's (the FTRL family's
// second slot table's row rides in block 1).  Three at the least: the existing optimizers' kernels keep the register
// allocation they were tuned with
constexpr int state_blocks(int opt) { return slot0_blocks(opt) > 3 ? slot0_blocks(opt) : 3; }

struct __attribute__((aligned(16))) Entry {
  long long key;
  unsigned row;
  unsigned hint;   // row of this key in the table's attached optimizer slot table (0 = not known yet); a
                   // hint is validated against the slot row's own key before use, so a stale one only costs a probe
};

// per-row metadata next to each other (one 16-byte record, so a key's frequency word and flags
// arrive with one memory transaction and an insert writes one line): embedding_value.h:225-235
struct RowMeta {
  long long key;
  unsigned freq;          // (day << 16) | saturating u16 count
  unsigned char flags;    // FLAG_*
  unsigned char delta;    // DELTA_TRAIN: key is in train_deltalist_ (kv_variable.h:870; set only while the table tracks
                          // deltas); DELTA_PRED: in prediction_deltalist_ (:871)
  unsigned short stamp;   // serial of the last kv_apply_*_unique launch that updated the row (kv_uapply.h: how an id that
                          // breaks the caller's promise of unique ids is caught); 0 = none
};
constexpr unsigned DELTA_TRAIN = 1u, DELTA_PRED = 2u;
static_assert(sizeof(RowMeta) == 16, "RowMeta layout");

// A row's record array holds META_STRIDE 16-byte units per row: [0] the RowMeta, [1] a SlotMirror — in the SAME 32-byte
// sector, so the two are one line to read and one request to write.  Every read miss on this chip is a 128-byte line
// (profiles/r06_fetch_calibration.txt): the optimizer apply used to read two lines per key for two 16-byte records — the
// var's and the hinted slot row's.  The mirror is a write-back copy of what the apply needs of the SLOT row's record (its
// frequency word and flags), kept next to the VAR row's record: while it is valid the apply neither reads nor writes the
// slot table's own record.  `srow` names the slot row it stands for (must equal the index entry's hint), `epoch` the
// generation of the pairing (the host bumps it — one integer — whenever anything but a mirror apply may have read or
// written the slot table's records, after flushing the dirty mirrors back: kvhip.hip mirror_*), `state` 0 invalid / 1 clean /
// 2 dirty.  Only var tables of an attached (var, slot) pair use their mirrors; the units exist in every table.
constexpr int META_STRIDE = 2;
struct SlotMirror {
  unsigned srow;          // the slot row this stands for
  unsigned freq;          // its frequency word (day << 16 | saturating count)
  unsigned char flags;    // its FLAG_* byte
  unsigned char state;    // MIRROR_*
  unsigned short epoch;   // pairing generation (PartArgs::mirror_epoch)
  unsigned pad;
};
static_assert(sizeof(SlotMirror) == 16, "SlotMirror layout");
constexpr unsigned MIRROR_INVALID = 0u, MIRROR_CLEAN = 1u, MIRROR_DIRTY = 2u;

struct Chunk {
  float* rows;
  RowMeta* meta;
};

// device view of one table; passed to kernels by value
struct TableDev {
  Chunk c0;                 // chunk 0 by value: the common single-chunk table needs no table hop
  Entry* entries;
  unsigned long long mask;  // cap - 1; entries[cap] = sentinel-key home
  Chunk* chunks;
  int chunk_bits;
  unsigned* counters;  // [0] next_row  [1] error flag (row overflow)  [2] (int) rows on the free list
  const unsigned* free_rows;  // rows released by Delete, popped by inserts (nullptr: none known)
  unsigned max_rows;
  const float* init_table;
  unsigned init_rows;
  int dim;
  unsigned enter_threshold;
  unsigned long long seed;
  unsigned track_delta;     // NeedDeltaInfo() kv_variable.h:816: touched keys are remembered for DeltaExport
  unsigned* err_host;       // pinned host copy of counters[1] (the host reads it without a synchronisation)
  unsigned single;          // the slab is chunk 0 alone (every pre-sized table): row addresses need no chunk-table hop —
                            // a UNIFORM test, so the loads behind it are not fenced by a per-lane branch
};

// device view of the per-batch workspace (kv_kernels.h explains the pipeline)
struct WsDev {
  long long* ent_key;      // [ntiles * TILE] tile t's deduplicated entries, sorted by partition
  unsigned* ent_a;         // index modes: occurrences of the key in the tile (low 16) | saturating frequency
                           // count of the tile (high 16); scatter / mark: one input position of the key
  unsigned* ent_b;         // OUT of the partition pass: var row id of the key (unique: dense index)
  unsigned* ent_base;      // OUT of the partition pass: where the entry's positions start in the sorted position
                           // list | HEAD_BIT (first entry of its key)
  unsigned* ent_rec;       // OUT of the partition pass, first entry of a key only: the key's record (list index,
                           // bit 31: hot list) — k_order files the key's first input position there
  unsigned* toff;          // [ntiles][P + 1] partition boundaries inside each tile: entry prefix (low 16) |
                           // position prefix (high 16)
  unsigned* slot_rank;     // [n] entry index of every input position | its rank among the key's occurrences
                           // in the tile << RANK_SHIFT
  unsigned* order;         // [n + 1] input positions sorted by key (a key's occurrences are contiguous), first
                           // one tagged HEAD_BIT; order[n] = HEAD_BIT
  uint4* coldlist;         // [n][2] KeyRec of the cold keys: {key lo, key hi, row, slot-row hint} {start, count, first position, -}
  uint4* hotlist;          // [n][2] the hot keys: ... {start, count, first chunk (in the partition), rows per chunk}
                           // (both indexed by the partition's first sorted position + the key's number in it)
  uint4* litem;            // [n] the partitions' work items, partition p's at [its first sorted position ...)
  uint4* pmeta;            // [P] per partition: {items, hot chunks, first sorted position, cold keys}
  uint4* items;            // [n] the dense work item directory (k_gather<ORDER> / k_order build it): hot chunk
                           // {hot list index | HEAD_BIT, chunk in the key, chunk number in the batch, -}, cold
                           // batch {first cold list index, keys, -, -}
  float* hpart;            // [hot chunks][dim] partial sums of the keys that have more than one chunk
  unsigned* ctr;           // [8] op counters, zeroed by the tile pass: [0] unique count (kv_unique / kv_dedup_segment_sum),
                           // [2] work items, [3] hot chunks
  unsigned ntiles, P;
  int pshift;              // 64 - log2(P)
  unsigned seg_cap;        // (id, count) input in fixed-capacity exchange segments of this many records (0: plain list)
  int* zero_counts;        // the tile pass clears this [n] array on its way (the sharded route's sparse unique counts); else null
  unsigned long long* dbg; // diagnostic build only (-DKV_STAMPS): per-block phase stamps
  // ---- the entry-list pipeline (kv_fused.h).  It reuses ent_b (row word), ent_base (slot-row hint), ent_rec (the
  //      entry's source: its input position, or EP_TAG | epart row), order (the entry list) and:
  unsigned* mrow;          // [n] per tile, the rows of its entries with more than one occurrence, entry by entry and in
                           // rank order: tile-local position (bits 0..10) | the entry's epart row in the tile (bits 11..20)
                           // | bit 31: first row of its entry  (in slot_rank's storage)
  unsigned* mcount;        // [ntiles] rows in mrow (low 16) | entries they belong to (high 16)
  float* epart;            // [ntiles][TILE / 2][dim] their gradient sums (k_tsum)
  // ---- sharded path: a rank's OWN segment of an exchange is not copied from the send to the receive buffer: the
  //      kernels that read a receive buffer read positions [self_lo, self_lo + self_len) from the send buffer instead
  unsigned self_lo, self_len;   // (length 0: no such range; one unsigned compare: pos - self_lo < self_len)
  const void* ids_self;         // k_ltile<IdCount>: the (id, count) records of that range (send_pairs)
  const float* grad_self;       // k_tsum / k_papply: its gradient rows (send_rows)
  unsigned short* pos_ent; // [n] k_ltile: every input position's entry number in its tile (sharded route: the finish reads
                           // position -> entry -> record); nullptr: not filed
};

// (Fields an optimizer's math has no use for carry that optimizer's own host scalars — the radam_* / adam_* accessors below:
// read l2s, lr_power and update_slots per optimizer, never for all of them.)
struct OptArgs {
  float lr, b1p, b2p, b1, b2, eps, l1, l2, l21, l2s, lr_power;
  float alpha, l21_norm;  // host-precomputed in fp32 exactly as the reference does (group RectifiedAdam: sqrt(1 - beta2_power); Adam: lr_t)
  int update_slots;
  int fast;               // row math on the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32 (kv_set_fast_math; 0: IEEE sequences)
};

// Group RectifiedAdam's own scalars ride in the fields its math has no use for.  OptArgs is part of every apply kernel's
// argument block and the older optimizers' kernels are kept instruction for instruction (tools/kres.sh): the struct
// stays as it is
constexpr int RADAM_TRACTABLE = 1, RADAM_AMSGRAD = 2, RADAM_NESTEROV = 4;
__host__ __device__ inline float& radam_r_t(OptArgs& a) { return a.l2s; }          // the rectification term r_t
__host__ __device__ inline float radam_r_t(const OptArgs& a) { return a.l2s; }
__host__ __device__ inline float& radam_c1(OptArgs& a) { return a.lr_power; }      // 1 - beta1_power
__host__ __device__ inline float radam_c1(const OptArgs& a) { return a.lr_power; }
__host__ __device__ inline int& radam_flags(OptArgs& a) { return a.update_slots; }  // RADAM_* bits
__host__ __device__ inline int radam_flags(const OptArgs& a) { return a.update_slots; }
// ... and plain Adam's: alpha carries lr_t = lr sqrt(1 - beta2_power) / (1 - beta1_power); 1 - beta1 and 1 - beta2 (host, fp32)
__host__ __device__ inline float& adam_omb1(OptArgs& a) { return a.l2s; }
__host__ __device__ inline float adam_omb1(const OptArgs& a) { return a.l2s; }
__host__ __device__ inline float& adam_omb2(OptArgs& a) { return a.lr_power; }
__host__ __device__ inline float adam_omb2(const OptArgs& a) { return a.lr_power; }

// arguments of the index / partition pass and the optimizer apply (kv_kernels.h: partition pass)
struct PartArgs {
  TableDev tv, ts0, ts1;      // var table; optimizer slot tables (apply)
  OptArgs opt;
  const float* grad;          // apply / dedup: input gradient rows; scatter: update rows
  unsigned day;
  int scatter_op, is_insert;  // MODE_SCATTER
  int mark_what;              // MODE_MARK: 0 = blacklist, 1 = frequency words (in fvals)
  const unsigned* fvals;
  long long* out_keys;        // MODE_UNIQUE
  float* out_sum;             // MODE_DEDUP fold: out_sum[row] = the key's sum
  const int* out_map;         // ... or out_sum[out_map[row]] when given
  int* out_counts;            // MODE_UNIQUE: occurrences (saturating) of each unique key
  int count_once;             // MODE_LOOKUP: frequency += 1 per unique key instead of per occurrence
  long long direct_rows;      // MODE_UNIQUE, > 0: keys ARE output row indices in [0, direct_rows)
                              // (tf.unsorted_segment_sum): no key list, no counter
  int use_hints;              // apply: ts0 is tv's attached slot table (Entry::hint names ts0's rows)
  int fold_op;                // MODE_DEDUP fold: KV_SCATTER_ADD (sum) / MUL (product) / MIN / MAX / ASSIGN (last)
  int det;                    // deterministic reduction mode
  int sparse_unique;          // MODE_UNIQUE: unique numbers = sorted position of the partition + local number (with gaps)
  long long n;                // ids in the batch
  const float* epart;         // entry-list pipeline: list words tagged EP_TAG name rows of this array (tile sums), else of grad
  unsigned day_lk;            // k_papply (kv_papply.h), PA_LOOKUP: the day stamp of the lookup whose bookkeeping it completes
  // k_papply PA_UNIQUE with route_world > 0 (sharded lookup route): every distinct id goes straight to its owner's segment
  int route_world, route_rule;     // owner_rank(id, world, rule)
  unsigned route_C;                // records per segment (header not counted)
  long long* route_seg;            // [world][C + 1][2] (id, count) records
  int* route_slot_of;              // [number] the record the id went to (0: no room)
  unsigned* route_overflow;        // pinned flag: a segment was too small
  unsigned* route_gcount;          // [MAXW + 1] records per owner so far; [MAXW]: blocks of the launch that are done
  unsigned* route_need;            // != nullptr: the LAST block of the launch writes the segments' headers, the largest segment
                                   // wanted (here) and clears the counters
  unsigned* route_uhint;           // pinned host word (may be null): the batch's distinct ids
  unsigned uniq_serial;            // k_uapply (kv_uapply.h): this launch's stamp (1 .. 65535)
  int use_mirror;                  // the lean update reads / writes the slot row's frequency word and flags in the var row's
  unsigned mirror_epoch;           // SlotMirror (kv_device.h) when it is valid for this epoch; the host flushes (kvhip.hip mirror_*)
  int dd_number;                   // k_papply PA_DEDUP: the pass numbers the distinct ids itself (dense, ctr[0]; out_keys[number] = id) —
                                   // kv_dedup_segment_sum in one partition pass instead of PA_UNIQUE's and then this one
};

// One op on many tables in one launch (blockIdx.y = table): the kernels' *_multi forms read their arguments from an array
// of these in device memory
struct MultiDesc {
  WsDev w;
  PartArgs a;            // a.tv is the table of this entry (lookup) / the var table (apply)
  const void* ids;
  const int* counts;
  float* out;            // lookup output rows
  long long n;
};
// The sharded sparse apply's pre-sum (kv_sums_seg.hip): the gradient arrives per SEGMENT, and the row of input position p is
// pscale[p] * seg_grad[pseg[p], :] — each element one multiply, the row kv_lookup_sparse_grad would have written.  The sum
// kernels' *_seg forms take this as an extra argument; WsDev, PartArgs and MultiDesc stay as the training step's kernels
// index them.
struct SegSrc {
  const float* seg_grad;   // [nseg, dim]
  const int* pseg;         // [n] the position's segment, clamped into [0, nseg)
  const float* pscale;     // [n] its scale (kv_op_kernels.h seg_scale)
};
// ... and per table of a batched launch, next to the MultiDesc array (as SparseDesc sits next to it in the sparse lookups):
// what the sum kernels read (src) and what the pre-pass that writes the position records reads and writes
struct SegDesc {
  SegSrc src;
  const void* seg;         // [n] segment ids (one dtype for the whole call)
  const float* wts;        // [n] or null
  unsigned* off;           // [nseg + 1] the route table's Workspace::seg_off
  float* den;              // [nseg] its Workspace::seg_den (weighted mean / sqrtn)
  int* pseg;               // [n] OUT: Workspace::pseg
  float* pscale;           // [n] OUT: Workspace::pscale
  long long n, nseg;
};

// k_papply's modes (kv_papply.h explains them): the `mode` of launch_papply / launch_papply_ud
enum PaMode { PA_LOOKUP = 0, PA_APPLYIDX = 1, PA_NONE = 2, PA_UNIQUE = 3, PA_DEDUP = 4,
              PA_DEDUP_NUM = 5 };   // (a template constant only: PA_DEDUP that numbers the ids itself — kv_dedup_segment_sum)

}  // namespace kvhip_internal
