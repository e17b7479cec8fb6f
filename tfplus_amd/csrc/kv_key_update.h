// kv_key_update.h — what a kernel does to ONE key's state once the key's gradient sum is in registers (included after
// kv_device.h, before kv_kernels.h): the general path (resolve_rows / prefetch_state / finish_key: any table, any key), the
// lean path (LeanCtx / key_update: the var row's slot mirror stands), a new key's row (init_var_row).  k_papply and k_uapply
// call the lean path, k_apply / k_apply_fin the general one.  The one-round-trip prefetch in front of the update stays in
// the two bodies, written on LeanCtx: as a function of this file it spilled registers (profiles/key_update_kres.txt).
#pragma once

// lo16 = sat_add(lo16, min(count, 65535)) of a frequency word (find_func / insert_func kv_variable.h:320-363, AddFrequency
// :409-414).  The day field is the caller's: lookups and applies carry different days.
__device__ __forceinline__ unsigned freq_add_sat(unsigned word, unsigned count) {
  const unsigned lo = (word & 0xFFFFu) + (count > 65535u ? 65535u : count);
  return lo > 65535u ? 65535u : lo;
}

// The slot-table rows of one key, resolved by the group leader.  FindOrInsertUnsafe(var, filter_out !=
// nullptr) kv_variable.h:382-408 and FindOrInsertUnsafe(slot, nullptr) :409-414; FTRL probes linear
// before accum (training_ops.cc:701-704).  `m0` is the record of the hinted slot row (requested early).
struct RowsOf { unsigned tag, r0, r1, nb; };   // nb: bit 1 / 2 = slot row 0 / 1 inserted now, bit 3 = slot row 0 is the hinted one,
                                               // bit 4 / 5 (scatter_chain(OPT)) = the var / slot row is blacklisted
template <int OPT>
__device__ __forceinline__ RowsOf resolve_rows(const PartArgs& a, long long key, unsigned rvw, unsigned hint,
                                               bool hint_loaded, const RowMeta& m0) {
  const unsigned rv = rvw & ROW_MASK;
  const bool vnew = (rvw >> 31) != 0u;   // inserted by this apply: not filtered (kv_variable.h:400-407, succ == false)
  RowsOf o{rv, 0u, 0u, 0u};
  if (rv == 0u) return o;
  // the var record is only needed for the frequency filter: a blacklisted row is all zeros already
  // (RemoveBlacklistUnsafe hands out a zero row, table_manager.h:359-372) and the group optimizers
  // rewrite the flags after the update, so with enter_threshold == 0 they never read it
  const bool need_vmeta = keeps_var_flags(OPT) || a.tv.enter_threshold != 0u;
  bool vblack = false, sblack = false;
  if (scatter_chain(OPT)) {   // ScatterSub (kv_variable.h:616-734): no filter; a blacklisted row is skipped, not lifted
    if (!vnew) vblack = (load_freq_flags(a.tv, rv).y & FLAG_BLACK) != 0u;
  } else if (need_vmeta && !vnew) {
    const uint2 mv = load_freq_flags(a.tv, rv);
    if ((mv.x & 0xFFFFu) < a.tv.enter_threshold) { o.tag = rv | ROW_FILTERED; return o; }  // kv_variable.h:910
    if (mv.y & FLAG_BLACK) meta_ptr(a.tv, rv)->flags = FLAG_UNDER;   // RemoveBlacklistUnsafe: fresh zero row (ours already is)
  }
  // slot rows are only created for keys the update will touch (filtered keys returned above)
  bool hinted = false;
  auto slot_row = [&](const TableDev& t, bool use_hint, bool* isnew) -> unsigned {
    *isnew = false;
    unsigned r = 0, f = 0;
    if (use_hint && hint_loaded && m0.key == key && !(m0.flags & FLAG_FREE)) {
      r = hint; f = m0.freq; hinted = true;
      if (scatter_chain(OPT)) sblack = (m0.flags & FLAG_BLACK) != 0u;
    } else {
      r = table_find(t, key);
      if (__builtin_expect(r == 0u, 0)) {
        r = table_find_or_insert(t, key, isnew);
        // (scatter_chain: GatherOrInsert's insert_func stamps the day, kv_variable.h:339-363; FindOrInsertUnsafe's does not)
        if (r && *isnew) { RowMeta* m = meta_ptr(t, r); m->freq = scatter_chain(OPT) ? ((a.day << 16) | 1u) : 1u; m->flags = 0; }
      }
      if (scatter_chain(OPT)) {
        if (r && !*isnew) { const uint2 ff = load_freq_flags(t, r); f = ff.x; sblack = (ff.y & FLAG_BLACK) != 0u; }
      } else if (r && !*isnew) f = meta_ptr(t, r)->freq;
      if (use_hint && r) {   // remember it in the var's index entry
        Entry* e = table_entry_of(a.tv, key);
        if (e) e->hint = r;
      }
    }
    // AddFrequency(1, today) on a slot row that already existed (kv_variable.h:409-414); a new one keeps word 1
    if (r && !*isnew) *freq_ptr(t, r) = (a.day << 16) | freq_add_sat(f, 1u);
    return r;
  };
  bool new0 = false, new1 = false;
  if (two_slots(OPT)) o.r1 = slot_row(a.ts1, false, &new1);
  o.r0 = slot_row(a.ts0, a.use_hints != 0, &new0);
  // MarkAsDeltaListElements on every table of the op, for the keys the update reaches (training_ops.cc:7196-7201)
  if (__builtin_expect(a.tv.track_delta | a.ts0.track_delta | (two_slots(OPT) ? a.ts1.track_delta : 0u), 0)) {
    mark_delta(a.tv, rv);
    if (o.r0) mark_delta(a.ts0, o.r0);
    if (two_slots(OPT) && o.r1) mark_delta(a.ts1, o.r1);
  }
  o.nb = (new0 ? 2u : 0u) | (new1 ? 4u : 0u) | (hinted ? 8u : 0u);
  if (scatter_chain(OPT)) o.nb |= (vblack ? 16u : 0u) | (sblack ? 32u : 0u);
  return o;
}

// Everything the update of one key needs besides its gradient, requested in ONE round trip: the var row, the
// hinted slot row and that row's own record (the hint is validated against it in resolve_rows).  Without this the
// finish walks slot index -> slot record -> rows, three dependent hops.  Called by the LPR lanes of the key's group.
template <int OPT, int V, int LPR, int K>
__device__ __forceinline__ void prefetch_state(const PartArgs& a, const uint4& ra, bool live, int lane, int D, RowMeta& m0,
                                               bool& hint_loaded, PreRows<OPT, V, K>& pre, bool& have_x, bool& have_s) {
  hint_loaded = false; have_x = false; have_s = false;
  if (!live || (ra.z & ROW_MASK) == 0u) return;
  const bool hok = a.use_hints && ra.w != 0u && ra.w < a.ts0.max_rows;
  if (lane == 0 && hok) {
    const uint4 mm = *reinterpret_cast<const uint4*>(meta_ptr(a.ts0, ra.w));
    m0.key = (long long)(((unsigned long long)mm.y << 32) | mm.x);
    m0.freq = mm.z;
    m0.flags = (unsigned char)(mm.w & 0xFFu);
    hint_loaded = true;
  }
  const float* xr = row_ptr(a.tv, ra.z & ROW_MASK);
  const float* sr = hok ? row_ptr(a.ts0, ra.w) : nullptr;
  constexpr int NS0 = slot0_blocks(OPT);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (lane + k * LPR) * V;
    if (e0 < D) {
      ldv<V>(xr + e0, pre.x[k]);
      if (hok) {
#pragma unroll
        for (int b3 = 0; b3 < NS0; ++b3) ldv<V>(sr + e0 + b3 * D, pre.s[b3][k]);
      }
    }
  }
  have_x = true; have_s = hok;
}

// finish one key whose combined gradient is in gv: optimizer update (MODE_APPLY) or emit (MODE_DEDUP).
// All LPR lanes of every group of the wave call it (shuffles inside); `live` masks groups without a key.
// hd = {key lo, key hi, row word, slot-row hint}
template <int MODE, int OPT, int V, int LPR, int K>
__device__ __forceinline__ void finish_key(const PartArgs& a, const uint4 hd, bool live, bool hint_loaded,
                                           const RowMeta& m0, float (&gv)[K][V], int lane,
                                           const PreRows<OPT, V, K>* pre = nullptr, bool have_x = false, bool have_s = false) {
  const int D = a.tv.dim;
  const long long key = (long long)(((unsigned long long)hd.y << 32) | hd.x);
  if (MODE == MODE_APPLY) {
    RowsOf ro{0u, 0u, 0u, 0u};
    if (live && lane == 0) ro = resolve_rows<OPT>(a, key, hd.z, hd.w, hint_loaded, m0);
    if (LPR > 1) {
      ro.tag = __shfl(ro.tag, 0, LPR); ro.r0 = __shfl(ro.r0, 0, LPR);
      ro.r1 = __shfl(ro.r1, 0, LPR); ro.nb = __shfl(ro.nb, 0, LPR);
    }
    // the slot rows in `pre` are those of the hinted row: good only if the hint stood up
    opt_update_row<OPT, V, LPR, K>(a.tv, a.ts0, a.ts1, key, ro.tag, ro.r0, (ro.nb & 2u) != 0, ro.r1, (ro.nb & 4u) != 0,
                                   live, gv, a.opt, lane, pre, have_x, have_s && (ro.nb & 8u) != 0,
                                   scatter_chain(OPT) && (ro.nb & 16u) != 0, scatter_chain(OPT) && (ro.nb & 32u) != 0);
    // the key's slot record as this update left it goes into the var row's mirror (clean: the slot table's own record is
    // up to date), so that the key's NEXT apply takes the lean path without reading it
    if (!two_slots(OPT) && a.use_mirror && live && lane == 0 && ro.r0 != 0u && (ro.tag & ROW_MASK) != 0u && !(ro.tag & ROW_FILTERED)) {
      const uint2 sm = load_freq_flags(a.ts0, ro.r0);
      SlotMirror nm;
      nm.srow = ro.r0; nm.freq = sm.x; nm.flags = (unsigned char)(sm.y & 0xFFu); nm.state = (unsigned char)MIRROR_CLEAN;
      nm.epoch = (unsigned short)a.mirror_epoch; nm.pad = 0u;
      *mirror_ptr(a.tv, ro.tag & ROW_MASK) = nm;
    }
  } else if (live && hd.z != ROW_MASK) {
    const size_t orow = a.out_map ? (size_t)a.out_map[hd.z] : (size_t)hd.z;   // sharded apply: the unique id's exchange slot
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (lane + k * LPR) * V;
      if (e0 < D) stv<V>(a.out_sum + orow * D + e0, gv[k]);
    }
  }
}

// ---- the lean path ---------------------------------------------------------------------------------------------------------
// THE MIRROR INVARIANT.  The slot table's OWN record is current for every key whose mirror (the SlotMirror
// behind the var row's record) is not (valid in this epoch and MIRROR_DIRTY).  Device side, all of it in this file:
// finish_key leaves a CLEAN mirror behind every update it makes; key_update, for a key whose mirror is valid in this epoch
// and names the hinted slot row, updates frequency word and flags in the MIRROR only and marks it DIRTY.  Host side
// (kvhip.hip mirror_*): mirror_decide says per launch whether mirrors are used; any other op on the pair first ends the
// epoch (mirror_on_entry): the dirty mirrors are written back, then all are invalid at once.
// What the lean path needs of the launch, built once per kernel (the values are wave-uniform: scalar registers).
struct LeanCtx {
  bool fast;          // single-chunk tables, one slot table, hints, no delta lists, mirrors: else every key is general
  float* vrows;       // the var table's rows, records and the slot table's rows: chunk 0 is the whole slab
  RowMeta* vmeta;
  float* srows;
  int SD;             // floats per slot row
  unsigned smax, thr; // rows of the slot table; the var's enter_threshold
  bool need_vmeta;    // the var record decides something (resolve_rows)
  unsigned mepoch;
};
template <int OPT>
__device__ __forceinline__ LeanCtx lean_ctx(const PartArgs& a) {
  LeanCtx c;
  c.fast = !two_slots(OPT) && a.tv.single != 0u && a.ts0.single != 0u && a.use_hints != 0 &&
           (a.tv.track_delta | a.ts0.track_delta) == 0u && a.use_mirror != 0;
  c.vrows = a.tv.c0.rows;
  c.vmeta = a.tv.c0.meta;
  c.srows = a.ts0.c0.rows;
  c.SD = a.ts0.dim;
  c.smax = a.ts0.max_rows; c.thr = a.tv.enter_threshold;
  c.need_vmeta = keeps_var_flags(OPT) || c.thr != 0u;
  c.mepoch = a.mirror_epoch & 0xFFFFu;
  return c;
}

// A key inserted now (nk; the other groups pass through): the init rule's row (kv_variable.h:889-898) — the row the update
// starts from, and what the table holds if the update does not act — computed into x and stored.  Returns whether any
// element of the group's row has |x| >= CUTOFF (UpdateUnderThreshold); every lane of the wave calls it.
template <int V, int LPR, int K>
__device__ __forceinline__ bool init_var_row(const TableDev& t, long long key, unsigned row, bool nk, int D, const int (&eoff)[K],
                                             const bool (&evalid)[K], float (&x)[K][V]) {
  bool big = false;
  if (nk) {
    const float *ia, *ib;
    init_rule_rows(t, key, &ia, &ib, D);
    float* xrow = row_ptr(t, row);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float va_[V], vb_[V];
      ldv<V>(ia + eoff[k], va_);
      ldv<V>(ib + eoff[k], vb_);
#pragma unroll
      for (int cc = 0; cc < V; ++cc) {
        x[k][cc] = (va_[cc] + vb_[cc]) * 0.5f;
        big |= evalid[k] && fabsf(x[k][cc]) >= CUTOFF;
      }
      if (evalid[k]) stv<V>(xrow + eoff[k], x[k]);
    }
  }
  return group_any<LPR>(big);
}

// The lean update of one key (go: the group has one and nothing stopped it; vnew: the caller inserted it — never filtered,
// kv_variable.h:400-407), done here where the mirror stands.  Returns whether the key is still finish_key's; that call
// stays in the kernel's body (one inlining level further down a.tv's row pointer stays in scratch).
template <int OPT, int V, int LPR, int K>
__device__ __forceinline__ bool key_update(const PartArgs& a, const LeanCtx& c, unsigned row, unsigned hint, bool vnew, bool go,
                                           int lane, int D, float (&gv)[K][V], const uint2 vm, const uint4 mir,
                                           const PreRows<OPT, V, K>& pre) {
  if (!c.fast) return go;
  const unsigned hh = hint < c.smax ? hint : 0u;
  // the hint stands up: the var row's mirror stands for exactly that slot row in this epoch (established by finish_key
  // or by kv_attach_slot) — what resolve_rows checks against the slot row's own record
  const bool ok = go && row != 0u && hh != 0u && ((mir.z >> 8) & 0xFFu) != MIRROR_INVALID && (mir.z >> 16) == c.mepoch &&
                  mir.x == hh;
  const unsigned sfreq = mir.y;   // the slot row's frequency word
  bool act = ok;
  bool vblack = false, sblack = false;
  if (scatter_chain(OPT)) {   // no filter; blacklisted rows stay as they are (resolve_rows)
    vblack = ok && !vnew && (vm.y & FLAG_BLACK) != 0u;
    sblack = ok && (mir.z & FLAG_BLACK) != 0u;
  } else if (c.need_vmeta && ok && !vnew) {   // frequency filter / un-blacklisting (resolve_rows; kv_variable.h:910)
    if ((vm.x & 0xFFFFu) < c.thr) act = false;
    else if ((vm.y & FLAG_BLACK) && lane == 0) c.vmeta[(size_t)row * META_STRIDE].flags = FLAG_UNDER;
  }
  const unsigned rr = act ? row : 0u, h2 = act ? hh : 0u;
  SlotMirror* const mp = reinterpret_cast<SlotMirror*>(c.vmeta + (size_t)rr * META_STRIDE + 1);
  if (act && lane == 0) {   // AddFrequency(1, today) on the slot row (kv_variable.h:409-414)
    mp->freq = (a.day << 16) | freq_add_sat(sfreq, 1u);
    mp->state = (unsigned char)MIRROR_DIRTY;
  }
  opt_core<OPT, V, LPR, K>(c.vrows + (size_t)rr * D, c.srows + (size_t)h2 * c.SD, nullptr, &c.vmeta[(size_t)rr * META_STRIDE].flags,
                           &mp->flags, nullptr, act, false, D, gv, a.opt, lane, pre.x, pre.s, false, vblack, sblack);
  return go && !ok;
}
