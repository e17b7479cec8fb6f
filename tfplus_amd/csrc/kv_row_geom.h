// kv_row_geom.h — the row geometry of a table's dim, stated once: which kernel instantiation (V, LPR, K) — vector width,
// lanes per row, vectors per lane — a dim runs in the apply and sum kernels, and the lane counts and predicates of the
// row-copy kernels.  Every launcher that dispatches on a dim does it through with_row_geom / with_lanes below (kv_kernels.h
// launch_apply_t, kv_papply.h, kv_uapply.h, kv_sums.hip; kvhip.hip, kv_ops.hip and kv_shard.hip for the row copies).
// Plain C++17: a host compiler builds it alone (tests/c_abi/row_geom_check.cc prints what it selects for every dim).
#pragma once

#include <type_traits>

#include "../../include/kvhip.h"

#ifdef __HIP__
#define KV_ROW_GEOM_HD __host__ __device__
#else
#define KV_ROW_GEOM_HD
#endif

namespace __attribute__((visibility("hidden"))) kvhip_internal {

// a kernel's row-geometry template arguments, as with_row_geom hands them to a launcher's lambda
template <int V_, int LPR_, int K_>
struct RowGeom { static constexpr int V = V_, LPR = LPR_, K = K_; };
// ... and as a value (row_class): V == 0: the dim has no class
struct RowClass {
  int V, LPR, K;
  constexpr bool none() const { return V == 0; }
};

// ---- the table ------------------------------------------------------------------------------------------------------------
// A rung serves the rows of up to TOP vectors (float4 rows: q = D / 4 float4; scalar rows, D % 4 != 0: D floats) that no
// earlier rung serves.
template <int TOP, int V, int LPR, int K>
struct Rung {};
template <class... R>
struct Ladder {};
using Float4Ladder = Ladder<Rung<1, 4, 1, 1>, Rung<2, 4, 2, 1>, Rung<4, 4, 4, 1>,
                            // (k_papply at dim 32 with 4 lanes x 2 vectors or 2 x 4 per key — 16 / 32 keys per wave and
                            // step: 102 / 177 us against 62.7)
                            Rung<8, 4, 8, 1>,
                            Rung<16, 4, 8, 2>,    // dims 36..64: 8 lanes x 2 float4
                            Rung<32, 4, 16, 2>,   // dims 68..128: 16 lanes x 2 float4
                            Rung<64, 4, 64, 1>, Rung<128, 4, 64, 2>, Rung<256, 4, 64, 4>>;
using ScalarLadder = Ladder<Rung<1, 1, 1, 1>, Rung<2, 1, 2, 1>, Rung<4, 1, 4, 1>, Rung<8, 1, 8, 1>, Rung<16, 1, 16, 1>,
                            Rung<32, 1, 32, 1>, Rung<64, 1, 64, 1>, Rung<128, 1, 64, 2>, Rung<256, 1, 64, 4>>;
constexpr int SORTED_MAX_Q = 256;   // k_apply / k_apply_fin (sorted positions): the whole float4 ladder and the scalar one
constexpr int ENTRY_MAX_Q = 64;     // the entry-list kernels (k_papply, k_uapply, k_tsum, k_ltsum, k_papply_dedup): float4 only
constexpr int SCALAR_MAX_D = 256;

// ---- the table as a value: row_class(D) of the sorted family, row_class(D, ENTRY_MAX_Q, false) of the entry family ----------
template <int... TOP, int... V, int... LPR, int... K>
constexpr RowClass ladder_class(Ladder<Rung<TOP, V, LPR, K>...>, int x, int max_x) {
  RowClass c{0, 0, 0};
  (void)((x <= TOP && TOP <= max_x ? (c = RowClass{V, LPR, K}, true) : false) || ...);
  return c;
}
constexpr RowClass row_class(int D, int max_q = SORTED_MAX_Q, bool allow_scalar = true) {
  if (D < 1) return RowClass{0, 0, 0};
  if ((D & 3) == 0) return ladder_class(Float4Ladder{}, D / 4, max_q);
  return allow_scalar ? ladder_class(ScalarLadder{}, D, SCALAR_MAX_D) : RowClass{0, 0, 0};
}

// ---- the table as a dispatch ------------------------------------------------------------------------------------------------
// with_row_geom<MAX_Q, ALLOW_SCALAR>(D, f): f(RowGeom<V, LPR, K>{}) for the class of D, and f's int; KV_UNIMPLEMENTED, f not
// called, for a D without a class in the family (D < 1, D / 4 > MAX_Q, D % 4 != 0 without ALLOW_SCALAR).  MAX_Q and
// ALLOW_SCALAR are compile-time: f is instantiated for the family's rungs alone, in the table's order, so a launcher
// instantiates the kernels of its own family and no others.  f is a generic lambda, called directly (a chain of compares, as
// the hand-written ladders were).
template <int MAX_TOP, class F>
int ladder_dispatch(Ladder<>, int, F&) { return KV_UNIMPLEMENTED; }
template <int MAX_TOP, class F, int TOP, int V, int LPR, int K, class... R>
int ladder_dispatch(Ladder<Rung<TOP, V, LPR, K>, R...>, int x, F& f) {
  if constexpr (TOP <= MAX_TOP) {
    if (x <= TOP) return f(RowGeom<V, LPR, K>{});
  }
  return ladder_dispatch<MAX_TOP>(Ladder<R...>{}, x, f);
}
template <int MAX_Q, bool ALLOW_SCALAR = false, class F>
int with_row_geom(int D, F&& f) {
  if (D < 1) return KV_UNIMPLEMENTED;
  if ((D & 3) == 0) return ladder_dispatch<MAX_Q>(Float4Ladder{}, D / 4, f);
  if constexpr (ALLOW_SCALAR) return ladder_dispatch<SCALAR_MAX_D>(ScalarLadder{}, D, f);
  return KV_UNIMPLEMENTED;
}

// dims the entry-list pipeline (kv_fused.h) serves: every multiple of 4 up to 256 (rows of dim / 4 float4; a row's lane group
// is the next power of two, the lanes past the row's end masked: dims 12, 20, 100 ... run the same kernels as 16, 32, 128)
constexpr bool fused_ok(int D) { return !row_class(D, ENTRY_MAX_Q, false).none(); }

// lanes that share one row in the apply kernels, by dim: 64 / lanes keys ride side by side in a wave = the cold batch the
// partition pass forms (device code, kv_kernels.h part_keys_body: the ladder's LPR, restated as compares)
KV_ROW_GEOM_HD constexpr int apply_lanes(int D) {
  if ((D & 3) == 0) {
    const int q = D / 4;
    return q <= 1 ? 1 : q <= 2 ? 2 : q <= 4 ? 4 : q <= 16 ? 8 : q <= 32 ? 16 : 64;
  }
  return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
}
constexpr bool apply_lanes_match_the_ladders() {
  for (int D = 1; D <= 4 * SORTED_MAX_Q; ++D)
    if (!row_class(D).none() && apply_lanes(D) != row_class(D).LPR) return false;
  return true;
}
static_assert(apply_lanes_match_the_ladders(), "apply_lanes(D) != row_class(D).LPR: the partition pass's cold batches and the apply disagree");

// ---- the row-copy kernels ---------------------------------------------------------------------------------------------------
// lanes per row of the row-copy kernels: dim / 4 rounded up to a power of two
constexpr int row_lanes(int D) {
  int p = 1;
  while (p < D / 4) p <<= 1;
  return p;
}
// f(std::integral_constant<int, VQ>) for a row of `lanes` lanes (row_lanes: a power of two): the VQ template argument of
// the row-copy kernels, 1 .. CAP (more lanes, or a count that is no power of two: CAP)
template <int CAP = 64, int L = 1, class F>
auto with_lanes(int lanes, F&& f) {
  if constexpr (L >= CAP) {
    return f(std::integral_constant<int, CAP>{});
  } else {
    if (lanes == L) return f(std::integral_constant<int, L>{});
    return with_lanes<CAP, 2 * L>(lanes, f);
  }
}
// a float4 row with a power-of-two vector count up to max_q: that count (a lane group holds the row exactly), else 0
constexpr int pow2_vectors(int D, int max_q) {
  const int q = D / 4;
  return ((D & 3) == 0 && q >= 1 && q <= max_q && (q & (q - 1)) == 0) ? q : 0;
}

}  // namespace kvhip_internal
