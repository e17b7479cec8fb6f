// Prints what the row-geometry header (tfplus_amd/csrc/kv_row_geom.h) selects for every dim 0..1028, one line per dim:
//   D  sorted  entry  fused_ok  row_lanes  with_lanes  with_lanes<256>  pow2_vectors(D, 64)  pow2_vectors(D, 256)
// sorted / entry: the V,LPR,K that with_row_geom hands the lambda in the sorted family (the whole float4 ladder and the
// scalar one) and in the entry family (float4 rungs up to ENTRY_MAX_Q), or - where it returns KV_UNIMPLEMENTED.  Then the
// checks: the lambda's value comes back unchanged, a dim without a class never reaches the lambda, the dispatch agrees with
// row_class, and the cap of with_lanes.  Built by tests/test_row_geometry.py with the host compiler and its sanitizers, the
// header alone.  Last line: ok, or one line per failed check; exit status: the number of failed checks.
#include "kv_row_geom.h"

#include <cstdio>
#include <initializer_list>

using namespace kvhip_internal;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static int calls = 0;

// the class the dispatch selects, encoded by the lambda as V * 1000000 + LPR * 1000 + K (never KV_UNIMPLEMENTED)
template <int MAX_Q, bool ALLOW_SCALAR>
static int selected(int D) {
  return with_row_geom<MAX_Q, ALLOW_SCALAR>(D, [&](auto g) -> int {
    ++calls;
    return decltype(g)::V * 1000000 + decltype(g)::LPR * 1000 + decltype(g)::K;
  });
}
static int encode(RowClass c) { return c.none() ? KV_UNIMPLEMENTED : c.V * 1000000 + c.LPR * 1000 + c.K; }
static void print_class(int code) {
  if (code == KV_UNIMPLEMENTED) std::printf(" -");
  else std::printf(" %d,%d,%d", code / 1000000, code / 1000 % 1000, code % 1000);
}
template <int CAP>
static int lanes_given(int lanes) {
  return with_lanes<CAP>(lanes, [](auto vq) { return (int)decltype(vq)::value; });
}

static_assert(row_class(32).V == 4 && row_class(32).LPR == 8 && row_class(32).K == 1, "row_class is usable in a static_assert");
static_assert(row_class(0).none() && row_class(257).none() && row_class(1028).none() && row_class(260, ENTRY_MAX_Q, false).none(), "");
static_assert(ENTRY_MAX_Q == 64, "");

int main() {
  for (int D = 0; D <= 1028; ++D) {
    const int before = calls;
    const int sorted = selected<SORTED_MAX_Q, true>(D), entry = selected<ENTRY_MAX_Q, false>(D);
    CHECK(calls - before == (sorted != KV_UNIMPLEMENTED) + (entry != KV_UNIMPLEMENTED));
    CHECK(sorted == encode(row_class(D)));
    CHECK(entry == encode(row_class(D, ENTRY_MAX_Q, false)));
    CHECK(fused_ok(D) == (entry != KV_UNIMPLEMENTED));
    std::printf("%d", D);
    print_class(sorted);
    print_class(entry);
    std::printf(" %d %d %d %d %d %d\n", (int)fused_ok(D), row_lanes(D), lanes_given<64>(row_lanes(D)),
                lanes_given<256>(row_lanes(D)), pow2_vectors(D, 64), pow2_vectors(D, 256));
  }
  // the lambda's value, whatever it is, comes back
  for (int v : {0, 7, -3, KV_UNIMPLEMENTED, KV_INTERNAL})
    for (int D : {1, 4, 36, 255, 1024}) CHECK((with_row_geom<SORTED_MAX_Q, true>(D, [&](auto) -> int { return v; })) == v);
  // a dim without a class: KV_UNIMPLEMENTED, the lambda not called
  int reached = 0;
  auto count = [&](auto) -> int { ++reached; return 0; };
  for (int D : {0, 257, 1028, -4}) CHECK((with_row_geom<SORTED_MAX_Q, true>(D, count)) == KV_UNIMPLEMENTED);
  for (int D : {0, 3, 257, 260, 1028, -4}) CHECK((with_row_geom<ENTRY_MAX_Q>(D, count)) == KV_UNIMPLEMENTED);
  CHECK(reached == 0);
  CHECK((with_row_geom<ENTRY_MAX_Q>(256, count)) == 0 && reached == 1);
  // with_lanes: a count that is no power of two, or one above the cap, gets the cap; the default cap is 64
  CHECK(lanes_given<64>(3) == 64 && lanes_given<64>(128) == 64 && lanes_given<256>(128) == 128 && lanes_given<256>(512) == 256);
  CHECK(with_lanes(32, [](auto vq) { return (int)decltype(vq)::value; }) == 32);
  CHECK(with_lanes(4096, [](auto vq) { return (int)decltype(vq)::value; }) == 64);
  if (!failures) std::printf("ok\n");
  return failures;
}
