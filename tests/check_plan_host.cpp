// The decisions of the debug invariants (icebergs_amd/csrc/kid_check_plan.hpp: sameid FW:4381, sameberg FW:4397, the sort key of
// the radix passes, the pairs of a group) on the host, against values written out by hand: +-0, a NaN in each key, groups of 1, 2,
// 3, 65 and 100 000 rows, and the 16 / 20 members of sameberg with one differing at a time.  count_groups() below is the pipeline
// of kid_check.inc in plain C++ -- sort by the key patterns, compare with the predecessor by value, add up the pairs of each group
// -- so the pieces are held together the way the kernels use them.  Plain C++17 with its own main (tests/test_check_cpu.py builds
// it with the address and undefined-behaviour sanitizers); no GPU, no HIP.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../icebergs_amd/csrc/kid_check_plan.hpp"

using namespace kid;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Counts { uint64_t pairs, extra, groups; };   // the sum of m(m-1)/2, the sum of (m - 1), the number of groups
static Counts count_groups(const std::vector<CheckKeys> &rows) {
  using Pattern = std::array<uint64_t, 5>;
  std::vector<size_t> order(rows.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = k;
  auto pattern = [&rows](size_t k) {
    const CheckKeys &r = rows[k];
    return Pattern{(uint64_t)((int64_t)r.start_year + 0x80000000ll), check_sort_key(r.start_day), check_sort_key(r.start_mass), check_sort_key(r.start_lon), check_sort_key(r.start_lat)};
  };
  std::stable_sort(order.begin(), order.end(), [&pattern](size_t a, size_t b) { return pattern(a) < pattern(b); });
  Counts c{0, 0, 0};
  int64_t m = 0;
  for (size_t q = 0; q < order.size(); ++q) {
    const bool head = q == 0 || !check_same_keys(rows[order[q]], rows[order[q - 1]]);
    if (head) { c.pairs += check_pair_count(m); c.groups += 1; m = 0; }
    else c.extra += 1;
    ++m;
  }
  c.pairs += check_pair_count(m);
  return c;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const CheckKeys base{1990, 12.5, 3.0e9, -61.25, -70.5};

  // ---- equality by value ----
  CHECK(check_same_keys(base, base));
  { CheckKeys o = base; o.start_year = 1991; CHECK(!check_same_keys(base, o)); }
  { CheckKeys o = base; o.start_day = 12.500000000000002; CHECK(!check_same_keys(base, o)); }     // one ulp
  { CheckKeys o = base; o.start_mass = 3.0000000000000005e9; CHECK(!check_same_keys(base, o)); }
  { CheckKeys o = base; o.start_lon = -61.25000000000001; CHECK(!check_same_keys(base, o)); }
  { CheckKeys o = base; o.start_lat = -70.50000000000001; CHECK(!check_same_keys(base, o)); }
  { CheckKeys a = base, b = base; a.start_lon = -0.0; b.start_lon = 0.0; CHECK(check_same_keys(a, b)); }   // -0.0 .ne. +0.0 is false
  // a NaN in each key: the row equals nothing, itself included
  { CheckKeys o = base; o.start_day = nan; CHECK(!check_same_keys(o, o) && !check_same_keys(base, o)); }
  { CheckKeys o = base; o.start_mass = nan; CHECK(!check_same_keys(o, o) && !check_same_keys(o, base)); }
  { CheckKeys o = base; o.start_lon = nan; CHECK(!check_same_keys(o, o)); }
  { CheckKeys o = base; o.start_lat = nan; CHECK(!check_same_keys(o, o)); }

  // ---- the sort key: the patterns written out ----
  CHECK(check_sort_key(0.0) == 0x8000000000000000ull);
  CHECK(check_sort_key(-0.0) == 0x8000000000000000ull);                 // taken for +0.0
  CHECK(check_sort_key(1.0) == 0xbff0000000000000ull);
  CHECK(check_sort_key(-1.0) == 0x400fffffffffffffull);
  CHECK(check_sort_key(inf) == 0xfff0000000000000ull);
  CHECK(check_sort_key(-inf) == 0x000fffffffffffffull);
  CHECK(check_sort_key(nan) == 0xffffffffffffffffull);
  CHECK(check_sort_key(-nan) == 0xffffffffffffffffull);                 // whatever its sign and payload
  CHECK(check_sort_key(std::nan("0x123")) == 0xffffffffffffffffull);
  {  // numbers keep their order, every NaN comes last
    const double asc[] = {-inf, -1.0e300, -2.5, -5.0e-324, 0.0, 5.0e-324, 1.0, 1.0000000000000002, 1.0e300, inf};
    for (size_t k = 0; k + 1 < sizeof(asc) / sizeof(asc[0]); ++k) CHECK(check_sort_key(asc[k]) < check_sort_key(asc[k + 1]));
    CHECK(check_sort_key(inf) < check_sort_key(nan));
  }

  // ---- pairs of a group ----
  CHECK(check_pair_count(-3) == 0 && check_pair_count(0) == 0 && check_pair_count(1) == 0);
  CHECK(check_pair_count(2) == 1 && check_pair_count(3) == 3 && check_pair_count(65) == 2080);
  CHECK(check_pair_count(100000) == 4999950000ull);                     // beyond 32 bits
  CHECK(check_pair_count(4294967296ll) == 9223372034707292160ull);      // 2^32 rows: 2^31 (2^32 - 1), the product before halving would not fit
  CHECK(check_pair_count(4294967297ll) == 9223372039002259456ull);      // odd m: (2^32 + 1) 2^31

  // ---- groups of 1, 2, 3, 65 and 100 000 rows, shuffled together ----
  {
    std::vector<CheckKeys> rows;
    const int sizes[5] = {1, 2, 3, 65, 100000};
    for (int g = 0; g < 5; ++g)
      for (int k = 0; k < sizes[g]; ++k) { CheckKeys r = base; r.start_day = 1.0 + g; rows.push_back(r); }
    uint64_t s = 12345;   // a fixed shuffle
    for (size_t k = rows.size() - 1; k > 0; --k) { s = s * 6364136223846793005ull + 1442695040888963407ull; std::swap(rows[k], rows[(size_t)((s >> 33) % (k + 1))]); }
    const Counts c = count_groups(rows);
    CHECK(c.groups == 5);
    CHECK(c.pairs == 0 + 1 + 3 + 2080 + 4999950000ull);
    CHECK(c.extra == 0 + 1 + 2 + 64 + 99999);
  }
  {  // (-0, a), (+0, a) with (-0, b) between them in the order of the raw bit patterns: one pair, which a key without x + 0.0 loses
    CheckKeys p = base, q = base, r = base;
    p.start_lon = -0.0; p.start_lat = 10.0;
    q.start_lon = 0.0; q.start_lat = 10.0;
    r.start_lon = -0.0; r.start_lat = 20.0;
    const Counts c = count_groups({p, r, q});
    CHECK(c.pairs == 1 && c.extra == 1 && c.groups == 2);
  }
  {  // two rows with a NaN start_mass and otherwise equal keys: two groups, no pair -- and they do not part the pair around them
    CheckKeys p = base, q = base;
    p.start_mass = nan; q.start_mass = nan;
    const Counts c = count_groups({base, p, q, base});
    CHECK(c.pairs == 1 && c.extra == 1 && c.groups == 3);
  }
  { const Counts c = count_groups({}); CHECK(c.pairs == 0 && c.extra == 0 && c.groups == 0); }
  { const Counts c = count_groups({base}); CHECK(c.pairs == 0 && c.extra == 0 && c.groups == 1); }

  // ---- the members of sameberg ----
  CHECK(check_sameberg_count(false) == 16 && check_sameberg_count(true) == 20);
  {
    const int want[20] = {KID_B_LON, KID_B_LAT, KID_B_MASS, KID_B_UVEL, KID_B_VVEL, KID_B_THICKNESS, KID_B_WIDTH, KID_B_LENGTH, KID_B_AXN, KID_B_AYN,
                          KID_B_BXN, KID_B_BYN, KID_B_UVEL_OLD, KID_B_VVEL_OLD, KID_B_LON_OLD, KID_B_LAT_OLD, KID_B_AXN_FAST, KID_B_AYN_FAST, KID_B_BXN_FAST, KID_B_BYN_FAST};
    for (int s = 0; s < 20; ++s) CHECK(check_sameberg_member(s) == want[s]);
    CHECK(check_sameberg_member(20) == -1 && check_sameberg_member(-1) == -1);
    // two rows equal in every field; then one member differing at a time
    std::vector<std::array<double, 2>> store(KID_NB_F64);
    std::vector<const double *> f(KID_NB_F64);
    for (int k = 0; k < KID_NB_F64; ++k) { store[k] = {1.5 + k, 1.5 + k}; f[k] = store[k].data(); }
    CHECK(check_same_members(f.data(), 0, 1, false) && check_same_members(f.data(), 0, 1, true));
    for (int s = 0; s < 20; ++s) {
      double &x = store[want[s]][1];
      const double keep = x;
      x = std::nextafter(keep, 1.0e9);
      CHECK(check_same_members(f.data(), 0, 1, false) == (s >= 16));     // the *_fast members count under mts only
      CHECK(!check_same_members(f.data(), 0, 1, true));
      x = nan;
      CHECK(!check_same_members(f.data(), 0, 1, true));
      x = keep;
    }
    // a member outside the list changes nothing; -0.0 equals +0.0; a NaN on both sides is a difference
    store[KID_B_XI][1] = 99.0;
    CHECK(check_same_members(f.data(), 0, 1, true));
    store[KID_B_UVEL] = {0.0, -0.0};
    CHECK(check_same_members(f.data(), 0, 1, true));
    store[KID_B_UVEL] = {nan, nan};
    CHECK(!check_same_members(f.data(), 0, 1, false));
  }

  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
