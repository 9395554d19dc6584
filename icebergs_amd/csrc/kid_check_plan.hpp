// kid_check_plan.hpp -- the decisions of the debug invariants (kid_check_bergs, kid_check.inc) as plain C++17: no HIP header,
// no handle.  What "the same identity" and "the same berg" mean (sameid FW:4381-4393, sameberg FW:4397-4428), the key the radix
// passes sort by so that rows equal by value end up next to each other, and the number of pairs a group of rows holds.
// The kernels of kid_check.inc call all four; tests/check_plan_host.cpp holds them against values written out by hand.
// "Equal by value" is the Fortran `.ne.` negated: a NaN equals nothing, itself included, and -0.0 equals +0.0.
#pragma once
#include <cstdint>
#include "../../include/kid_types.h"

#if defined(__HIPCC__)
#define KID_CHK_HD __host__ __device__
#else
#define KID_CHK_HD
#endif

namespace kid {

// the five members sameid compares, in its order
struct CheckKeys { int32_t start_year; double start_day, start_mass, start_lon, start_lat; };
KID_CHK_HD inline bool check_same_keys(const CheckKeys &a, const CheckKeys &b) {
  if (a.start_year != b.start_year) return false;
  if (a.start_day != b.start_day) return false;
  if (a.start_mass != b.start_mass) return false;
  if (a.start_lon != b.start_lon) return false;
  if (a.start_lat != b.start_lat) return false;
  return true;
}

// The unsigned pattern a radix pass sorts a double by.  Two doubles that are equal by value get the same pattern, so rows equal
// in every key are neighbours after the passes: -0.0 is taken for +0.0 first (x + 0.0; otherwise (-0, a) and (+0, a) are parted by
// (-0, b)).  Numbers keep their order.  Every NaN gets the largest pattern: NaN rows come last, next to each other, and the
// compare by value that follows makes each of them a group of its own.
KID_CHK_HD inline uint64_t check_sort_key(double x) {
  if (x != x) return ~(uint64_t)0;
  const double c = x + 0.0;
  uint64_t u;
  __builtin_memcpy(&u, &c, sizeof(u));
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// pairs among m rows, m(m-1)/2, with the even factor halved first: exact for every m whose result fits 64 bits
KID_CHK_HD inline uint64_t check_pair_count(int64_t m) {
  if (m < 2) return 0;
  const uint64_t u = (uint64_t)m;
  return (u & 1ull) ? u * ((u - 1ull) >> 1) : (u >> 1) * (u - 1ull);
}

// the members sameberg compares beyond the keys: FW:4404-4419, and under mts FW:4422-4425
enum { CHECK_SAMEBERG_MEMBERS = 16, CHECK_SAMEBERG_MEMBERS_MTS = 20 };
KID_CHK_HD inline int check_sameberg_count(bool mts) { return mts ? CHECK_SAMEBERG_MEMBERS_MTS : CHECK_SAMEBERG_MEMBERS; }
KID_CHK_HD inline int check_sameberg_member(int s) {   // the KID_B_* of member s, in the reference's order; -1 beyond the list
  switch (s) {
    case 0: return KID_B_LON;
    case 1: return KID_B_LAT;
    case 2: return KID_B_MASS;
    case 3: return KID_B_UVEL;
    case 4: return KID_B_VVEL;
    case 5: return KID_B_THICKNESS;
    case 6: return KID_B_WIDTH;
    case 7: return KID_B_LENGTH;
    case 8: return KID_B_AXN;
    case 9: return KID_B_AYN;
    case 10: return KID_B_BXN;
    case 11: return KID_B_BYN;
    case 12: return KID_B_UVEL_OLD;
    case 13: return KID_B_VVEL_OLD;
    case 14: return KID_B_LON_OLD;
    case 15: return KID_B_LAT_OLD;
    case 16: return KID_B_AXN_FAST;
    case 17: return KID_B_AYN_FAST;
    case 18: return KID_B_BXN_FAST;
    case 19: return KID_B_BYN_FAST;
    default: return -1;
  }
}
// sameberg of rows a and b whose keys are already known to be equal: f[member][row]
KID_CHK_HD inline bool check_same_members(const double *const *f, long long a, long long b, bool mts) {
  const int n = check_sameberg_count(mts);
  for (int s = 0; s < n; ++s) {
    const double *p = f[check_sameberg_member(s)];
    if (p[a] != p[b]) return false;
  }
  return true;
}

}  // namespace kid
