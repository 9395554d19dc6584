// Host-side check of the cold-field rule of icebergs_amd/csrc/kid_rows_plan.hpp (ColdIn, step_touches_f64 / _i32, cold_set,
// origin_compose): the rule over every combination of its inputs against its statement in words, restated here as literals, and
// the composition of `origin` over sequences of permutations against the rows moved one permutation at a time.
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_cold_rows_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../icebergs_amd/csrc/kid_rows_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);  \
      std::printf(__VA_ARGS__);                                       \
      std::printf("\n");                                              \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

typedef unsigned long long u64;
constexpr u64 bit(int f) { return 1ull << f; }
// config 2 (plain namelist, RK4, nothing optional): what DESIGN section 4 lists as carried along for nothing, and the members
// of the MTS / DEM path
constexpr kid::ColdIn C2{true, true, false, false, false, false, false};
static_assert(kid::cold_set(C2).id && kid::cold_set(C2).i32 == ((1u << KID_BI_START_YEAR) | (1u << KID_BI_N_BONDS) | (1u << KID_BI_CONGLOM_ID)), "constexpr");
static_assert(kid::cold_set(kid::ColdIn{false, true, false, false, false, false, false}).empty(), "nothing is cold outside the plain fused step");
static_assert(!kid::cold_set(C2).empty(), "a fusable handle defers something");

// the rule in words.  Never cold: what berg_kernel loads at its head or stores for a berg it steps -- position, velocity,
// accelerations, in-cell coordinates, size, mass_scaling, bits, heat density, the stored environment, the cell, alive.
static void check_rule() {
  const u64 always_touched = bit(KID_B_LON) | bit(KID_B_LAT) | bit(KID_B_UVEL) | bit(KID_B_VVEL) | bit(KID_B_MASS) | bit(KID_B_THICKNESS) | bit(KID_B_WIDTH) |
                             bit(KID_B_LENGTH) | bit(KID_B_AXN) | bit(KID_B_AYN) | bit(KID_B_BXN) | bit(KID_B_BYN) | bit(KID_B_MASS_SCALING) | bit(KID_B_MASS_OF_BITS) |
                             bit(KID_B_HEAT_DENSITY) | bit(KID_B_XI) | bit(KID_B_YJ) | bit(KID_B_UO) | bit(KID_B_VO) | bit(KID_B_UI) | bit(KID_B_VI) | bit(KID_B_UA) |
                             bit(KID_B_VA) | bit(KID_B_SSH_X) | bit(KID_B_SSH_Y) | bit(KID_B_SST) | bit(KID_B_SSS) | bit(KID_B_CN) | bit(KID_B_HI) | bit(KID_B_OD);
  const u64 never_touched = bit(KID_B_START_LON) | bit(KID_B_START_LAT) | bit(KID_B_AXN_FAST) | bit(KID_B_AYN_FAST) | bit(KID_B_BXN_FAST) | bit(KID_B_BYN_FAST) |
                            bit(KID_B_ANG_VEL) | bit(KID_B_ANG_ACCEL) | bit(KID_B_ROT);
  int nonempty = 0;
  for (int bits = 0; bits < 128; ++bits) {
    const bool fusable = bits & 1, rk = bits & 2, reentry = bits & 4, has_static = bits & 8, has_fl = bits & 16, bonds = bits & 32, by_class = bits & 64;
    const kid::ColdIn s{fusable, rk, reentry, has_static, has_fl, bonds, by_class};
    const kid::ColdSet c = kid::cold_set(s);
    if (!fusable) { CHECK(c.empty() && c.bytes_per_row() == 0, "bits %d: a handle that is not fusable defers nothing", bits); continue; }
    ++nonempty;
    CHECK(!c.empty() && c.id, "bits %d: a fusable handle defers at least the id", bits);
    u64 want = never_touched;
    if (rk) want |= bit(KID_B_UVEL_PREV) | bit(KID_B_VVEL_PREV);
    if (!reentry) want |= bit(KID_B_UVEL_OLD) | bit(KID_B_VVEL_OLD) | bit(KID_B_LON_OLD) | bit(KID_B_LAT_OLD);
    if (!has_static) want |= bit(KID_B_HALO_BERG) | bit(KID_B_STATIC_BERG);
    if (!has_fl) want |= bit(KID_B_MASS_OF_FL_BITS) | bit(KID_B_MASS_OF_FL_BERGY_BITS) | bit(KID_B_FL_K) | bit(KID_B_START_DAY);
    if (!by_class) want |= bit(KID_B_START_MASS);
    CHECK(c.f64 == want, "bits %d: fp64 cold set %llx, the rule in words gives %llx", bits, c.f64, want);
    CHECK((c.f64 & always_touched) == 0ull, "bits %d: a field the step loads or stores is cold", bits);
    unsigned want4 = 1u << KID_BI_CONGLOM_ID;
    if (!has_fl) want4 |= 1u << KID_BI_START_YEAR;
    if (!bonds) want4 |= 1u << KID_BI_N_BONDS;
    CHECK(c.i32 == want4, "bits %d: int32 cold set %x, the rule in words gives %x", bits, c.i32, want4);
    CHECK(!(c.i32 & ((1u << KID_BI_INE) | (1u << KID_BI_JNE) | (1u << KID_BI_ALIVE))), "bits %d: the cell or alive is cold", bits);
    // origin takes the place of a cold int32 field among the head copies of the re-binning instance (four slots; the cell is not one)
    int moving4 = 0;
    for (int f = 0; f < KID_NB_I32; ++f) if (f != KID_BI_INE && f != KID_BI_JNE && !((c.i32 >> f) & 1u)) ++moving4;
    CHECK(moving4 + 1 <= 4, "bits %d: %d moving int32 fields and origin do not fit four head copies", bits, moving4);
    int bytes = 8;
    for (int f = 0; f < KID_NB_F64; ++f) bytes += ((want >> f) & 1ull) ? 8 : 0;
    for (int f = 0; f < KID_NB_I32; ++f) bytes += ((want4 >> f) & 1u) ? 4 : 0;
    CHECK(c.bytes_per_row() == bytes, "bits %d: %d bytes per row, counted %d", bits, c.bytes_per_row(), bytes);
    // within: a set holds against itself and against a larger one, not against a smaller one
    CHECK(c.within(c) && kid::ColdSet{}.within(c), "bits %d: within", bits);
    kid::ColdIn t = s; t.melt_by_class = true;
    CHECK(kid::cold_set(t).within(c), "bits %d: switching the diagnostic on can only shrink the set", bits);
    if (!by_class) CHECK(!c.within(kid::cold_set(t)), "bits %d: start_mass deferred, then read: the deferred set must not hold", bits);
    t = s; t.periodic_reentry = true;
    if (!reentry) CHECK(!c.within(kid::cold_set(t)), "bits %d: *_old deferred, then written: the deferred set must not hold", bits);
    t = s; t.fusable = false;
    CHECK(!c.within(kid::cold_set(t)), "bits %d: a handle that stops being fusable holds no deferred set", bits);
  }
  CHECK(nonempty == 64, "%d", nonempty);
  // not a field: touched (never cold)
  CHECK(kid::step_touches_f64(C2, -1) && kid::step_touches_f64(C2, KID_NB_F64) && kid::step_touches_i32(C2, -1) && kid::step_touches_i32(C2, KID_NB_I32), "out of range");
  // config 2: the 68 bytes per row of the twelve head copies that no step reads (the issue's list without mass_scaling and alive),
  // and whatever else the population carries
  const kid::ColdSet c2 = kid::cold_set(C2);
  const u64 listed = bit(KID_B_START_LON) | bit(KID_B_START_LAT) | bit(KID_B_START_DAY) | bit(KID_B_START_MASS) | bit(KID_B_LON_OLD) | bit(KID_B_LAT_OLD);
  CHECK((c2.f64 & listed) == listed, "config 2");
}

// origin over a sequence of permutations: moving a cold field once through the composed origin gives the rows that moving it
// with every permutation gives
static void check_compose() {
  unsigned long long seed = 88172645463325252ull;
  auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  for (long long n : {1ll, 2ll, 63ll, 64ll, 65ll, 257ll, 1000ll}) {
    std::vector<double> cold((size_t)n), eager((size_t)n), next((size_t)n);
    for (long long k = 0; k < n; ++k) cold[(size_t)k] = eager[(size_t)k] = 1000.5 + (double)k;
    std::vector<int32_t> origin((size_t)n), origin_alt((size_t)n);
    std::iota(origin.begin(), origin.end(), 0);
    long long rows = n;   // a permutation may keep fewer rows (the dead tail dropped): destination rows [0, rows)
    for (int pass = 0; pass < 5; ++pass) {
      std::vector<unsigned> perm((size_t)rows);
      std::iota(perm.begin(), perm.end(), 0u);
      for (long long k = rows - 1; k > 0; --k) std::swap(perm[(size_t)k], perm[(size_t)(rnd() % (unsigned long long)(k + 1))]);
      const long long kept = (pass == 2 && rows > 3) ? rows - rows / 4 : rows;
      kid::origin_compose(origin.data(), perm.data(), kept, origin_alt.data());
      std::swap(origin, origin_alt);
      for (long long k = 0; k < kept; ++k) next[(size_t)k] = eager[perm[(size_t)k]];
      std::swap(eager, next);
      rows = kept;
      for (long long k = 0; k < rows; ++k) {
        CHECK(origin[(size_t)k] >= 0 && origin[(size_t)k] < n, "n %lld pass %d row %lld: origin %d out of the rows it was planned on", n, pass, k, origin[(size_t)k]);
        CHECK(cold[(size_t)origin[(size_t)k]] == eager[(size_t)k], "n %lld pass %d row %lld", n, pass, k);
      }
    }
    // materialise: one gather, then the identity
    std::vector<double> mat((size_t)rows);
    for (long long k = 0; k < rows; ++k) mat[(size_t)k] = cold[(size_t)origin[(size_t)k]];
    CHECK(std::equal(mat.begin(), mat.end(), eager.begin()), "n %lld: the gathered rows", n);
  }
}

int main() {
  check_rule();
  check_compose();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
