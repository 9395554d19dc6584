// Host-side check of icebergs_amd/csrc/kid_rows_plan.hpp: the wire record of a berg against the three lists it replaced, and
// the skip rule of the row permutation against the switch it replaced, all restated here as literals.  Line numbers:
// icebergs_amd/csrc/kid_migrate.inc and kid_hip.hip of commit 5050db6, the last one with the hand-written lists.
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_rows_plan_cpu.py.
#include <cstdio>
#include <cstdlib>

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

static_assert(kid::MIG_WIDTH == 34, "usable in static_assert");
static_assert(kid::field_never_written(kid::NeverWrittenIn{false, false, false, false, true, false, false}, KID_B_UO), "constexpr");

// special words of the former lists
enum { START_YEAR = -1, INE = -2, JNE = -3, ID_HI = -4, ID_LO = -5 };

// mig_write_record, kid_migrate.inc:30-44: the order of its o[c++] = ... stores
static const int written[34] = {
    KID_B_LON, KID_B_LAT, KID_B_UVEL, KID_B_VVEL, KID_B_UVEL_PREV, KID_B_VVEL_PREV, KID_B_XI, KID_B_YJ,                        // :33-34
    KID_B_START_LON, KID_B_START_LAT, START_YEAR, KID_B_START_DAY,                                                             // :35
    KID_B_START_MASS, KID_B_MASS, KID_B_THICKNESS, KID_B_WIDTH,                                                                // :36
    KID_B_LENGTH, KID_B_FL_K, KID_B_MASS_SCALING, KID_B_MASS_OF_BITS,                                                          // :37
    KID_B_MASS_OF_FL_BITS, KID_B_MASS_OF_FL_BERGY_BITS, KID_B_HEAT_DENSITY,                                                    // :38
    INE, JNE,                                                                                                                  // :39
    KID_B_AXN, KID_B_AYN, KID_B_BXN, KID_B_BYN,                                                                                // :40
    KID_B_HALO_BERG, KID_B_STATIC_BERG,                                                                                        // :41 (`halo` goes where halo_berg goes)
    ID_HI, ID_LO,                                                                                                              // :42
    KID_B_OD};                                                                                                                 // :43

// the decode of unpack_immigrants_kernel, kid_migrate.inc:84-96: (word, what it was stored to); xi and yj (words 6, 7) were not
// taken from the record
struct Decoded { int word, target; };
static const Decoded decoded[] = {
    {0, KID_B_LON}, {1, KID_B_LAT}, {2, KID_B_UVEL}, {3, KID_B_VVEL}, {4, KID_B_UVEL_PREV}, {5, KID_B_VVEL_PREV},             // :84-86
    {8, KID_B_START_LON}, {9, KID_B_START_LAT}, {10, START_YEAR}, {11, KID_B_START_DAY},                                       // :87
    {12, KID_B_START_MASS}, {13, KID_B_MASS}, {14, KID_B_THICKNESS}, {15, KID_B_WIDTH},                                        // :88
    {16, KID_B_LENGTH}, {17, KID_B_FL_K}, {18, KID_B_MASS_SCALING}, {19, KID_B_MASS_OF_BITS},                                  // :89
    {20, KID_B_MASS_OF_FL_BITS}, {21, KID_B_MASS_OF_FL_BERGY_BITS}, {22, KID_B_HEAT_DENSITY},                                  // :90
    {25, KID_B_AXN}, {26, KID_B_AYN}, {27, KID_B_BXN}, {28, KID_B_BYN},                                                        // :91
    {29, KID_B_HALO_BERG}, {30, KID_B_STATIC_BERG}, {33, KID_B_OD},                                                            // :92
    {31, ID_HI}, {32, ID_LO},                                                                                                  // :93
    {23, INE}, {24, JNE}};                                                                                                     // :96

// the host table wire_f64[], kid_migrate.inc:235-238, and the words that marked has_static (:242) and has_fl (:243)
static const int wire_f64[34] = {KID_B_LON, KID_B_LAT, KID_B_UVEL, KID_B_VVEL, KID_B_UVEL_PREV, KID_B_VVEL_PREV, KID_B_XI, KID_B_YJ,
    KID_B_START_LON, KID_B_START_LAT, -1 /* start_year */, KID_B_START_DAY, KID_B_START_MASS, KID_B_MASS, KID_B_THICKNESS, KID_B_WIDTH,
    KID_B_LENGTH, KID_B_FL_K, KID_B_MASS_SCALING, KID_B_MASS_OF_BITS, KID_B_MASS_OF_FL_BITS, KID_B_MASS_OF_FL_BERGY_BITS, KID_B_HEAT_DENSITY,
    -2 /* ine */, -3 /* jne */, KID_B_AXN, KID_B_AYN, KID_B_BXN, KID_B_BYN, KID_B_HALO_BERG, KID_B_STATIC_BERG, -4 /* id_cnt */, -5 /* id_ij */, KID_B_OD};
static const int static_words[] = {30, 29};
static const int fl_words[] = {20, 21, 17};

// what a word of the table stands for, in the terms of the former lists
static int meaning(const kid::WireWord &w) {
  switch (w.kind) {
    case kid::WIRE_F64: return w.field;
    case kid::WIRE_I32: return w.field == KID_BI_START_YEAR ? START_YEAR : -100;
    case kid::WIRE_INE: return INE;
    case kid::WIRE_JNE: return JNE;
    case kid::WIRE_ID_HI: return ID_HI;
    case kid::WIRE_ID_LO: return ID_LO;
  }
  return -100;
}
static bool in(const int *list, int n, int w) { for (int q = 0; q < n; ++q) if (list[q] == w) return true; return false; }

static void check_record() {
  for (int w = 0; w < kid::MIG_WIDTH; ++w) {
    const int m = meaning(kid::WIRE_RECORD[w]);
    CHECK(m == written[w], "word %d: table %d, mig_write_record %d", w, m, written[w]);
    CHECK(m == wire_f64[w], "word %d: table %d, wire_f64 %d", w, m, wire_f64[w]);
    const bool f64 = kid::WIRE_RECORD[w].kind == kid::WIRE_F64;
    CHECK((f64 && kid::marks_has_static(kid::WIRE_RECORD[w].field)) == in(static_words, 2, w), "word %d: has_static", w);
    CHECK((f64 && kid::marks_has_fl(kid::WIRE_RECORD[w].field)) == in(fl_words, 3, w), "word %d: has_fl", w);
  }
  bool seen[34] = {};
  for (const Decoded &d : decoded) {
    CHECK(d.word >= 0 && d.word < kid::MIG_WIDTH && !seen[d.word], "decode list, word %d", d.word);
    seen[d.word] = true;
    CHECK(meaning(kid::WIRE_RECORD[d.word]) == d.target, "word %d: table %d, decode %d", d.word, meaning(kid::WIRE_RECORD[d.word]), d.target);
  }
  for (int w = 0; w < kid::MIG_WIDTH; ++w)   // the two words the decode leaves to the receiving grid
    CHECK(seen[w] == !(kid::WIRE_RECORD[w].kind == kid::WIRE_F64 && (kid::WIRE_RECORD[w].field == KID_B_XI || kid::WIRE_RECORD[w].field == KID_B_YJ)), "word %d: decoded or not", w);
  // the words the code addresses singly: r[23], r[24], r[29], r[30], r[31], r[32], r[33], r[0..3]
  CHECK(kid::WIRE_W_INE == 23 && kid::WIRE_W_JNE == 24 && kid::WIRE_W_HALO_BERG == 29 && kid::WIRE_W_STATIC_BERG == 30, "named indices");
  CHECK(kid::WIRE_W_ID_HI == 31 && kid::WIRE_W_ID_LO == 32 && kid::WIRE_W_OD == 33, "named indices");
  CHECK(kid::WIRE_W_LON == 0 && kid::WIRE_W_LAT == 1 && kid::WIRE_W_UVEL == 2 && kid::WIRE_W_VVEL == 3, "named indices");
}

// field_never_written, kid_hip.hip:938-957, on plain values
static bool former_never_written(bool footloose, bool mts, bool calving_on, int periodic_reentry, int runge_not_verlet, int has_fl, bool env_ever_stored, int f) {
  if (footloose || mts || calving_on) return false;
  switch (f) {
    case KID_B_AXN_FAST: case KID_B_AYN_FAST: case KID_B_BXN_FAST: case KID_B_BYN_FAST: case KID_B_ANG_VEL: case KID_B_ANG_ACCEL: case KID_B_ROT:
    case KID_B_UVEL_OLD: case KID_B_VVEL_OLD: case KID_B_LON_OLD: case KID_B_LAT_OLD:
      return periodic_reentry == 0;
    case KID_B_HALO_BERG: case KID_B_STATIC_BERG: case KID_B_START_LON: case KID_B_START_LAT: case KID_B_START_MASS: case KID_B_HEAT_DENSITY:
      return true;
    case KID_B_UVEL_PREV: case KID_B_VVEL_PREV:
      return runge_not_verlet != 0;
    case KID_B_MASS_OF_FL_BITS: case KID_B_MASS_OF_FL_BERGY_BITS: case KID_B_FL_K: case KID_B_START_DAY: case KID_B_MASS_SCALING:
      return has_fl == 0;
    case KID_B_UO: case KID_B_VO: case KID_B_UI: case KID_B_VI: case KID_B_UA: case KID_B_VA: case KID_B_SSH_X: case KID_B_SSH_Y:
    case KID_B_SST: case KID_B_SSS: case KID_B_CN: case KID_B_HI: case KID_B_OD:
      return !env_ever_stored;
    default:
      return false;
  }
}
static void check_never_written() {
  int skipped_somewhere = 0;
  for (int bits = 0; bits < 128; ++bits) {
    const bool fl = bits & 1, mts = bits & 2, calv = bits & 4, per = bits & 8, rk = bits & 16, has_fl = bits & 32, env = bits & 64;
    const kid::NeverWrittenIn s{fl, mts, calv, per, rk, has_fl, env};
    for (int f = -1; f <= KID_NB_F64; ++f) {   // one past either end too: not a field, never skipped
      const bool got = kid::field_never_written(s, f), want = former_never_written(fl, mts, calv, per ? 1 : 0, rk ? 1 : 0, has_fl ? 1 : 0, env, f);
      CHECK(got == want, "switches %d, field %d: %d, formerly %d", bits, f, (int)got, (int)want);
      skipped_somewhere += got ? 1 : 0;
    }
  }
  CHECK(skipped_somewhere > 0, "the rule never skips anything");
}

int main() {
  check_record();
  check_never_written();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
