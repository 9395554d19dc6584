// Host-side check of the rule "field f holds only zeros in every row" of icebergs_amd/csrc/kid_rows_plan.hpp (ZeroState,
// field_known_zero, known_zero_mask): the rule over every combination of its inputs against its statement in words, restated
// here as literals, and the masks a handle would hand to the plain hot builds along scripted sequences of the events that
// kid_rows.inc and kid_launch.inc report (upload, launches, changes of the namelist, appended rows).
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_zero_fields_cpu.py.
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

typedef unsigned long long u64;
static const u64 AXN = 1ull << KID_B_AXN, AYN = 1ull << KID_B_AYN, BITS = 1ull << KID_B_MASS_OF_BITS, HD = 1ull << KID_B_HEAT_DENSITY;
static const u64 ALL = AXN | AYN | BITS | HD;
static_assert(kid::KID_ZERO_FIELDS == ((1ull << KID_B_AXN) | (1ull << KID_B_AYN) | (1ull << KID_B_MASS_OF_BITS) | (1ull << KID_B_HEAT_DENSITY)), "the four fields");
static_assert(kid::field_known_zero(kid::KnownZeroIn{false, false, false, true, true}, KID_B_AXN), "constexpr");
static_assert(kid::known_zero_mask(kid::ZeroState{}, true, true, true) == kid::KID_ZERO_FIELDS, "constexpr");

// the rule in words: never after a non-zero upload; axn, ayn while no launch could have written them and the integrator is RK;
// mass_of_bits while no launch could have and the erosion fraction is 0; heat_density while no kernel of the configuration
// writes it; no other field
static void check_rule() {
  int known = 0;
  for (int bits = 0; bits < 32; ++bits) {
    const bool up = bits & 1, la = bits & 2, nw = bits & 4, rk = bits & 8, ez = bits & 16;
    const kid::KnownZeroIn s{up, la, nw, rk, ez};
    for (int f = -1; f <= KID_NB_F64; ++f) {   // one past either end too: not a field, never zero
      bool want = false;
      if (f == KID_B_AXN || f == KID_B_AYN) want = !up && !la && rk;
      else if (f == KID_B_MASS_OF_BITS) want = !up && !la && ez;
      else if (f == KID_B_HEAT_DENSITY) want = !up && nw;
      const bool got = kid::field_known_zero(s, f);
      CHECK(got == want, "inputs %d, field %d: %d, want %d", bits, f, (int)got, (int)want);
      known += got ? 1 : 0;
    }
  }
  CHECK(known > 0, "the rule never knows anything");
}

// a handle, as far as the rule sees it
struct Model {
  kid::ZeroState zs;
  bool rk = true, calving_on = false, has_fl = false;
  double erosion = 0.;
  void upload(u64 nonzero) { for (int f = 0; f < KID_NB_F64; ++f) zs.uploaded(f, ((nonzero >> f) & 1ull) != 0); }
  void step() { zs.launched_berg(true, true, rk, erosion == 0., has_fl, false); }          // the fused step
  void evolve() { zs.launched_berg(true, false, rk, erosion == 0., has_fl, false); }       // kid_evolve_icebergs
  void thermo() { zs.launched_berg(false, true, rk, erosion == 0., has_fl, false); }       // kid_thermodynamics
  u64 mask() const { return kid::known_zero_mask(zs, !calving_on, rk, erosion == 0.); }
};

// the mask: the rule field by field, except that axn and ayn are known together or not at all
static void check_mask() {
  for (int bits = 0; bits < (1 << 11); ++bits) {
    kid::ZeroState z;
    const int fields[4] = {KID_B_AXN, KID_B_AYN, KID_B_MASS_OF_BITS, KID_B_HEAT_DENSITY};
    for (int q = 0; q < 4; ++q) { z.uploaded_nonzero[fields[q]] = (bits >> q) & 1; z.launched_nonzero[fields[q]] = (bits >> (4 + q)) & 1; }
    const bool nw = bits & 256, rk = bits & 512, ez = bits & 1024;
    u64 want = 0ull;
    for (int q = 0; q < 4; ++q)
      if (kid::field_known_zero(kid::KnownZeroIn{z.uploaded_nonzero[fields[q]], z.launched_nonzero[fields[q]], nw, rk, ez}, fields[q])) want |= 1ull << fields[q];
    if ((want & (AXN | AYN)) != (AXN | AYN)) want &= ~(AXN | AYN);
    const u64 got = kid::known_zero_mask(z, nw, rk, ez);
    CHECK(got == want, "inputs %d: %llx, want %llx", bits, got, want);
    z.uploaded_nonzero[KID_B_LON] = true; z.launched_nonzero[KID_B_MASS] = true;   // other fields do not enter
    CHECK(kid::known_zero_mask(z, nw, rk, ez) == want, "inputs %d with other fields marked", bits);
  }
}

static void check_sequences() {
  {  // a plain RK4 run: everything stays known, however long
    Model m; m.upload(0);
    for (int s = 0; s < 5; ++s) { m.step(); CHECK(m.mask() == ALL, "plain run, step %d: %llx", s, m.mask()); }
    m.evolve(); m.thermo();
    CHECK(m.mask() == ALL, "phase by phase: %llx", m.mask());
  }
  {  // a field uploaded non-zero is unknown until an upload proves zeros, and only that field
    Model m; m.upload(AXN);
    m.step(); CHECK(m.mask() == (ALL & ~(AXN | AYN)), "axn uploaded -- ayn goes with it: %llx", m.mask());
    for (int s = 0; s < 3; ++s) m.step();
    CHECK(m.mask() == (ALL & ~(AXN | AYN)), "... and it stays unknown: %llx", m.mask());
    m.upload(HD); m.step(); CHECK(m.mask() == (ALL & ~HD), "heat_density uploaded: %llx", m.mask());
    m.upload(0); m.step(); CHECK(m.mask() == ALL, "zeros uploaded again: %llx", m.mask());
  }
  {  // Verlet: not known while the integrator is Verlet, and not afterwards either -- the switch back clears nothing
    Model m; m.upload(0);
    m.rk = false;
    CHECK(m.mask() == (ALL & ~(AXN | AYN)), "Verlet now: %llx", m.mask());
    m.rk = true;
    CHECK(m.mask() == ALL, "no Verlet launch was enqueued: %llx", m.mask());
    m.rk = false; m.step(); m.step(); m.rk = true; m.step();
    CHECK(m.mask() == (ALL & ~(AXN | AYN)), "two Verlet steps, then RK: %llx", m.mask());
    m.upload(0); m.step();
    CHECK(m.mask() == ALL, "an upload of zeros clears the mark: %llx", m.mask());
    m.rk = false; m.thermo(); m.rk = true;
    CHECK(m.mask() == ALL, "a Verlet handle's thermodynamics does not write axn: %llx", m.mask());
    m.rk = false; m.evolve(); m.rk = true;
    CHECK(m.mask() == (ALL & ~(AXN | AYN)), "its evolve does: %llx", m.mask());
  }
  {  // bergy bits: the erosion fraction now, and at every thermodynamics launch since the upload
    Model m; m.upload(0);
    m.erosion = 0.5;
    CHECK(m.mask() == (ALL & ~BITS), "erosion on: %llx", m.mask());
    m.erosion = 0.;
    CHECK(m.mask() == ALL, "no launch with it: %llx", m.mask());
    m.erosion = 0.5; m.evolve(); m.erosion = 0.;
    CHECK(m.mask() == ALL, "the evolve does not touch the bits: %llx", m.mask());
    m.erosion = 0.5; m.step(); m.step(); m.erosion = 0.; m.step();
    CHECK(m.mask() == (ALL & ~BITS), "two steps with erosion, then without: %llx", m.mask());
    m.upload(0);
    CHECK(m.mask() == ALL, "upload: %llx", m.mask());
    m.has_fl = true; m.thermo(); m.has_fl = false;
    CHECK(m.mask() == (ALL & ~BITS), "footloose bits can take a melted parent's place: %llx", m.mask());
  }
  {  // MTS, interacting evolve, footloose
    Model m; m.upload(0);
    m.zs.launched_other();
    CHECK(m.mask() == HD, "MTS / interactive / footloose pass: %llx", m.mask());
    m.upload(0);
    m.zs.launched_berg(true, true, true, true, true, true);   // the fused step with footloose calving inside
    CHECK(m.mask() == HD, "footloose step: %llx", m.mask());
  }
  {  // appended rows: records are judged word by word, rows a kernel wrote may hold anything
    Model m; m.upload(0); m.step();
    m.zs.appended_word(KID_B_LON); m.zs.appended_word(KID_B_MASS);
    CHECK(m.mask() == ALL, "immigrants with zeros in the four fields: %llx", m.mask());
    m.zs.appended_word(KID_B_MASS_OF_BITS);
    CHECK(m.mask() == (ALL & ~BITS), "an immigrant with bergy bits: %llx", m.mask());
    m.zs.appended_word(KID_B_AYN);
    CHECK(m.mask() == HD, "... and one with ayn (axn goes with it): %llx", m.mask());
    m.zs.appended_by_kernel();
    CHECK(m.mask() == 0ull, "rows a kernel wrote: %llx", m.mask());
    m.step(); CHECK(m.mask() == 0ull, "... for good: %llx", m.mask());
    m.upload(0); CHECK(m.mask() == ALL, "until the next upload: %llx", m.mask());
  }
  {  // calving writes heat_density into new rows: never known while it is on
    Model m; m.calving_on = true; m.upload(0); m.step();
    CHECK(m.mask() == (ALL & ~HD), "calving on: %llx", m.mask());
  }
}

int main() {
  check_rule();
  check_mask();
  check_sequences();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
