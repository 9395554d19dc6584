// Host-side check of icebergs_amd/csrc/kid_launch_select.hpp: every input of the selection functions, against the rules of the
// launch macros they replaced, restated here independently (masks as numbers: 1 interp, 2 evolve, 4 thermo, 8 spread, 16
// footloose, 32 tspread).  Line numbers: icebergs_amd/csrc/kid_hip.hip of commit d563ffb, the last one with the macros.
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_launch_select_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../icebergs_amd/csrc/kid_launch_select.hpp"

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

static_assert(kid::PH_INTERP == 1u && kid::PH_EVOLVE == 2u && kid::PH_THERMO == 4u && kid::PH_SPREAD == 8u && kid::PH_FL == 16u && kid::PH_TSPREAD == 32u, "phase masks");
static_assert(kid::instance_exists(true, 14u, true) && !kid::instance_exists(false, 14u, false), "usable in if constexpr / static_assert");
static_assert(kid::hot_build_k(true, true, 14u, true, false, true, false) == 3, "constexpr");

// KID_LAUNCH(RKV, OLDV), :1233-1256, with launch_stage :1169-1174: its four ifs
static int macro_k(bool rk, bool old, unsigned ph, bool plain, bool flprof, bool store_env, bool stage) {
  if (stage) return 0;                                                      // :1235 launch_stage<RKV, OLDV, PH>: berg_kernel<..., true, 0, true>
  if (ph == 14u && rk && old && plain) return store_env ? 3 : 1;            // :1241-1242 launch_hot_plain(... store_env ? 3 : 1)
  else if (ph == 31u && !rk && !old && flprof) return 2;                    // :1243-1244
  else return 0;                                                            // :1246
}

// what a walk over kid_step_local's branches and the entry points can request.  orders: 1 old, 2 new, 3 both.  stage: may
// the launch run with reproducible sums on (a scatter phase, and not behind repro_refuse: mts, interacting bergs, footloose)
struct Request { int line; unsigned ph; int orders; bool stage; const char *site; };
static const Request requests[] = {
    {1361, 1u, 3, false, "kid_interp_gridded_fields_to_bergs"},
    {1372, 2u, 3, false, "kid_evolve_icebergs"},
    {1386, 4u, 3, true, "kid_thermodynamics"},
    {1511, 8u, 3, true, "kid_create_gridded_icebergs_fields"},
    {79, 8u, 3, true, "kid_calculate_mass_on_ocean (kid_halo.inc:79)"},
    {1548, 12u, 3, false, "kid_step_local, mts: thermo | spread"},
    {1553, 1u, 2, false, "interacting STS, new order: interp"},
    {1558, 12u, 1, false, "interacting STS: thermo | spread, old"},
    {1558, 13u, 2, false, "interacting STS: interp | thermo | spread, new"},
    {1567, 30u, 1, false, "footloose fused, old"},
    {1567, 31u, 2, false, "footloose fused, new"},
    {1584, 12u, 1, false, "footloose children, old"},
    {1584, 13u, 2, false, "footloose children, new"},
    {1588, 1u, 3, false, "footloose phase by phase, static: interp"},
    {1588, 3u, 3, false, "footloose phase by phase: interp | evolve"},
    {1592, 13u, 3, false, "footloose phase by phase: interp | thermo | spread"},
    {1602, 2u, 1, false, "find_melt_using_spread_mass: evolve, old"},
    {1602, 3u, 2, false, "find_melt_using_spread_mass: interp | evolve, new"},
    {1607, 8u, 3, true, "find_melt_using_spread_mass: spread before the melt"},
    {1617, 36u, 1, true, "Iceberg_melt_without_decay: thermo | tspread, old"},
    {1617, 37u, 2, true, "Iceberg_melt_without_decay: interp | thermo | tspread, new"},
    {1623, 8u, 3, true, "Iceberg_melt_without_decay: spread"},
    {1625, 12u, 1, true, "find_melt_using_spread_mass: thermo | spread, old"},
    {1625, 13u, 2, true, "find_melt_using_spread_mass: interp | thermo | spread, new"},
    {1628, 12u, 1, true, "default old, static_icebergs"},
    {1629, 14u, 1, false, "default old, launch_berg_lanes<true>"},
    {1630, 14u, 1, true, "default old, fused step"},
    {1634, 15u, 2, false, "default new, launch_berg_lanes<false>"},
    {1635, 15u, 2, true, "default new, fused step"},
    {1636, 1u, 2, false, "default new, static: interp"},
    {1636, 3u, 2, false, "default new unfused: interp | evolve"},
    {1638, 13u, 2, true, "default new unfused / static: interp | thermo | spread"},
};

int main() {
  // 1. the K choice, every input
  for (unsigned ph = 0; ph < 64u; ++ph)
    for (int bits = 0; bits < 64; ++bits) {
      const bool rk = bits & 1, old = bits & 2, plain = bits & 4, flprof = bits & 8, store_env = bits & 16, stage = bits & 32;
      const int want = macro_k(rk, old, ph, plain, flprof, store_env, stage), got = kid::hot_build_k(rk, old, ph, plain, flprof, store_env, stage);
      CHECK(got == want, "ph %u bits %d: K %d, the macro chose %d", ph, bits, got, want);
    }
  // 2. every request exists
  for (const Request &r : requests)
    for (int o = 0; o < 2; ++o) {
      const bool old = o == 0;
      if (!(r.orders & (old ? 1 : 2))) continue;
      CHECK(kid::instance_exists(old, r.ph, false), ":%d %s (ph %u, %s order)", r.line, r.site, r.ph, old ? "old" : "new");
      if (r.stage) CHECK(kid::instance_exists(old, r.ph, true), ":%d %s (ph %u, %s order, staging)", r.line, r.site, r.ph, old ? "old" : "new");
    }
  // 3. the dead set.  The order ternaries (p.old_interp_flds_order ? launch_berg<X> : launch_berg<PH_INTERP | X>) call each of
  // these six masks under one order only; repro_refuse (:1184) turns footloose away before a staging launch
  const unsigned old_only[3] = {14u, 30u, 36u};
  for (unsigned x : old_only)
    for (int st = 0; st < 2; ++st) {
      CHECK(!kid::instance_exists(false, x, st != 0), "ph %u under the new order", x);
      CHECK(!kid::instance_exists(true, x | 1u, st != 0), "ph %u under the old order", x | 1u);
    }
  CHECK(!kid::instance_exists(true, 30u, true), "staging with PH_FL (old)");
  CHECK(!kid::instance_exists(false, 31u, true), "staging with PH_FL (new)");
  // nothing to stage without a scatter phase; nothing outside the thirteen masks; 129 kernels in kid_hip.o: hot and general
  // build of both integrators for every triple, and the footloose-profile hot build
  int triples = 0;
  for (unsigned ph = 0; ph < 64u; ++ph)
    for (int bits = 0; bits < 4; ++bits) {
      const bool old = bits & 1, stage = bits & 2;
      bool requested = false;
      for (const Request &r : requests) requested = requested || (r.ph == ph && (r.orders & (old ? 1 : 2)) && (!stage || (ph & 12u)));
      const bool dead_stage = stage && (ph & 16u);
      const bool got = kid::instance_exists(old, ph, stage);
      // (a scatter mask behind repro_refuse on every path of today still has its staging instance, as before: the rule
      // is the mask's, not the path's; so `requested` uses the mask's scatter bits, not Request::stage)
      CHECK(got == (requested && !dead_stage), "ph %u old %d stage %d: exists %d", ph, (int)old, (int)stage, (int)got);
      if (stage && !(ph & 12u)) CHECK(!got, "ph %u: a staging instance without a scatter phase", ph);
      triples += got ? 1 : 0;
    }
  CHECK(triples == 32, "%d (old, ph, stage) triples", triples);
  CHECK(triples * 4 + 1 == 129, "%d kernels", triples * 4 + 1);
  // 4. part count (:1212) and slow-lane eligibility (:1280-1284) on a grid of their inputs
  const long long ns[] = {0, 1, 4095, 4096, 4097, 1ll << 20, 1ll << 33};
  for (long long n : ns)
    for (int bits = 0; bits < 32; ++bits) {
      const bool pipelined = bits & 1, stage = bits & 2, mts = bits & 4, footloose = bits & 8, whole = bits & 16;
      const long long range_len = whole ? -1 : 7;
      const int want = (pipelined && !stage && !mts && !footloose && n >= 4096 && range_len < 0) ? 2 : 1;
      CHECK(kid::launch_parts(pipelined, stage, mts, footloose, n, whole) == want, "n %lld bits %d", n, bits);
    }
  const double gfs[] = {0., -1., 0.5, 1e-300};
  for (long long n : ns)
    for (int side_mode = 0; side_mode < 4; ++side_mode)
      for (double gf : gfs)
        for (int bits = 0; bits < 128; ++bits) {
          const bool side_stream = bits & 1, repro = bits & 2, static_icebergs = bits & 4, mts = bits & 8, interactive = bits & 16, footloose = bits & 32, fmusm = bits & 64;
          const bool want = side_mode == 2 && side_stream && !repro && !static_icebergs && !mts && !interactive && !footloose && !(gf > 0.) && !fmusm && n >= 4096;
          CHECK(kid::lanes_eligible(side_mode, side_stream, repro, static_icebergs, mts, interactive, footloose, gf, fmusm, n) == want,
                "n %lld mode %d gf %g bits %d", n, side_mode, gf, bits);
        }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
