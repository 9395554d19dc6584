// kid_launch_select.hpp -- which berg_kernel a launch gets, as plain C++17: no HIP header, no handle.  kid_berg_kernel.hpp
// takes the phase masks from here, kid_launch.inc asks the functions below before every launch (and instantiates a kernel
// only where instance_exists says so), tests/launch_select_host.cpp enumerates them on the host.
#pragma once

namespace kid {

enum : unsigned { PH_INTERP = 1u, PH_EVOLVE = 2u, PH_THERMO = 4u, PH_SPREAD = 8u, PH_FL = 16u, PH_TSPREAD = 32u };   // PH_FL: footloose_calving between evolve and thermodynamics
constexpr unsigned PH_SCATTER = PH_THERMO | PH_SPREAD;                  // a launch with one of these adds to the per-cell sums
constexpr unsigned PH_STEP = PH_EVOLVE | PH_THERMO | PH_SPREAD;         // the fused step of the old order; PH_INTERP | PH_STEP: of the new
constexpr unsigned PH_STEP_FL = PH_STEP | PH_FL;                        // ... with footloose calving inside

// The masks kid_launch.inc launches:
//   one phase        -- the four phase entry points (interp, evolve, thermo, spread; the last also kid_calculate_mass_on_ocean)
//   interp | evolve  -- the unfused sequences (footloose phase by phase, KID_NEW_ORDER_UNFUSED, find_melt_using_spread_mass)
//   [interp |] thermo | spread            -- the second half of every unfused sequence, MTS, interacting STS, footloose children
//   [interp |] evolve [| fl] | thermo | spread -- the fused step
//   [interp |] thermo | tspread           -- find_melt_using_spread_mass with Iceberg_melt_without_decay
constexpr bool mask_launched(unsigned ph) {
  const unsigned x = ph & ~PH_INTERP;
  return ph == PH_INTERP || ph == PH_EVOLVE || ph == PH_THERMO || ph == PH_SPREAD || ph == (PH_INTERP | PH_EVOLVE) ||
         x == (PH_THERMO | PH_SPREAD) || x == PH_STEP || x == PH_STEP_FL || x == (PH_THERMO | PH_TSPREAD);
}
// A mask that only launch_ordered ever requests: PH_INTERP is in it exactly under the new order (.not.old_interp_flds_order).
// These are the fused step (an evolve together with a scatter phase) and the thermodynamics that spreads for itself.
// Every other mask is reached by a sequence that runs under both orders (the entry points, MTS, the unfused sequences).
constexpr bool order_bound(unsigned ph) { return ((ph & PH_EVOLVE) && (ph & PH_SCATTER)) || (ph & PH_TSPREAD); }

// Can the host request berg_kernel<*, OLD_ORDER = old, ph, *, *, STAGE = stage>?  (Both integrators, hot and general build.)
constexpr bool instance_exists(bool old, unsigned ph, bool stage) {
  if (!mask_launched(ph)) return false;
  if (order_bound(ph) && old != !(ph & PH_INTERP)) return false;
  // the staging instance belongs to reproducible sums: nothing to stage without a scatter phase, and repro_refuse turns
  // footloose away before anything is launched
  if (stage && (!(ph & PH_SCATTER) || (ph & PH_FL))) return false;
  return true;
}

// Which hot build: 0 the general switches, 1 the plain namelist, 3 the same with the stored environment, 2 the footloose
// profile (Sw<K>, kid_device.hpp).  plain / flprof: plain_namelist() / fl_profile_namelist() of the handle.
constexpr int hot_build_k(bool rk, bool old, unsigned ph, bool plain, bool flprof, bool store_env, bool stage) {
  if (stage) return 0;
  if (ph == PH_STEP && rk && old && plain) return store_env ? 3 : 1;
  if (ph == (PH_INTERP | PH_STEP_FL) && !rk && !old && flprof) return 2;
  return 0;
}

// Two half launches (the general build of a half on the side stream, under the hot build of the other half) or one.
// whole: the launch covers the whole population, not a range of rows.
constexpr int launch_parts(bool pipelined, bool stage, bool mts, bool footloose, long long n, bool whole) {
  return (pipelined && !stage && !mts && !footloose && n >= 4096 && whole) ? 2 : 1;
}

// May a fused step run on the slow-lane schedule (kid_set_side_stream mode 2)?
constexpr bool lanes_eligible(int side_mode, bool side_stream, bool repro, bool static_icebergs, bool mts, bool interactive, bool footloose,
                              double grounding_fraction, bool find_melt_using_spread_mass, long long n) {
  return side_mode == 2 && side_stream && !repro && !static_icebergs && !mts && !interactive && !footloose && !(grounding_fraction > 0.) &&
         !find_melt_using_spread_mass && n >= 4096;
}

}  // namespace kid
