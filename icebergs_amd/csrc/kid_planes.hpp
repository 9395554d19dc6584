// kid_planes.hpp -- the layout of the accumulator block (KID_A_*, include/kid_types.h), as plain C++17: no HIP header, no handle.
// Which planes a step keeps live, which of them a halo update exchanges, and the nine-point sum of sum_up_spread_fields are
// written down here once; kid_cells.inc, kid_halo.inc, kid_repro.inc and kid_chksum_device.inc ask the functions below,
// tests/planes_host.cpp enumerates them on the host.
#pragma once
#include "../../include/kid_types.h"

namespace kid {

struct PlaneRange {
  int first, count;
  constexpr int end() const { return first + count; }
  constexpr bool contains(int plane) const { return plane >= first && plane < end(); }
};
// mass/area/Uvel/Vvel_on_ocean (IB:4088): four families (v = 0 .. 3) of nine slots each, one after the other
constexpr int ON_OCEAN_SLOTS = 9;
constexpr PlaneRange on_ocean_family(int v) { return {KID_A_MASS_ON_OCEAN + ON_OCEAN_SLOTS * v, ON_OCEAN_SLOTS}; }
constexpr PlaneRange MASS_ON_OCEAN = on_ocean_family(0);
constexpr PlaneRange ON_OCEAN_ALL{KID_A_MASS_ON_OCEAN, 4 * ON_OCEAN_SLOTS};   // what calculate_mass_on_ocean zeroes, IB:4984-4987
constexpr PlaneRange ON_OCEAN_VEL{KID_A_UVEL_ON_OCEAN, 2 * ON_OCEAN_SLOTS};   // what thermodynamics zeroes, IB:2872-2873
static_assert(on_ocean_family(1).first == KID_A_AREA_ON_OCEAN && on_ocean_family(2).first == KID_A_UVEL_ON_OCEAN && on_ocean_family(3).first == KID_A_VVEL_ON_OCEAN &&
              ON_OCEAN_ALL.end() == KID_NACC_CORE && ON_OCEAN_VEL.end() == KID_NACC_CORE, "the four families end the core planes");

// area/Uvel/Vvel_on_ocean (27 planes) are intermediates of spread_area / spread_uvel / spread_vvel / ustar_iceberg
// (IB:3419-3474), which the reference evaluates only for `id_*>0` or pass_fields_to_ocean_model: when nobody reads them
// they are neither scattered nor zeroed nor exchanged (the reference fills them regardless and drops them)
constexpr bool footprint_needed(int pass_fields_to_ocean_model, int diag_mask) {
  return pass_fields_to_ocean_model || (diag_mask & (KID_DIAG_SPREAD_UVEL | KID_DIAG_SPREAD_VVEL | KID_DIAG_SPREAD_AREA | KID_DIAG_USTAR_ICEBERG));
}
// the planes a step zeroes, fills and reduces: a prefix of the block
constexpr int nacc_live(int pass_fields_to_ocean_model, int diag_mask) {
  constexpr int diag_planes = KID_DIAG_MELT_BY_CLASS | KID_DIAG_FL_PARENT_MELT | KID_DIAG_FL_CHILD_MELT | KID_DIAG_MELT_BUOY | KID_DIAG_MELT_EROS |
                              KID_DIAG_MELT_CONV | KID_DIAG_MELT_BUOY_FL | KID_DIAG_MELT_EROS_FL | KID_DIAG_MELT_CONV_FL | KID_DIAG_VIRTUAL_AREA |
                              KID_DIAG_MASS | KID_DIAG_U_ICEBERG | KID_DIAG_V_ICEBERG;
  return (diag_mask & diag_planes) ? KID_NACC : footprint_needed(pass_fields_to_ocean_model, diag_mask) ? KID_NACC_CORE : MASS_ON_OCEAN.end();
}
// are planes [plane, plane + nk) live?  (Inside the prefix, and not among the 27 that nobody reads.)
constexpr bool plane_range_live(int plane, int nk, int pass_fields_to_ocean_model, int diag_mask) {
  return plane + nk <= nacc_live(pass_fields_to_ocean_model, diag_mask) &&
         (footprint_needed(pass_fields_to_ocean_model, diag_mask) || plane < MASS_ON_OCEAN.end() || plane >= ON_OCEAN_ALL.end());
}
// the on-ocean planes a halo update exchanges, counted from MASS_ON_OCEAN.first
constexpr int halo_plane_count(int pass_fields_to_ocean_model, int diag_mask) {
  return footprint_needed(pass_fields_to_ocean_model, diag_mask) ? ON_OCEAN_ALL.count : MASS_ON_OCEAN.count;
}

// The nine-point sum of sum_up_spread_fields, IB:6126-6131: slot `slot` (1-based) of the cell at (i + di, j + dj) is the share
// its bergs spread into cell (i, j).  Listed in the order the reference adds them: the centre, then the four diagonal and the
// four edge neighbours in opposite pairs; nine_point_sum keeps its parentheses, which is what makes spread_mass match to the bit.
struct StencilPoint { int di, dj, slot; };
constexpr StencilPoint NINE_POINT[9] = {{0, 0, 5}, {-1, -1, 9}, {1, 1, 1}, {1, -1, 7}, {-1, 1, 3}, {-1, 0, 6}, {1, 0, 4}, {0, -1, 8}, {0, 1, 2}};
template <class At>   // at(di, dj, slot): the value of one entry of NINE_POINT
constexpr double nine_point_sum(At &&at) {
#define KID_P(k) at(NINE_POINT[k].di, NINE_POINT[k].dj, NINE_POINT[k].slot)
  return KID_P(0) + (((KID_P(1) + KID_P(2)) + (KID_P(3) + KID_P(4))) + ((KID_P(5) + KID_P(6)) + (KID_P(7) + KID_P(8))));
#undef KID_P
}

}  // namespace kid
