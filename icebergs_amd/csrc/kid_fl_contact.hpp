// kid_fl_contact.hpp -- the two decisions of adjust_fl_berg_interactivity (IB:2765-2841) as plain C++17: no HIP header, no
// handle.  Which cells a footloose child looks into, and whether another berg found there is within contact range.
// fl_adjust_interactivity_kernel (kid_fl_interact.inc) asks both per candidate; tests/fl_contact_host.cpp checks them on the
// host against values written out by hand.  The expressions keep the reference's order of operations.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KID_FLC_HD __host__ __device__
#else
#define KID_FLC_HD
#endif

namespace kid {

// The cells around (i, j) whose lists are searched, IB:2805-2806: nc cells either way, cut at the data domain -- with the
// reference's +1 on the low side (the first row and column of the data domain are never looked into).
struct FlWindow { int j0, j1, i0, i1; };
KID_FLC_HD inline FlWindow fl_contact_window(int i, int j, int nc_x, int nc_y, int isd, int ied, int jsd, int jed) {
  FlWindow w;
  w.j0 = (j - nc_y > jsd + 1) ? j - nc_y : jsd + 1; w.j1 = (j + nc_y < jed) ? j + nc_y : jed;
  w.i0 = (i - nc_x > isd + 1) ? i - nc_x : isd + 1; w.i1 = (i + nc_x < ied) ? i + nc_x : ied;
  return w;
}

// What the pair test reads of the namelist and the grid (IB:2779-2795).
struct FlContactRule {
  bool radial_contact;       // contact_cells_lon == 1 and contact_cells_lat == 1: the bergs' radii count
  bool latlon;               // grd%grid_is_latlon
  double rdenom;             // radius**2 = length * width * rdenom
  double contact_distance, pi_180, Rearth;
};
KID_FLC_HD inline double fl_contact_rdenom(bool hexagonal_icebergs, bool iceberg_bonds_on, double pi) {   // IB:2783-2791
  if (hexagonal_icebergs) return 1. / (2. * sqrt(3.));
  if (iceberg_bonds_on) return 1. / 4.;
  return 1. / pi;
}
KID_FLC_HD inline FlContactRule fl_contact_rule(int contact_cells_lon, int contact_cells_lat, bool hexagonal_icebergs, bool iceberg_bonds_on,
                                                bool latlon, double contact_distance, double pi, double Rearth) {
  FlContactRule r;
  r.radial_contact = contact_cells_lon == 1 && contact_cells_lat == 1;
  r.latlon = latlon;
  r.rdenom = fl_contact_rdenom(hexagonal_icebergs, iceberg_bonds_on, pi);
  r.contact_distance = contact_distance; r.pi_180 = pi / 180.; r.Rearth = Rearth;
  return r;
}
KID_FLC_HD inline double fl_contact_radius(const FlContactRule &r, double length, double width) { return sqrt(length * width * r.rdenom); }   // IB:2804, 2813
// the squared distance below which two bergs are in contact (IB:2794, 2814); R1, R2 are read with radial contact only
KID_FLC_HD inline double fl_crit_dist(const FlContactRule &r, double R1, double R2) {
  if (!r.radial_contact) return r.contact_distance * r.contact_distance;
  const double reach = (R1 + R2 > r.contact_distance) ? R1 + R2 : r.contact_distance;
  return reach * reach;
}
// the squared distance of berg 2 from berg 1 (IB:2811, 2816-2822): metres on a lat-lon grid, grid units otherwise
KID_FLC_HD inline double fl_r_dist(const FlContactRule &r, double lon1, double lat1, double lon2, double lat2) {
  const double dlon = lon2 - lon1, dlat = lat2 - lat1;
  if (r.latlon) {
    const double lat_ref = 0.5 * (lat1 + lat2);
    const double dx_dlon = r.pi_180 * r.Rearth * cos(lat_ref * r.pi_180), dy_dlat = r.pi_180 * r.Rearth;
    const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
    return rx * rx + ry * ry;
  }
  return dlon * dlon + dlat * dlat;
}
// Does berg 2 keep the child berg 1 non-interactive (IB:2809-2826)?  A berg is never its own partner; the other berg's fl_k is
// not asked for -- a sibling child or the parent counts like anybody else.
KID_FLC_HD inline bool fl_in_contact(const FlContactRule &r, int64_t id1, double lon1, double lat1, double R1,
                                     int64_t id2, double lon2, double lat2, double R2) {
  if (id2 == id1) return false;
  return fl_r_dist(r, lon1, lat1, lon2, lat2) < fl_crit_dist(r, R1, R2);
}

}  // namespace kid
