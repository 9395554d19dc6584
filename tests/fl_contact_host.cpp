// The two decisions of adjust_fl_berg_interactivity (icebergs_amd/csrc/kid_fl_contact.hpp, IB:2765-2841) on the host, against
// values written out by hand: the cell window at the corners and the low edge of the data domain, rdenom for the three shapes,
// radial against fixed crit_dist, r_dist on a lat-lon and on a Cartesian grid, the strict `<` at equality, and the same-id
// exclusion.  Plain C++17 with its own main (tests/test_fl_interactive_cpu.py builds it with the address and undefined-behaviour
// sanitizers); no GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../icebergs_amd/csrc/kid_fl_contact.hpp"

using namespace kid;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
static bool near(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }
static bool window_is(const FlWindow &w, int i0, int i1, int j0, int j1) { return w.i0 == i0 && w.i1 == i1 && w.j0 == j0 && w.j1 == j1; }

int main() {
  const double pi = 3.14159265358979323846, Rearth = 6360000.0;

  // ---- the cell window: data domain 1..20 by 1..16, one cell either way ----
  CHECK(window_is(fl_contact_window(1, 1, 1, 1, 1, 20, 1, 16), 2, 2, 2, 2));        // south-west corner: the first row and column are never searched
  CHECK(window_is(fl_contact_window(20, 1, 1, 1, 1, 20, 1, 16), 19, 20, 2, 2));     // south-east
  CHECK(window_is(fl_contact_window(1, 16, 1, 1, 1, 20, 1, 16), 2, 2, 15, 16));     // north-west
  CHECK(window_is(fl_contact_window(20, 16, 1, 1, 1, 20, 1, 16), 19, 20, 15, 16));  // north-east
  CHECK(window_is(fl_contact_window(2, 5, 1, 1, 1, 20, 1, 16), 2, 3, 4, 6));        // low edge in i: column 1 is cut, column 2 is the berg's own
  CHECK(window_is(fl_contact_window(5, 2, 1, 1, 1, 20, 1, 16), 4, 6, 2, 3));        // low edge in j
  CHECK(window_is(fl_contact_window(10, 8, 1, 1, 1, 20, 1, 16), 9, 11, 7, 9));      // interior: 3 x 3
  CHECK(window_is(fl_contact_window(3, 3, 2, 3, 1, 20, 1, 16), 2, 5, 2, 6));        // contact_cells_lon = 2, contact_cells_lat = 3
  CHECK(window_is(fl_contact_window(0, 0, 1, 1, -1, 18, -1, 14), 0, 1, 0, 1));      // a data domain that starts at -1 (halo of 2)
  CHECK(window_is(fl_contact_window(18, 14, 1, 1, -1, 18, -1, 14), 17, 18, 13, 14));

  // ---- rdenom ----
  CHECK(near(fl_contact_rdenom(true, false, pi), 0.2886751345948129, 1e-15));    // hexagons: 1 / (2 sqrt 3)
  CHECK(near(fl_contact_rdenom(true, true, pi), 0.2886751345948129, 1e-15));     // ... bonded or not
  CHECK(fl_contact_rdenom(false, true, pi) == 0.25);                             // bonded squares: 1 / 4
  CHECK(near(fl_contact_rdenom(false, false, pi), 0.3183098861837907, 1e-15));   // discs: 1 / pi

  // ---- radial_contact and crit_dist ----
  const FlContactRule radial = fl_contact_rule(1, 1, false, false, false, 2000.0, pi, Rearth);
  const FlContactRule fixed_x = fl_contact_rule(2, 1, false, false, false, 2000.0, pi, Rearth);
  const FlContactRule fixed_y = fl_contact_rule(1, 2, false, false, false, 2000.0, pi, Rearth);
  CHECK(radial.radial_contact && !fixed_x.radial_contact && !fixed_y.radial_contact);
  CHECK(near(fl_contact_radius(radial, std::sqrt(pi) * 1500.0, std::sqrt(pi) * 1500.0), 1500.0, 1e-14));   // a disc of 1.5 km
  CHECK(fl_crit_dist(radial, 900.0, 800.0) == 4.0e6);       // the radii fall short of contact_distance: 2000**2
  CHECK(fl_crit_dist(radial, 1500.0, 1400.0) == 8.41e6);    // (1500 + 1400)**2
  CHECK(fl_crit_dist(fixed_x, 1500.0, 1400.0) == 4.0e6);    // no radial contact: contact_distance**2 whatever the radii
  CHECK(fl_crit_dist(fixed_y, 1.0e9, 1.0e9) == 4.0e6);
  const FlContactRule stern = fl_contact_rule(1, 1, false, false, false, 0.0, pi, Rearth);   // Stern et al.'s search: contact_distance = 0
  CHECK(fl_crit_dist(stern, 1500.0, 1500.0) == 9.0e6);

  // ---- r_dist ----
  CHECK(fl_r_dist(radial, 1000.0, 2000.0, 4000.0, 6000.0) == 25.0e6);              // Cartesian: 3000**2 + 4000**2
  CHECK(fl_r_dist(radial, 4000.0, 6000.0, 1000.0, 2000.0) == 25.0e6);
  const FlContactRule ll = fl_contact_rule(1, 1, false, false, true, 2000.0, pi, Rearth);
  // one degree of longitude at 60 N: pi/180 * 6360000 * cos(60 deg) = 55501.47021341969 m, squared
  CHECK(near(fl_r_dist(ll, 10.0, 60.0, 11.0, 60.0), 3080413195.8511133, 1e-13));
  // half a degree of latitude: 0.5 * 111002.94042683936 m, the same length
  CHECK(near(fl_r_dist(ll, 10.0, 60.0, 10.0, 60.5), 3080413195.8511133, 1e-13));
  // both, about the mean latitude 60 N: 55501.47**2 + 111002.94**2 = 5 * 55501.47**2
  CHECK(near(fl_r_dist(ll, 10.0, 59.5, 11.0, 60.5), 5.0 * 3080413195.8511133, 1e-13));

  // ---- the pair test: strict `<`, never its own partner, the other berg's fl_k is not an argument ----
  const FlContactRule five = fl_contact_rule(2, 2, false, false, false, 5000.0, pi, Rearth);   // crit_dist = 25e6
  CHECK(!fl_in_contact(five, 1, 0.0, 0.0, 0.0, 2, 3000.0, 4000.0, 0.0));      // r_dist == crit_dist: no contact
  CHECK(fl_in_contact(five, 1, 0.0, 0.0, 0.0, 2, 3000.0, 3999.0, 0.0));
  CHECK(!fl_in_contact(five, 1, 0.0, 0.0, 0.0, 2, 3000.0, 4001.0, 0.0));
  CHECK(!fl_in_contact(radial, 1, 0.0, 0.0, 1500.0, 2, 2900.0, 0.0, 1400.0));  // discs that just touch: (R1 + R2)**2 == r_dist
  CHECK(fl_in_contact(radial, 1, 0.0, 0.0, 1500.0, 2, 2899.0, 0.0, 1400.0));
  CHECK(!fl_in_contact(five, 7, 100.0, 100.0, 0.0, 7, 100.0, 100.0, 0.0));    // the same id: never, even at zero distance
  CHECK(fl_in_contact(five, 7, 100.0, 100.0, 0.0, 8, 100.0, 100.0, 0.0));     // a sibling on the same spot keeps the child waiting
  CHECK(!fl_in_contact(stern, 1, 0.0, 0.0, 0.0, 2, 0.0, 0.0, 0.0));           // nothing is closer than zero

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
