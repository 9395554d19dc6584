// Host-side check of icebergs_amd/csrc/kid_planes.hpp: every function against the expression it replaced, restated here as it
// stood in the sources (kid_hip.hip, kid_halo.inc, kid_chksum_device.inc, kid_repro.inc, kid_launch.inc of commit 4b69dbb), for
// every diag_mask bit alone and in pairs, pass_fields_to_ocean_model 0 and 1, every plane 0 .. KID_NACC; and the stencil table
// against the pairing of sum_up_spread_fields (IB:6126-6131) written out longhand.
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_planes_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../icebergs_amd/csrc/kid_planes.hpp"

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

static_assert(kid::nacc_live(0, 0) == KID_A_MASS_ON_OCEAN + 9 && kid::halo_plane_count(1, 0) == 36, "usable in static_assert");

// kid_hip.hip :311-321
static bool old_footprint_needed(int pass, int diag_mask) {
  const int diag = KID_DIAG_SPREAD_UVEL | KID_DIAG_SPREAD_VVEL | KID_DIAG_SPREAD_AREA | KID_DIAG_USTAR_ICEBERG;
  return pass || (diag_mask & diag);
}
static int old_nacc_active(int pass, int diag_mask) {
  const int diag_planes = KID_DIAG_MELT_BY_CLASS | KID_DIAG_FL_PARENT_MELT | KID_DIAG_FL_CHILD_MELT | KID_DIAG_MELT_BUOY |
                          KID_DIAG_MELT_EROS | KID_DIAG_MELT_CONV | KID_DIAG_MELT_BUOY_FL | KID_DIAG_MELT_EROS_FL |
                          KID_DIAG_MELT_CONV_FL | KID_DIAG_VIRTUAL_AREA | KID_DIAG_MASS | KID_DIAG_U_ICEBERG | KID_DIAG_V_ICEBERG;
  if (diag_mask & diag_planes) return KID_NACC;
  return old_footprint_needed(pass, diag_mask) ? KID_NACC_CORE : KID_A_MASS_ON_OCEAN + 9;
}
// kid_chksum_device.inc :435-438
static bool old_chk_live(int plane, int nk, int pass, int diag_mask) {
  const int nacc = old_nacc_active(pass, diag_mask);
  const bool foot = old_footprint_needed(pass, diag_mask);
  return plane + nk <= nacc && (foot || plane < KID_A_AREA_ON_OCEAN || plane >= KID_NACC_CORE);
}
// kid_repro.inc :237-238: the planes repro_fold folds value by value
static bool old_fold_value(int pl, int pass, int diag_mask) { return pl < old_nacc_active(pass, diag_mask) && (pl < KID_A_MASS_ON_OCEAN || pl >= KID_NACC_CORE); }
// kid_halo.inc :50
static int old_halo_planes(int pass, int diag_mask) { return old_footprint_needed(pass, diag_mask) ? 36 : 9; }

static void check_masks(int pass, int diag_mask) {
  CHECK(kid::footprint_needed(pass, diag_mask) == old_footprint_needed(pass, diag_mask), "pass %d mask %#x", pass, (unsigned)diag_mask);
  CHECK(kid::nacc_live(pass, diag_mask) == old_nacc_active(pass, diag_mask), "pass %d mask %#x", pass, (unsigned)diag_mask);
  CHECK(kid::halo_plane_count(pass, diag_mask) == old_halo_planes(pass, diag_mask), "pass %d mask %#x", pass, (unsigned)diag_mask);
  const int nks[] = {1, 2, 9, 10, 36};
  for (int plane = 0; plane <= KID_NACC; ++plane) {
    for (int nk : nks)
      CHECK(kid::plane_range_live(plane, nk, pass, diag_mask) == old_chk_live(plane, nk, pass, diag_mask), "plane %d nk %d pass %d mask %#x", plane, nk, pass, (unsigned)diag_mask);
    const bool fold = kid::plane_range_live(plane, 1, pass, diag_mask) && !kid::ON_OCEAN_ALL.contains(plane);
    CHECK(fold == old_fold_value(plane, pass, diag_mask), "fold: plane %d pass %d mask %#x", plane, pass, (unsigned)diag_mask);
  }
}

int main() {
  // 1. the named ranges against the literals they replace
  CHECK(kid::ON_OCEAN_ALL.first == KID_A_MASS_ON_OCEAN && kid::ON_OCEAN_ALL.count == 36, "%d + %d", kid::ON_OCEAN_ALL.first, kid::ON_OCEAN_ALL.count);
  CHECK(kid::ON_OCEAN_VEL.first == KID_A_UVEL_ON_OCEAN && kid::ON_OCEAN_VEL.count == 18, "%d + %d", kid::ON_OCEAN_VEL.first, kid::ON_OCEAN_VEL.count);
  CHECK(kid::MASS_ON_OCEAN.first == KID_A_MASS_ON_OCEAN && kid::MASS_ON_OCEAN.count == 9 && kid::ON_OCEAN_SLOTS == 9, "mass family");
  const int first[4] = {KID_A_MASS_ON_OCEAN, KID_A_AREA_ON_OCEAN, KID_A_UVEL_ON_OCEAN, KID_A_VVEL_ON_OCEAN};
  for (int v = 0; v < 4; ++v) {
    CHECK(kid::on_ocean_family(v).first == KID_A_MASS_ON_OCEAN + 9 * v && kid::on_ocean_family(v).first == first[v] && kid::on_ocean_family(v).count == 9, "family %d", v);
    for (int plane = 0; plane <= KID_NACC; ++plane)
      CHECK(kid::on_ocean_family(v).contains(plane) == (plane >= first[v] && plane < first[v] + 9), "family %d plane %d", v, plane);
  }
  for (int plane = 0; plane <= KID_NACC; ++plane)
    CHECK(kid::ON_OCEAN_ALL.contains(plane) == (plane >= KID_A_MASS_ON_OCEAN && plane < KID_NACC_CORE), "plane %d", plane);
  // 2. liveness: no bit, every bit alone (all 32, the unused ones too), every pair, everything
  for (int pass = 0; pass < 2; ++pass) {
    check_masks(pass, 0);
    check_masks(pass, -1);
    for (int a = 0; a < 32; ++a)
      for (int b = a; b < 32; ++b) check_masks(pass, (int)((1u << a) | (1u << b)));
  }
  // 3. the stencil: slot s of the neighbour at (di, dj), as sum_up_spread_fields pairs them (IB:6126-6131)
  //   dmda = v(i,j,5) + ( ( (v(i-1,j-1,9)+v(i+1,j+1,1)) + (v(i+1,j-1,7)+v(i-1,j+1,3)) )
  //                     + ( (v(i-1,j,6)+v(i+1,j,4)) + (v(i,j-1,8)+v(i,j+1,2)) ) )
  static const int pairing[9][3] = {{0, 0, 5}, {-1, -1, 9}, {1, 1, 1}, {1, -1, 7}, {-1, 1, 3}, {-1, 0, 6}, {1, 0, 4}, {0, -1, 8}, {0, 1, 2}};
  bool slot_seen[10] = {};
  for (int k = 0; k < 9; ++k) {
    const kid::StencilPoint p = kid::NINE_POINT[k];
    CHECK(p.di == pairing[k][0] && p.dj == pairing[k][1] && p.slot == pairing[k][2], "entry %d: (%d, %d) slot %d", k, p.di, p.dj, p.slot);
    // the slot a berg at (i + di, j + dj) fills for its neighbour at (-di, -dj): slots count 1..9 from the south-west, row by row
    CHECK(p.slot == 5 - p.di - 3 * p.dj, "entry %d: slot %d is not the mirror of (%d, %d)", k, p.slot, p.di, p.dj);
    CHECK(p.slot >= 1 && p.slot <= 9 && !slot_seen[p.slot], "entry %d: slot %d twice", k, p.slot);
    if (p.slot >= 1 && p.slot <= 9) slot_seen[p.slot] = true;
  }
  // ... and the order of the additions, on values whose sum depends on it: v[dj + 1][di + 1][slot], bit by bit
  unsigned long long seed = 0x9e3779b97f4a7c15ull;
  for (int trial = 0; trial < 1000; ++trial) {
    double v[3][3][10];
    for (auto &row : v) for (auto &cell : row) for (double &x : cell) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      const int e = (int)((seed >> 20) & 63u) - 32;
      x = (double)(long long)(seed >> 11) / 9007199254740992.0 * (e >= 0 ? (double)(1ull << e) : 1.0 / (double)(1ull << -e)) * ((seed & 1u) ? -1. : 1.);
    }
#define V(di, dj, s) v[(dj) + 1][(di) + 1][s]
    const double want = V(0, 0, 5) + (((V(-1, -1, 9) + V(1, 1, 1)) + (V(1, -1, 7) + V(-1, 1, 3))) + ((V(-1, 0, 6) + V(1, 0, 4)) + (V(0, -1, 8) + V(0, 1, 2))));
#undef V
    const double got = kid::nine_point_sum([&](int di, int dj, int slot) { return v[dj + 1][di + 1][slot]; });
    CHECK(std::memcmp(&got, &want, sizeof(double)) == 0, "trial %d: %a, the reference's order gives %a", trial, got, want);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
