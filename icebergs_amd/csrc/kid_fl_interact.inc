// kid_fl_interact.inc -- footloose calving among interacting bergs (footloose with interactive_icebergs_on, mts=F), gfx950.
// Included inside the anonymous namespace of kid_hip.hip after kid_mts.inc (needs BergPtrs, MtsDev, MF / MI).
//   adjust_fl_berg_interactivity IB:2765-2841 (called at IB:5486)
//
// A footloose child is born with fl_k = -1 and neither feels nor exerts a contact force (interactive_force, calculate_force and
// its kin in kid_mts.inc).  This pass sets it to fl_k = -2 the first time no other berg is within contact range; from then on it
// collides like any other berg.  One lane per row.  A lane writes its own row's fl_k and reads no other row's, so the pass does
// not depend on the order of the rows and needs no atomics but the one count per wave a caller may ask for.  The two decisions
// -- which cells, which pairs -- are kid_fl_contact.hpp's.
__global__ void __launch_bounds__(256) fl_adjust_interactivity_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                                      const MtsDev *__restrict__ mt, const long long n, int *__restrict__ promoted) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  bool promote = false;
  if (k < n) {
    const BergPtrs &b = *bt;
    // every row that is not a child waiting to become interactive leaves after this one load
    if (MF(KID_B_FL_K, k) == -1. && MI(KID_BI_ALIVE, k) != 0 && MF(KID_B_HALO_BERG, k) < 0.5) {
      const kid_params &p = *pp; const MtsDev &m = *mt;
      const FlContactRule rule = fl_contact_rule(p.contact_cells_lon, p.contact_cells_lat, p.hexagonal_icebergs != 0, p.iceberg_bonds_on != 0,
                                                 g.latlon != 0, p.contact_distance, p.pi, p.Rearth);
      const FlWindow w = fl_contact_window(MI(KID_BI_INE, k), MI(KID_BI_JNE, k), p.contact_cells_lon, p.contact_cells_lat, g.isd, g.ied, g.jsd, g.jed);
      const int64_t id1 = b.id[k];
      const double lon1 = MF(KID_B_LON, k), lat1 = MF(KID_B_LAT, k);
      const double R1 = rule.radial_contact ? fl_contact_radius(rule, MF(KID_B_LENGTH, k), MF(KID_B_WIDTH, k)) : 0.;
      bool contact = false;
      for (int gj = w.j0; gj <= w.j1 && !contact; ++gj) for (int gi = w.i0; gi <= w.i1 && !contact; ++gi) {
        const int c = g.idx(gi, gj);
        const int q1 = m.cell_start[c + 1];
        for (int q = m.cell_start[c]; q < q1; ++q) {
          const int o = m.order[q];
          // the tables hold live rows only; a row that has died or been retired as a halo copy since they were built is nobody's partner
          if (MI(KID_BI_ALIVE, o) == 0 || MF(KID_B_HALO_BERG, o) >= 0.5) continue;
          const double R2 = rule.radial_contact ? fl_contact_radius(rule, MF(KID_B_LENGTH, o), MF(KID_B_WIDTH, o)) : 0.;
          if (fl_in_contact(rule, id1, lon1, lat1, R1, b.id[o], MF(KID_B_LON, o), MF(KID_B_LAT, o), R2)) { contact = true; break; }
        }
      }
      if (!contact) { MF(KID_B_FL_K, k) = -2.; promote = true; }
    }
  }
  if (promoted) {   // (uniform: every lane of the wave is here)
    const unsigned long long votes = __ballot(promote);
    if (votes != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(promoted, __popcll(votes));
  }
}
