// kid_mts.inc -- multiple-time-stepping velocity Verlet with bonded (DEM) sub-steps on the SoA, gfx950.
// Included inside the anonymous namespace of kid_hip.hip (needs BergPtrs).
//   evolve_icebergs_mts IB:6576-7078    accel_mts IB:1278-1706    accel_explicit_inner_mts IB:1710-1947
//   interactive_force / calculate_force IB:480-804    calculate_unbonded_same_conglom_dem_force IB:807-955
//   calculate_force_dem IB:959-1242     break_bonds_dem FW:4713-4799     set_conglom_ids FW:2601-2731
//   orig_bond_length FW:4589-4614       quad_interp_from_agrid FW:7163-7252
//
// Layout.  Bergs keep their rows for the whole run (no re-binning while bonds exist); a bond list is `bcount[k]`
// slots of slot-major arrays x[s*stride + k], so lane k reading slot s is a coalesced access.  The reference walks
// cells j-outer/i-inner and the sorted list inside a cell; that traversal order is materialised once per step as
// rank[row] / order[rank] (+ cell_start[] for the contact searches) by a radix sort on (cell, inorder key).
// One sweep of the reference loop over all bergs becomes one launch with one lane per berg; what made the reference
// loop order dependent is handled explicitly: with save_bond_forces a bond pair is evaluated once, by the berg that
// comes first in the traversal (rank[k] < rank[other]) -- here a per-bond pass (bond_pass_kernel) in which that
// "primary" side computes the pair and writes both sides' bond records, followed by a per-berg pass that only reads.
// A bond that fractures on this sweep is tagged 3 until both sides have consumed the forces stored with it.

struct MtsDev {
  int32_t *bcount; int64_t *bother_id; int32_t *bbroken; double *bf[KID_NBOND_F64];
  int32_t *bother_row, *bother_slot;
  long long stride;
  int mb, nperm;
  int32_t *rank, *order, *cell_start;
  int32_t *cell_conglom;   // conglomerate id shared by every berg of the cell, -1 if mixed (skips whole cells in the collision search)
  int32_t *label, *root_flag, *root_scan;
  double *red;   // [0] usum [1] usum1 [2] usum2 [3] had_collision [4] bond_break_detected [5] changed [6] nbroken
  const double *lonc, *latc, *glon;
  double constant_area, constant_radius, dem_K_damp, mts_fast_dt;
  double *rec;             // 3 copies x capacity x 8 doubles: what one berg reads of another during a sub-step, as one 64-byte record
                           // {lon_old, lat_old, uvel_old, vvel_old, ang_vel, rot, -, -} per berg; the fused sub-step loop
                           // (mts_substeps_kernel) rotates through the copies
};
// What a berg reads of ANOTHER berg during a sub-step (and of itself, in the same places of the reference's code)
struct DemRec { double lon, lat, u, v, w, rot; };
enum { MR_USUM = 0, MR_USUM1, MR_USUM2, MR_COLLISION, MR_BREAK, MR_CHANGED, MR_NBROKEN, MR_NTICKETS, MR_NERR, MR_COUNT };

#define MB_S(s, k) ((size_t)(s) * (size_t)m.stride + (size_t)(k))
#define MF(fld, k) (b.f[fld][k])
#define MI(fld, k) (b.i[fld][k])
#define MBD(fld, s, k) (m.bf[fld][MB_S(s, k)])
__device__ __forceinline__ DemRec dem_rec_main(const BergPtrs &b, long long k) {
  return DemRec{MF(KID_B_LON_OLD, k), MF(KID_B_LAT_OLD, k), MF(KID_B_UVEL_OLD, k), MF(KID_B_VVEL_OLD, k), MF(KID_B_ANG_VEL, k), MF(KID_B_ROT, k)};
}

__device__ __forceinline__ void grid_to_meters(const DevGrid &g, const kid_params &p, double lat_ref, double &dx_dlon, double &dy_dlat) {  // IB:444-459
  if (g.latlon) { dx_dlon = (p.pi / 180.) * p.Rearth * cos((lat_ref) * (p.pi / 180.)); dy_dlat = (p.pi / 180.) * p.Rearth; }
  else { dx_dlon = 1.; dy_dlat = 1.; }
}
__device__ __forceinline__ double radius_of(const kid_params &p, double A) {  // IB:693-705
  if (p.hexagonal_icebergs) return sqrt(A / (2. * sqrt(3.)));
  if (p.iceberg_bonds_on) return 0.5 * sqrt(A);
  return sqrt(A / p.pi);
}
__device__ __forceinline__ bool is_partner(const MtsDev &m, long long k, int o) {  // the id-negation mark, IB:537, 1772
  if (m.mb == 0) return false;
  const int cnt = m.bcount[k];
  for (int s = 0; s < cnt; ++s) if (m.bother_row[MB_S(s, k)] == o) return true;
  return false;
}

struct IaSum { double IA_x, IA_y, P11, P12, P21, P22, Ptu_x, Ptu_y; };

// IB:611-804.  c_crit: -1 absent, 0 .false., 1 .true.
__device__ __noinline__ void calculate_force(const DevGrid &g, const kid_params &p, const BergPtrs &b, long long k, long long o, IaSum &S,
                                             double u0, double v0, double u1, double v1, bool bonded, int c_crit) {
  if (!(b.id[k] != b.id[o] && MF(KID_B_FL_K, k) != -1 && MF(KID_B_FL_K, o) != -1)) return;
  const double T1 = MF(KID_B_THICKNESS, k), lon1 = MF(KID_B_LON_OLD, k), lat1 = MF(KID_B_LAT_OLD, k);
  const double T2 = MF(KID_B_THICKNESS, o), lon2 = MF(KID_B_LON_OLD, o), lat2 = MF(KID_B_LAT_OLD, o);
  const double u2 = MF(KID_B_UVEL_OLD, o), v2 = MF(KID_B_VVEL_OLD, o);
  double A1, M1, A2, M2;
  if (p.constant_interaction_LW && p.mts && bonded) {
    A1 = p.constant_length * p.constant_width; M1 = A1 * T1 * p.rho_bergs; A2 = A1; M2 = A2 * T2 * p.rho_bergs;
  } else {
    M1 = MF(KID_B_MASS, k); A1 = MF(KID_B_LENGTH, k) * MF(KID_B_WIDTH, k);
    M2 = MF(KID_B_MASS, o); A2 = MF(KID_B_LENGTH, o) * MF(KID_B_WIDTH, o);
  }
  const double dlon = lon1 - lon2, dlat = lat1 - lat2;
  double dx_dlon, dy_dlat; grid_to_meters(g, p, 0.5 * (lat1 + lat2), dx_dlon, dy_dlat);
  const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
  const double r_dist = sqrt((rx * rx) + (ry * ry));
  const double R1 = radius_of(p, A1), R2 = radius_of(p, A2);
  const double M_min = dmin(M1, M2);
  double crit_dist, spring_coef;
  if (bonded) { crit_dist = R1 + R2; spring_coef = p.spring_coef; }
  else {
    spring_coef = p.contact_spring_coef;
    if (c_crit == 1) { crit_dist = R1 + R2; spring_coef = p.spring_coef; }
    else crit_dist = dmax(R1 + R2, p.contact_distance);
  }
  double radial = p.radial_damping_coef, tang = p.tangental_damping_coef;
  if (p.critical_interaction_damping_on) {
    radial = 2. * sqrt(spring_coef);
    if (p.tang_crit_int_damp_on) tang = (2. * sqrt(spring_coef)) / 4;
  }
  bool tbonded = bonded;
  if (bonded && !(p.mts || (p.contact_distance > 0.) || (p.contact_spring_coef != p.spring_coef)))
    if (!(r_dist > crit_dist)) tbonded = false;
  if ((r_dist > 0.) && (tbonded || (r_dist < crit_dist && !bonded))) {
    const double accel_spring = spring_coef * (M_min / M1) * (crit_dist - r_dist);
    S.IA_x = S.IA_x + (accel_spring * (rx / r_dist));
    S.IA_y = S.IA_y + (accel_spring * (ry / r_dist));
    double P_11 = (rx * rx) / (r_dist * r_dist), P_12 = (rx * ry) / (r_dist * r_dist);
    double P_21 = (rx * ry) / (r_dist * r_dist), P_22 = (ry * ry) / (r_dist * r_dist);
    double coef = radial * (M_min / M1);
    if (p.scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    S.P11 += coef * P_11; S.P12 += coef * P_12; S.P21 += coef * P_21; S.P22 += coef * P_22;
    S.Ptu_x = S.Ptu_x + (coef * ((P_11 * u2) + (P_12 * v2)));
    S.Ptu_y = S.Ptu_y + (coef * ((P_12 * u2) + (P_22 * v2)));
    P_11 = 1 - P_11; P_12 = -P_12; P_21 = -P_21; P_22 = 1 - P_22;
    coef = tang * (M_min / M1);
    if (p.scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    S.P11 += coef * P_11; S.P12 += coef * P_12; S.P21 += coef * P_21; S.P22 += coef * P_22;
    S.Ptu_x = S.Ptu_x + (coef * ((P_11 * u2) + (P_12 * v2)));
    S.Ptu_y = S.Ptu_y + (coef * ((P_12 * u2) + (P_22 * v2)));
  }
}

// IB:480-607
__device__ __noinline__ void interactive_force(const DevGrid &g, const kid_params &p, const BergPtrs &b, const MtsDev &m, long long k, int mts_part,
                                               IaSum &S, double u0, double v0, double u1, double v1) {
  S = IaSum{0., 0., 0., 0., 0., 0., 0., 0.};
  if (MF(KID_B_FL_K, k) == -1) return;
  const int ine = MI(KID_BI_INE, k), jne = MI(KID_BI_JNE, k);
  const int nc_x = p.contact_cells_lon, nc_y = p.contact_cells_lat;
  if (p.mts || (p.contact_distance > 0.) || (p.contact_spring_coef != p.spring_coef)) {
    if (!p.mts || (p.mts && mts_part == 3)) {
      if (p.iceberg_bonds_on) {
        const int cnt = m.bcount[k];
        for (int s = 0; s < cnt; ++s) {
          const int o = m.bother_row[MB_S(s, k)];
          if (o >= 0) calculate_force(g, p, b, k, o, S, u0, v0, u1, v1, true, -1);
        }
        const int j0 = max(jne - 2, g.jsd + 1), j1 = min(jne + 2, g.jed), i0 = max(ine - 2, g.isd + 1), i1 = min(ine + 2, g.ied);
        for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi) {
          const int c = g.idx(gi, gj);
          for (int q = m.cell_start[c]; q < m.cell_start[c + 1]; ++q) {
            const int o = m.order[q];
            if (!is_partner(m, k, o) && MI(KID_BI_CONGLOM_ID, o) == MI(KID_BI_CONGLOM_ID, k))
              calculate_force(g, p, b, k, o, S, u0, v0, u1, v1, false, 1);
          }
        }
      }
    }
    if (!(p.mts && mts_part == 3)) {
      const int j0 = max(jne - nc_y, g.jsd), j1 = min(jne + nc_y, g.jed), i0 = max(ine - nc_x, g.isd), i1 = min(ine + nc_x, g.ied);
      for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi) {
        const int c = g.idx(gi, gj);
        if (m.cell_conglom[c] == MI(KID_BI_CONGLOM_ID, k)) continue;  // nothing but the berg's own conglomerate in there
        for (int q = m.cell_start[c]; q < m.cell_start[c + 1]; ++q) {
          const int o = m.order[q];
          if (MI(KID_BI_CONGLOM_ID, o) != MI(KID_BI_CONGLOM_ID, k)) calculate_force(g, p, b, k, o, S, u0, v0, u1, v1, false, -1);
        }
      }
    }
  } else {
    for (int gj = jne - 1; gj <= jne + 1; ++gj) for (int gi = ine - 1; gi <= ine + 1; ++gi) {
      const int c = g.idx(gi, gj);
      for (int q = m.cell_start[c]; q < m.cell_start[c + 1]; ++q) calculate_force(g, p, b, k, m.order[q], S, u0, v0, u1, v1, false, -1);
    }
    if (p.iceberg_bonds_on) {
      const int cnt = m.bcount[k];
      for (int s = 0; s < cnt; ++s) {
        const int o = m.bother_row[MB_S(s, k)];
        if (o >= 0) calculate_force(g, p, b, k, o, S, u0, v0, u1, v1, true, -1);
      }
    }
  }
}

// IB:1861-1877: the loads of the beam tests of Wang (2020), sections 3.1 (simply supported: no vertical load on the two ends,
// a point load at the centre) and 3.2 (cantilever: the load on the free end); elements are told apart by their start_lon
__device__ __forceinline__ void dem_beam_test_load(const kid_params &p, double start_lon, double &F_y, double &Fd_y) {
  if (p.dem_beam_test == 1) {
    if (start_lon == p.dem_tests_start_lon || start_lon == p.dem_tests_end_lon) { F_y = 0.0; Fd_y = 0.0; }
    else if (start_lon == 0.5 * (p.dem_tests_start_lon + p.dem_tests_end_lon)) F_y = F_y - 1.5e5;
  } else if (p.dem_beam_test == 2) {
    if (start_lon == p.dem_tests_end_lon) F_y = F_y - 1.5e10 / 3.;
  }
}

// Is a pair certainly farther apart than the reach of calculate_unbonded_same_conglom_dem_force (IB:858-871: it returns when
// (R1+R2)**2 <= r_dist)?  Same expressions; the margin covers the last bit of the routine's own pow(): "true" here means the
// routine would return there, "false" leaves the decision to it.
__device__ __forceinline__ bool dem_out_of_reach(const DevGrid &g, const kid_params &p, const MtsDev &m, double lon_k, double lat_k, double lon_o, double lat_o,
                                                 double A1, double A2) {
  const double dlon = lon_k - lon_o, dlat = lat_k - lat_o;
  double dx_dlon, dy_dlat; grid_to_meters(g, p, 0.5 * (lat_k + lat_o), dx_dlon, dy_dlat);
  const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
  const double r_dist = (rx * rx) + (ry * ry);
  const double reach = p.constant_interaction_LW ? 2 * m.constant_radius : radius_of(p, A1) + radius_of(p, A2);
  return reach * reach * (1. + 1.e-12) <= r_dist;
}

// IB:807-955; K, O: the old positions and velocities of the two bergs
__device__ __noinline__ void unbonded_dem_force(const DevGrid &g, const kid_params &p, const BergPtrs &b, const MtsDev &m, const DemRec K, const DemRec O, long long k, long long o,
                                                double &IA_x, double &IA_y, double &IAd_x, double &IAd_y, double u0, double v0, double u1, double v1) {
  if (!(b.id[k] != b.id[o] && MF(KID_B_FL_K, k) != -1 && MF(KID_B_FL_K, o) != -1)) return;
  const double lat_k = K.lat, lat_o = O.lat;
  const double uold_k = K.u, vold_k = K.v, uold_o = O.u, vold_o = O.v;
  const double dlon = K.lon - O.lon, dlat = lat_k - lat_o;
  double dx_dlon, dy_dlat; grid_to_meters(g, p, 0.5 * (lat_k + lat_o), dx_dlon, dy_dlat);
  const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
  double r_dist = (rx * rx) + (ry * ry);
  double R1, R2, M1, M2;
  if (p.constant_interaction_LW) {
    if (kid_pow(2 * m.constant_radius, 2.) <= r_dist) return;
    R1 = m.constant_radius;
    M1 = m.constant_area * MF(KID_B_THICKNESS, k) * p.rho_bergs;
    M2 = m.constant_area * MF(KID_B_THICKNESS, o) * p.rho_bergs;
    R2 = R1;
  } else {
    const double A1 = MF(KID_B_LENGTH, k) * MF(KID_B_WIDTH, k), A2 = MF(KID_B_LENGTH, o) * MF(KID_B_WIDTH, o);
    R1 = radius_of(p, A1); R2 = radius_of(p, A2);
    if (kid_pow(R1 + R2, 2.) <= r_dist) return;
    M1 = MF(KID_B_MASS, k); M2 = MF(KID_B_MASS, o);
  }
  r_dist = sqrt(r_dist);
  const double u2 = uold_o, v2 = vold_o;
  const double M_min = dmin(M1, M2), crit_dist = R1 + R2, spring_coef = p.spring_coef;
  double radial = p.radial_damping_coef, tang = p.tangental_damping_coef;
  if (p.critical_interaction_damping_on) {
    radial = 2. * sqrt(spring_coef);
    if (p.tang_crit_int_damp_on) tang = (2. * sqrt(spring_coef)) / 4;
  }
  if ((r_dist > 0.) && (r_dist < crit_dist)) {
    const double accel_spring = spring_coef * (M_min / M1) * (crit_dist - r_dist);
    IA_x = IA_x + (accel_spring * (rx / r_dist));
    IA_y = IA_y + (accel_spring * (ry / r_dist));
    double P_11 = (rx * rx) / (r_dist * r_dist), P_12 = (rx * ry) / (r_dist * r_dist), P_22 = (ry * ry) / (r_dist * r_dist);
    double coef = radial * (M_min / M1);
    if (p.scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    double Pia11 = coef * P_11, Pia12 = coef * P_12, Pia22 = coef * P_22;
    P_11 = 1 - P_11; P_12 = -P_12; P_22 = 1 - P_22;
    coef = tang * (M_min / M1);
    if (p.scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    Pia11 = Pia11 + coef * P_11; Pia12 = Pia12 + coef * P_12; Pia22 = Pia22 + coef * P_22;
    const double du = uold_o - uold_k, dv = vold_o - vold_k;
    IAd_x = IAd_x + Pia11 * du + Pia12 * dv;
    IAd_y = IAd_y + Pia12 * du + Pia22 * dv;
  }
}

// IB:959-1242 calculate_force_dem as a function of the pair: `k` is the side that evaluates (the primary, the berg the
// reference's sweep reaches first), `o` its partner; t1, t2, relrot0 are the primary's copies of the bond's tangential
// displacement and relative rotation (the partner's copies are their negatives).  Nothing is written here.
struct PairOut {
  int status;   // 0 evaluated; 1 not an interacting pair (same id, or a footloose child): the stored forces are zeroed, IB:1000-1004; 2 zero separation (FATAL IB:1054)
  double len, tg1, tg2, relrot, nstress, sstress, Fx, Fy, Fdx, Fdy, Tq, Tdq, To_q;
  bool broke;
};
// what of a pair does not change over the sub-steps of a step
struct PairConst { bool interacting; double Tk, To, M1, M2, R1, R2, Rmin, T_Rmin, l0, damping_coef; Rcp rl0, rss, r12l0; };
__device__ __forceinline__ PairConst pair_const(const kid_params &p, const BergPtrs &b, const MtsDev &m, long long k, long long o) {
  PairConst c{};
  c.interacting = b.id[k] != b.id[o] && MF(KID_B_FL_K, k) != -1 && MF(KID_B_FL_K, o) != -1;
  const double hexdenom = 1. / (2. * sqrt(3.));
  const double Tk = MF(KID_B_THICKNESS, k), To = MF(KID_B_THICKNESS, o);
  c.Tk = Tk; c.To = To;
  if (p.constant_interaction_LW) {
    c.M1 = m.constant_area * Tk * p.rho_bergs; c.M2 = m.constant_area * To * p.rho_bergs;
    c.R1 = m.constant_radius; c.R2 = c.R1; c.Rmin = c.R1; c.l0 = 2 * c.R1; c.T_Rmin = To;
  } else {
    c.M1 = MF(KID_B_MASS, k); c.M2 = MF(KID_B_MASS, o);
    const double A1 = MF(KID_B_LENGTH, k) * MF(KID_B_WIDTH, k), A2 = MF(KID_B_LENGTH, o) * MF(KID_B_WIDTH, o);
    if (p.hexagonal_icebergs) { c.R1 = sqrt(A1 * hexdenom); c.R2 = sqrt(A2 * hexdenom); }
    else { c.R1 = 0.5 * sqrt(A1); c.R2 = 0.5 * sqrt(A2); }
    if (c.R1 < c.R2) { c.Rmin = c.R1; c.T_Rmin = Tk; } else { c.Rmin = c.R2; c.T_Rmin = To; }
    c.l0 = c.R1 + c.R2;
  }
  c.damping_coef = p.dem_damping_coef * sqrt(m.dem_K_damp * c.M1 * c.M2 / (c.M1 + c.M2));
  c.rl0 = kid_rcp(c.l0); c.rss = kid_rcp(c.l0 * 2.0 * (1.0 + p.poisson)); c.r12l0 = kid_rcp(12. * c.l0);
  return c;
}
// calculate_force_dem in three pieces without control flow between them (every `if` of the reference is a select here, on
// the same values): the geometry and the tangential update, the sine of the relative rotation, the stresses and the
// outcome.  One pair after the other they are what they were; the fused sub-step kernel runs the first piece for all of a
// berg's bonds, then the sines, then the last piece, so that the four independent chains of fp64 operations can be
// interleaved by the scheduler instead of each waiting out its own latencies (one wave per SIMD there: nobody else to
// issue from).
struct PairMid {
  bool interacting, zero_len;
  double len, half_delta, L, Thick, Fn_x, Fn_y, ur, vr, dw, tg1, tg2, Fs_x, Fs_y, sstress, Ts, relrot, arg;
};
__device__ __forceinline__ PairMid pair_geom(const DevGrid &g, const kid_params &p, const MtsDev &m, const PairConst &c, const DemRec &K, const DemRec &O,
                                             double t1, double t2, double relrot0, double dt) {
  PairMid q;
  q.interacting = c.interacting;
  const double Tk = c.Tk, To = c.To, R1 = c.R1, R2 = c.R2, Rmin = c.Rmin, l0 = c.l0, T_Rmin = c.T_Rmin;
  const double lat_k = K.lat, lat_o = O.lat;
  double dx_dlon, dy_dlat; grid_to_meters(g, p, 0.5 * (lat_k + lat_o), dx_dlon, dy_dlat);
  const double rx = (K.lon - O.lon) * dx_dlon;
  const double ry = (lat_k - lat_o) * dy_dlat;
  const double len = kid_sqrt((rx * rx) + (ry * ry));
  q.len = len;
  q.zero_len = len == 0;
  const Rcp rlen = kid_rcp(q.zero_len ? 1. : len);   // (a pair at zero distance is an error, IB:1054: nothing below is used then)
  const double n1 = rx * rlen, n2 = ry * rlen;
  const double half_delta = 0.5 * (l0 - len);
  const double RR1 = R1 - half_delta, RR2 = R2 - half_delta;
  const double RR1x = RR1 * n1, RR1y = RR1 * n2, RR2x = RR2 * n1, RR2y = RR2 * n2;
  const double L = 2.0 * (Rmin + (Rmin - half_delta) * fabs(R1 - R2) * rlen);
  const double Thick = T_Rmin + (Rmin - half_delta) * fabs(Tk - To) * rlen;
  double Fn_x = p.dem_spring_coef * Thick * 2. * half_delta * L * c.rl0;
  const double Fn_y = Fn_x * n2; Fn_x = Fn_x * n1;
  const double ur = K.u - O.u, vr = K.v - O.v;
  const double wk = K.w, wo = O.w;
  double tg1, tg2;
  {
    const double tmag = t1 * t1 + t2 * t2;
    const double tangdotnt = t1 * n1 + t2 * n2;
    double tangd1p = t1 - tangdotnt * n1, tangd2p = t2 - tangdotnt * n2;
    const double tmagp = tangd1p * tangd1p + tangd2p * tangd2p;
    const bool rescale = tmagp > 0.;
    const double t_rat = kid_sqrt(kid_div(tmag, rescale ? tmagp : 1.));
    tangd1p = rescale ? t_rat * tangd1p : 0.; tangd2p = rescale ? t_rat * tangd2p : 0.;
    const double rotu = RR1y * wk + RR2y * wo;
    const double rotv = -(RR1x * wk + RR2x * wo);
    const double ur2 = ur + rotu, vr2 = vr + rotv;
    double up = ur2 * n1 + vr2 * n2; const double vp = up * n2; up = up * n1;
    tg1 = tangd1p + (ur2 - up) * dt; tg2 = tangd2p + (vr2 - vp) * dt;
  }
  double ss_factor = -L * Thick * p.dem_spring_coef * c.rss;
  if (p.ignore_tangential_force) ss_factor = 0.;
  const double Fs_x = ss_factor * tg1, Fs_y = ss_factor * tg2;
  q.half_delta = half_delta; q.L = L; q.Thick = Thick; q.Fn_x = Fn_x; q.Fn_y = Fn_y; q.ur = ur; q.vr = vr; q.dw = wk - wo;
  q.tg1 = tg1; q.tg2 = tg2; q.Fs_x = Fs_x; q.Fs_y = Fs_y;
  q.sstress = kid_div(kid_sqrt(Fs_x * Fs_x + Fs_y * Fs_y), L * Thick);
  q.Ts = -(RR1x * Fs_y - RR1y * Fs_x);
  q.relrot = relrot0 + (wk - wo) * dt;
  q.arg = K.rot - O.rot;
  return q;
}
__device__ __forceinline__ double pair_theta(const kid_params &p, double arg) { return p.orig_dem_moment_of_inertia ? arg : sin(arg); }
__device__ __forceinline__ PairOut pair_finish(const kid_params &p, const PairConst &c, const PairMid &q, double theta) {
  PairOut r{};
  r.len = q.len; r.tg1 = q.tg1; r.tg2 = q.tg2; r.sstress = q.sstress; r.relrot = q.relrot;
  const double L = q.L, Thick = q.Thick;
  const double Tr = p.orig_dem_moment_of_inertia ? -(p.dem_spring_coef * c.rl0) * (2. / 3.) * kid_cube(0.5 * L) * Thick * theta
                                                 : -p.dem_spring_coef * kid_cube(L) * Thick * theta * c.r12l0;
  const double nstress = (p.dem_spring_coef * c.rl0) * (-2 * q.half_delta + fabs(theta * 0.5 * L));
  r.nstress = nstress;
  const bool broke = p.break_bonds_on_sub_steps && p.fracture_criterion_stress && (nstress > p.frac_thres_n || q.sstress > p.frac_thres_t);
  const double damping_coef = c.damping_coef;
  const double Fdx = -damping_coef * q.ur, Fdy = -damping_coef * q.vr;
  const bool pull = nstress < 0;   // a bond that fails in compression-free state leaves no force behind (IB:1176-1186)
  r.broke = broke;
  r.Fx = broke ? (pull ? q.Fn_x : 0.) : q.Fn_x + q.Fs_x;
  r.Fy = broke ? (pull ? q.Fn_y : 0.) : q.Fn_y + q.Fs_y;
  r.Fdx = (broke && !pull) ? 0. : Fdx;
  r.Fdy = (broke && !pull) ? 0. : Fdy;
  r.Tq = broke ? 0. : q.Ts + Tr;
  r.Tdq = broke ? 0. : -damping_coef * q.dw;
  r.To_q = broke ? 0. : q.Ts - Tr;
  // 1: not an interacting pair, 2: zero separation (FATAL IB:1054), 3: sub-step fracture without the stress criterion (FATAL IB:1206; the forces are still returned)
  r.status = !q.interacting ? 1 : (q.zero_len ? 2 : ((!broke && p.break_bonds_on_sub_steps && !p.fracture_criterion_stress) ? 3 : 0));
  if (r.status == 1 || r.status == 2) r.broke = false;
  return r;
}
__device__ __forceinline__ PairOut pair_force_dem(const DevGrid &g, const kid_params &p, const MtsDev &m, const PairConst &c, const DemRec &K, const DemRec &O,
                                                  double t1, double t2, double relrot0, double dt) {
  const PairMid q = pair_geom(g, p, m, c, K, O, t1, t2, relrot0, dt);
  return pair_finish(p, c, q, pair_theta(p, q.arg));
}

__device__ __forceinline__ bool mts_active(const BergPtrs &b, long long k) {
  return MI(KID_BI_ALIVE, k) != 0 && MF(KID_B_STATIC_BERG, k) < 0.5 && MI(KID_BI_CONGLOM_ID, k) != 0;
}
// (savestress, save_bond_forces): the primary side (k,s) evaluates the pair and writes both records
__device__ __forceinline__ void calculate_force_dem(const DevGrid &g, const kid_params &p, const BergPtrs &b, const MtsDev &m, long long k, int s, double dt) {
  const int o = m.bother_row[MB_S(s, k)];
  const int so = m.bother_slot[MB_S(s, k)];
  const PairOut r = pair_force_dem(g, p, m, pair_const(p, b, m, k, o), dem_rec_main(b, k), dem_rec_main(b, o), MBD(KID_BOND_TANGD1, s, k), MBD(KID_BOND_TANGD2, s, k), MBD(KID_BOND_REL_ROTATION, s, k), dt);
  if (r.status == 1) {
    MBD(KID_BOND_F_X, s, k) = 0.; MBD(KID_BOND_F_Y, s, k) = 0.; MBD(KID_BOND_FD_X, s, k) = 0.; MBD(KID_BOND_FD_Y, s, k) = 0.;
    MBD(KID_BOND_T, s, k) = 0.; MBD(KID_BOND_T_D, s, k) = 0.;
    if (so >= 0) { MBD(KID_BOND_F_X, so, o) = 0.; MBD(KID_BOND_F_Y, so, o) = 0.; MBD(KID_BOND_FD_X, so, o) = 0.; MBD(KID_BOND_FD_Y, so, o) = 0.;
                   MBD(KID_BOND_T, so, o) = 0.; MBD(KID_BOND_T_D, so, o) = 0.; }
    return;
  }
  MBD(KID_BOND_LENGTH, s, k) = r.len;
  if (r.status == 2) { unsafeAtomicAdd(m.red + MR_NERR, 1.); return; }  // FATAL IB:1054
  if (r.status == 3) unsafeAtomicAdd(m.red + MR_NERR, 1.);              // FATAL IB:1206
  MBD(KID_BOND_TANGD1, s, k) = r.tg1; MBD(KID_BOND_TANGD2, s, k) = r.tg2;
  MBD(KID_BOND_SSTRESS, s, k) = r.sstress; MBD(KID_BOND_REL_ROTATION, s, k) = r.relrot; MBD(KID_BOND_NSTRESS, s, k) = r.nstress;
  if (so >= 0) {
    MBD(KID_BOND_NSTRESS, so, o) = r.nstress; MBD(KID_BOND_SSTRESS, so, o) = r.sstress; MBD(KID_BOND_REL_ROTATION, so, o) = -r.relrot;
    MBD(KID_BOND_TANGD1, so, o) = -r.tg1; MBD(KID_BOND_TANGD2, so, o) = -r.tg2; MBD(KID_BOND_LENGTH, so, o) = r.len;
  }
  if (r.broke) m.red[MR_BREAK] = 1.;
  MBD(KID_BOND_F_X, s, k) = r.Fx; MBD(KID_BOND_F_Y, s, k) = r.Fy; MBD(KID_BOND_FD_X, s, k) = r.Fdx; MBD(KID_BOND_FD_Y, s, k) = r.Fdy;
  MBD(KID_BOND_T, s, k) = r.Tq; MBD(KID_BOND_T_D, s, k) = r.Tdq;
  if (so >= 0) {
    MBD(KID_BOND_F_X, so, o) = -r.Fx; MBD(KID_BOND_F_Y, so, o) = -r.Fy; MBD(KID_BOND_FD_X, so, o) = -r.Fdx; MBD(KID_BOND_FD_Y, so, o) = -r.Fdy;
    MBD(KID_BOND_T, so, o) = r.To_q; MBD(KID_BOND_T_D, so, o) = -r.Tdq;
  }
  if (r.broke) {
    m.bbroken[MB_S(s, k)] = 3;
    double nb = 1.;
    if (p.use_broken_bonds_for_substep_contact) atomicSub(&MI(KID_BI_N_BONDS, k), 1);
    if (so >= 0) {
      m.bbroken[MB_S(so, o)] = mts_active(b, o) ? 3 : 1; nb = 2.;   // a partner that is not swept never consumes the forces: broken at once, as the reference leaves it
      if (p.use_broken_bonds_for_substep_contact) atomicSub(&MI(KID_BI_N_BONDS, o), 1);
    }
    unsafeAtomicAdd(m.red + MR_NBROKEN, nb);
  }
}

// one lane per bond slot (slot-major: a wave holds one slot of 64 consecutive bergs, so the slot-major tables are read
// coalesced); every unbroken bond whose primary side this berg is gets evaluated (IB:1791-1795 via IB:1757-1770)
__global__ void __launch_bounds__(256) bond_pass_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                        const MtsDev *__restrict__ mt, const long long n, const double dt) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  const BergPtrs &b = *bt; const MtsDev &m = *mt; const kid_params &p = *pp;
  if (q >= n * (long long)m.mb) return;
  const int s = (int)(q / n);
  const long long k = q - (long long)s * n;
  // every address below is valid for any (s, k): issue the loads together and test afterwards (as a chain of early
  // returns each test waited for its own round trip to memory: the kernel is ~200 k lanes of pure latency)
  const int cnt = m.bcount[k], broken = m.bbroken[MB_S(s, k)], o = m.bother_row[MB_S(s, k)], rank_k = m.rank[k];
  const bool act_k = mts_active(b, k);
  if (s >= cnt || broken != 0 || o < 0 || !act_k) return;
  // the other side evaluates the pair if it is swept first; a berg that is not swept at all never does
  const int rank_o = m.rank[o];
  const bool act_o = mts_active(b, o);
  if (act_o && rank_o < rank_k) return;
  calculate_force_dem(g, p, b, m, k, s, dt);
}

__device__ __forceinline__ double speed_limit_dx(const DevGrid &g, int i, int j) {   // the cell's length scale of the speed limit
  return dmin(0.5 * (g.dx[g.idx(i, j)] + g.dx[g.idx(i, j - 1)]), 0.5 * (g.dy[g.idx(i, j)] + g.dy[g.idx(i - 1, j)]));
}
__device__ __forceinline__ void speed_limit(const DevGrid &g, const kid_params &p, const MtsDev &m, int i, int j, double dt, double &uveln, double &vveln, double loc_dx_known = -1.) {
  if ((p.speed_limit > 0.) || (p.speed_limit == -1.)) {
    const double speed = sqrt(uveln * uveln + vveln * vveln);
    if (speed > 0.) {
      const double loc_dx = loc_dx_known >= 0. ? loc_dx_known : speed_limit_dx(g, i, j);
      const double new_speed = loc_dx / dt * p.speed_limit;
      if (new_speed < speed && p.speed_limit > 0.) {
        uveln = uveln * (new_speed / speed); vveln = vveln * (new_speed / speed);
        unsafeAtomicAdd(m.red + MR_NTICKETS, 1.);
      }
    }
  }
}

// IB:1278-1706
__device__ __noinline__ void accel_mts(const DevGrid &g, const kid_params &p, const BergPtrs &b, const MtsDev &m, long long k, int mts_part,
                                       bool only_interactive, int i, int j, double lat, double &uvel, double &vvel, double &uvel0, double &vvel0,
                                       double dt, double &ax, double &ay, double &axn, double &ayn, double &bxn, double &byn, double &Fdc_x, double &Fdc_y) {
  const double pi_180 = p.pi / 180.;
  const double scaling = 0.5, Cr0 = 0.06;
  double u_star = uvel0 + (axn * (dt / 2.)), v_star = vvel0 + (ayn * (dt / 2.));
  if (mts_part == 1) {
    u_star = MF(KID_B_UVEL, k); v_star = MF(KID_B_VVEL, k);
    uvel0 = MF(KID_B_UVEL, k); vvel0 = MF(KID_B_VVEL, k);
    uvel = MF(KID_B_UVEL, k); vvel = MF(KID_B_VVEL, k);
  }
  axn = 0.; ayn = 0.; bxn = 0.; byn = 0.;
  IaSum S{0., 0., 0., 0., 0., 0., 0., 0.};
  double uo = 0, vo = 0, ua = 0, va = 0, ui = 0, vi = 0, ssh_x = 0, ssh_y = 0, f_cori = 0, c_ocn = 0, c_atm = 0, c_ice = 0, c_gnd = 0;
  double wave_rad = 0, uwave = 0, vwave = 0;
  const bool ia_on = p.interactive_icebergs_on != 0;
  if (!only_interactive) {
    uo = MF(KID_B_UO, k); vo = MF(KID_B_VO, k); ua = MF(KID_B_UA, k); va = MF(KID_B_VA, k); ui = MF(KID_B_UI, k); vi = MF(KID_B_VI, k);
    ssh_x = MF(KID_B_SSH_X, k); ssh_y = MF(KID_B_SSH_Y, k);
    double hi = MF(KID_B_HI, k); const double od = MF(KID_B_OD, k);
    if (g.latlon && !p.use_f_plane) f_cori = (2. * p.omega) * sin(pi_180 * lat);
    else f_cori = (2. * p.omega) * sin(pi_180 * p.lat_ref);
    const double M = MF(KID_B_MASS, k), T = MF(KID_B_THICKNESS, k);
    const double D = (p.rho_bergs / RHO_SEAWATER) * T, F = T - D;
    const double W = MF(KID_B_WIDTH, k), L = MF(KID_B_LENGTH, k);
    hi = dmin(hi, D);
    const double D_hi = dmax(0., D - hi);
    double L2, W2;
    if (p.dem && p.hexagonal_icebergs && p.radius_based_drag) { L2 = 2. * sqrt(L * W / (2. * sqrt(3.))); W2 = L2; }
    else { L2 = L; W2 = W; }
    double groundfrac;
    if (p.h_to_init_grounding > 0.0) { groundfrac = 1.0 - (od - D) / p.h_to_init_grounding; groundfrac = dmax(groundfrac, 0.0); groundfrac = dmin(groundfrac, 1.0); }
    else groundfrac = (D > od) ? 1.0 : 0.0;
    c_gnd = (groundfrac > 0.0) ? (p.cdrag_grounding * W * L * groundfrac) / M : 0.0;
    if (p.short_step_mts_grounding) c_gnd = 0.;
    uwave = ua - uo; vwave = va - vo;
    double wmod = uwave * uwave + vwave * vwave;
    const double ampl = 0.5 * 0.02025 * wmod, Lwavelength = 0.32 * wmod, Lcutoff = 0.125 * Lwavelength, Ltop = 0.25 * Lwavelength;
    const double Cr = Cr0 * dmin(dmax(0., (L2 - Lcutoff) / ((Ltop - Lcutoff) + 1.e-30)), 1.);
    wave_rad = 0.5 * RHO_SEAWATER / M * Cr * GRAVITY * ampl * dmin(ampl, F) * (2. * W2 * L2) / (W2 + L2);
    wmod = sqrt(ua * ua + va * va);
    if (wmod != 0.) { uwave = ua / wmod; vwave = va / wmod; } else { uwave = 0.; vwave = 0.; wave_rad = 0.; }
    double dragfrac = 1.0;
    if (p.iceberg_bonds_on && p.internal_bergs_for_drag) {
      double N_bonds = 0., N_max = 4.0;
      if (p.hexagonal_icebergs) N_max = 6.0;
      const int cnt = m.bcount[k];
      for (int s = 0; s < cnt; ++s) {
        if (p.dem) { if (m.bbroken[MB_S(s, k)] != 1) N_bonds = N_bonds + 1.0; } else N_bonds = N_bonds + 1.0;
      }
      dragfrac = ((N_max - N_bonds) / N_max);
    }
    c_ocn = RHO_SEAWATER / M * p.ocean_drag_scale * (0.5 * CD_WV * dragfrac * W2 * (D_hi) + CD_WH * W * L);
    c_atm = RHO_AIR / M * (0.5 * CD_AV * dragfrac * W2 * F + CD_AH * W * L);
    if (fabs(hi) == 0.) c_ice = 0.; else c_ice = RHO_ICE / M * (0.5 * CD_IV * dragfrac * W2 * hi);
    if (fabs(ui) + fabs(vi) == 0.) c_ice = 0.;
    axn = -GRAVITY * ssh_x + wave_rad * uwave; ayn = -GRAVITY * ssh_y + wave_rad * vwave;
    if (ia_on) { interactive_force(g, p, b, m, k, mts_part, S, uvel0, vvel0, uvel0, vvel0); axn = axn + S.IA_x; ayn = ayn + S.IA_y; }
    axn = axn + f_cori * v_star; ayn = ayn - f_cori * u_star;
  } else {
    if (ia_on) interactive_force(g, p, b, m, k, mts_part, S, uvel0, vvel0, uvel0, vvel0);
  }
  double uveln = uvel0, vveln = vvel0, us, vs;
  double RHS_x = 0, RHS_y = 0, A11 = 1, A12 = 0, A21 = 0, A22 = 1;
#pragma unroll 1
  for (int itloop = 1; itloop <= 2; ++itloop) {
    if (itloop == 2) { us = uveln; vs = vveln; } else { us = uvel0; vs = vvel0; }
    if (only_interactive) {
      if (ia_on) {
        if (itloop > 1) interactive_force(g, p, b, m, k, mts_part, S, uvel0, vvel0, us, vs);
        RHS_x = (S.IA_x / 2) - scaling * (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
        RHS_y = (S.IA_y / 2) - scaling * (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
        A11 = 1 + (scaling * dt * S.P11); A22 = 1 + (scaling * dt * S.P22);
        A12 = (scaling * dt * S.P12); A21 = (scaling * dt * S.P21);
      }
    } else {
      const double drag_ocn = c_ocn * 0.5 * (sqrt((uveln - uo) * (uveln - uo) + (vveln - vo) * (vveln - vo)) + sqrt((uvel0 - uo) * (uvel0 - uo) + (vvel0 - vo) * (vvel0 - vo)));
      const double drag_atm = c_atm * 0.5 * (sqrt((uveln - ua) * (uveln - ua) + (vveln - va) * (vveln - va)) + sqrt((uvel0 - ua) * (uvel0 - ua) + (vvel0 - va) * (vvel0 - va)));
      const double drag_ice = c_ice * 0.5 * (sqrt((uveln - ui) * (uveln - ui) + (vveln - vi) * (vveln - vi)) + sqrt((uvel0 - ui) * (uvel0 - ui) + (vvel0 - vi) * (vvel0 - vi)));
      const double drag_gnd = c_gnd;
      RHS_x = (axn / 2) + scaling * (-drag_ocn * (u_star - uo) - drag_atm * (u_star - ua) - drag_ice * (u_star - ui) - drag_gnd * u_star);
      RHS_y = (ayn / 2) + scaling * (-drag_ocn * (v_star - vo) - drag_atm * (v_star - va) - drag_ice * (v_star - vi) - drag_gnd * v_star);
      if (ia_on) {
        if (itloop > 1) interactive_force(g, p, b, m, k, mts_part, S, uvel0, vvel0, us, vs);
        RHS_x = RHS_x - scaling * (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
        RHS_y = RHS_y - scaling * (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
      }
      const double lambda = drag_ocn + drag_atm + drag_ice + drag_gnd;
      A11 = 1. + scaling * dt * lambda; A22 = 1. + scaling * dt * lambda;
      A12 = -scaling * dt * f_cori; A21 = scaling * dt * f_cori;
      A12 = A12 / 2.; A21 = A21 / 2.;
      if (ia_on) {
        A11 = A11 + (scaling * dt * S.P11); A22 = A22 + (scaling * dt * S.P22);
        A12 = A12 + (scaling * dt * S.P12); A21 = A21 + (scaling * dt * S.P21);
      }
    }
    const double detA = 1. / ((A11 * A22) - (A12 * A21));
    ax = detA * (A22 * RHS_x - A12 * RHS_y); ay = detA * (A11 * RHS_y - A21 * RHS_x);
    uveln = u_star + dt * ax; vveln = v_star + dt * ay;
  }
  if (only_interactive) { axn = S.IA_x; ayn = S.IA_y; }
  else {
    axn = -GRAVITY * ssh_x + wave_rad * uwave; ayn = -GRAVITY * ssh_y + wave_rad * vwave;
    if (ia_on) { axn = axn + S.IA_x; ayn = ayn + S.IA_y; }
    axn = axn + f_cori * vveln; ayn = ayn - f_cori * uveln;
  }
  bxn = 2 * ax - axn; byn = 2 * ay - ayn;
  if (mts_part == 1) {
    Fdc_x = MF(KID_B_MASS, k) * (S.Ptu_x - (S.P11 * uveln + S.P12 * vveln));
    Fdc_y = MF(KID_B_MASS, k) * (S.Ptu_y - (S.P21 * uveln + S.P22 * vveln));
  }
  speed_limit(g, p, m, i, j, dt, uveln, vveln);
  if (p.override_iceberg_velocities) { ax = 0.; ay = 0.; axn = 0.; ayn = 0.; bxn = 0.; byn = 0.; }
}

// PART 1 sweep (IB:6672-6711); iter = ii.  The convergence norms are reduced per wave before they go to memory: a
// same-address fp64 atomic per lane serialises at the memory side (measured 1.8 ms for 5e4 bergs)
__global__ void __launch_bounds__(256) mts_part1_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                        const MtsDev *__restrict__ mt, const long long n, const int iter) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const BergPtrs &b = *bt; const MtsDev &m = *mt; const kid_params &p = *pp;
  bool act = k < n;
  if (act) act = MI(KID_BI_ALIVE, k) != 0;
  if (act) act = MF(KID_B_STATIC_BERG, k) < 0.5 && (MI(KID_BI_CONGLOM_ID, k) != 0 || p.force_convergence);
  if (act) act = (iter == 1 || MF(KID_B_STATIC_BERG, k) == 0.1);
  double s0 = 0., s1 = 0., s2 = 0.;
  bool collided = false;
  if (act) {
    const double dt = p.dt;
    double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k), u0 = uvel1, v0 = vvel1;
    double axn = 0., ayn = 0., bxn = 0., byn = 0., ax1, ay1, Fdc_x = 0., Fdc_y = 0.;
    accel_mts(g, p, b, m, k, 1, p.only_interactive_forces != 0, MI(KID_BI_INE, k), MI(KID_BI_JNE, k), MF(KID_B_LAT, k), uvel1, vvel1, u0, v0, dt,
              ax1, ay1, axn, ayn, bxn, byn, Fdc_x, Fdc_y);
    if (Fdc_x != 0. || (Fdc_y != 0. && p.force_convergence)) { collided = true; MF(KID_B_STATIC_BERG, k) = 0.1; }
    MF(KID_B_AXN, k) = axn; MF(KID_B_AYN, k) = ayn; MF(KID_B_BXN, k) = bxn; MF(KID_B_BYN, k) = byn;
    const double u = MF(KID_B_UVEL, k), v = MF(KID_B_VVEL, k);
    if (p.force_convergence) {
      const double up = u + (dt * ax1), vp = v + (dt * ay1);
      MF(KID_B_UVEL_PREV, k) = up; MF(KID_B_VVEL_PREV, k) = vp;
      const double uo_ = MF(KID_B_UVEL_OLD, k), vo_ = MF(KID_B_VVEL_OLD, k);
      if (iter == 1) s0 = uo_ * uo_ + vo_ * vo_;
      s1 = up * up + vp * vp;
      s2 = (up - uo_) * (up - uo_) + (vp - vo_) * (vp - vo_);
    } else {
      const double un = u + (dt * ax1), vn = v + (dt * ay1);
      MF(KID_B_UVEL, k) = un; MF(KID_B_VVEL, k) = vn; MF(KID_B_UVEL_PREV, k) = un; MF(KID_B_VVEL_PREV, k) = vn;
    }
  }
  if (p.force_convergence) {
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    const bool any_col = __ballot(collided) != 0ull;
    if (__lane_id() == 0) {
      if (iter == 1 && s0 != 0.) unsafeAtomicAdd(m.red + MR_USUM, s0);
      if (s1 != 0.) unsafeAtomicAdd(m.red + MR_USUM1, s1);
      if (s2 != 0.) unsafeAtomicAdd(m.red + MR_USUM2, s2);
      if (any_col) m.red[MR_COLLISION] = 1.;
    }
  } else if (collided) m.red[MR_COLLISION] = 1.;
}
// IB:6714-6725
__global__ void __launch_bounds__(256) mts_part1_old_kernel(const BergPtrs *__restrict__ bt, const long long n, const int last_iter) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt;
  if (MI(KID_BI_ALIVE, k) == 0 || !(MF(KID_B_STATIC_BERG, k) < 0.5)) return;
  MF(KID_B_UVEL_OLD, k) = MF(KID_B_UVEL_PREV, k); MF(KID_B_VVEL_OLD, k) = MF(KID_B_VVEL_PREV, k);
  if (last_iter && MF(KID_B_STATIC_BERG, k) == 0.1) MF(KID_B_STATIC_BERG, k) = 0.;
}
// PART 2 (IB:6752-6772)
__global__ void __launch_bounds__(256) mts_part2_kernel(const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp;
  if (!mts_active(b, k)) return;
  const double dt_2 = 0.5 * p.dt;
  double u = MF(KID_B_UVEL_PREV, k), v = MF(KID_B_VVEL_PREV, k);
  u = u + dt_2 * (MF(KID_B_AXN, k) + MF(KID_B_BXN, k));
  v = v + dt_2 * (MF(KID_B_AYN, k) + MF(KID_B_BYN, k));
  MF(KID_B_UVEL, k) = u; MF(KID_B_VVEL, k) = v; MF(KID_B_UVEL_OLD, k) = u; MF(KID_B_VVEL_OLD, k) = v;
  if (p.force_convergence) {
    MF(KID_B_AXN, k) = MF(KID_B_AXN_FAST, k); MF(KID_B_AYN, k) = MF(KID_B_AYN_FAST, k);
    MF(KID_B_BXN, k) = MF(KID_B_BXN_FAST, k); MF(KID_B_BYN, k) = MF(KID_B_BYN_FAST, k);
  }
}

__device__ __forceinline__ double groundfrac_of(const kid_params &p, double od, double thickness) {
  const double D = (p.rho_bergs / RHO_SEAWATER) * thickness;
  double gf;
  if (p.h_to_init_grounding > 0.0) { gf = 1.0 - (od - D) / p.h_to_init_grounding; gf = dmax(gf, 0.0); gf = dmin(gf, 1.0); }
  else gf = (D > od) ? 1.0 : 0.0;
  return gf;
}

// Pieces of a sub-step shared by the per-launch kernels and the fused loop (mts_substeps_kernel)
struct LonLat { double lon, lat; };
struct UV { double u, v; };
struct Element { double M, R, A; };   // mass, radius, area: under constant_interaction_LW those of the constant element
__device__ __forceinline__ Element element_of(const kid_params &p, const BergPtrs &b, long long k) {
  if (p.constant_interaction_LW) {
    const double A = p.constant_length * p.constant_width;
    return Element{A * MF(KID_B_THICKNESS, k) * p.rho_bergs, radius_of(p, A), A};
  }
  const double A = MF(KID_B_LENGTH, k) * MF(KID_B_WIDTH, k);
  return Element{MF(KID_B_MASS, k), radius_of(p, A), A};
}
// update_verlet_position (IB:6786-6822, IB:7684-7764): the position after dt with the velocity u + dt/2 (axn + bxn),
// on the tangent plane near the pole
__device__ __forceinline__ LonLat verlet_position(const DevGrid &g, const kid_params &p, double lon1, double lat1, double uvel1, double vvel1,
                                                  double axn, double ayn, double bxn, double byn, double dt) {
  const double dt_2 = 0.5 * dt;
  const double uvel2 = uvel1 + (dt_2 * axn) + (dt_2 * bxn), vvel2 = vvel1 + (dt_2 * ayn) + (dt_2 * byn);
  double lonn, latn;
  if ((lat1 > 89.) && g.latlon) {
    double x1, y1, xdot2, ydot2;
    rotpos_to_tang(p, lon1, lat1, x1, y1);
    rotvec_to_tang(p, lon1, uvel2, vvel2, xdot2, ydot2);
    rotpos_from_tang(p, x1 + (dt * xdot2), y1 + (dt * ydot2), lonn, latn);
  } else {
    double dxdl1, dydl;
    if (g.latlon) { dxdl1 = (180. / p.pi) / (p.Rearth * cos((lat1) * (p.pi / 180.))); dydl = (180. / p.pi) / p.Rearth; } else { dxdl1 = 1.; dydl = 1.; }
    const double u2 = uvel2 * dxdl1, v2 = vvel2 * dydl;
    lonn = lon1 + (dt * u2); latn = lat1 + (dt * v2);
  }
  return LonLat{lonn, latn};
}
// the *_old velocities MTS leaves after the position update (IB:6826-6827); the v component takes bxn, not byn (sic, IB:6831)
__device__ __forceinline__ UV mts_old_velocity(double uvel, double vvel, double axn, double ayn, double bxn, double dt_2) {
  return UV{uvel + dt_2 * (axn + bxn), vvel + dt_2 * (ayn + bxn)};
}
// the new velocity uvel3 + dt ax1 (IB:6906-6918, IB:7272-7281), on the tangent plane near the pole
__device__ __forceinline__ UV verlet_velocity(const DevGrid &g, const kid_params &p, double lonn, double latn, double uvel3, double vvel3,
                                              double ax1, double ay1, double dt) {
  double uveln, vveln;
  if ((latn > 89.) && g.latlon) {
    double xdot3, ydot3, xddot1, yddot1;
    rotvec_to_tang(p, lonn, uvel3, vvel3, xdot3, ydot3);
    rotvec_to_tang(p, lonn, ax1, ay1, xddot1, yddot1);
    rotvec_from_tang(p, lonn, xdot3 + (dt * xddot1), ydot3 + (dt * yddot1), uveln, vveln);
  } else { uveln = uvel3 + (dt * ax1); vveln = vvel3 + (dt * ay1); }
  return UV{uveln, vveln};
}
// accel_explicit_inner_mts after its sums (IB:1861-1947).  With DEM bonds: the bond sums F, Fd, T, T_d as accelerations
// (rM = 1/M, rI = 1/I, I = M R^2 / 2) added to IA, IAd; start_lon matters to the beam tests only.
struct DemAccel { double IA_x, IA_y, IAd_x, IAd_y, ang_accel; };
__device__ __forceinline__ DemAccel dem_bond_accel(const kid_params &p, double IA_x, double IA_y, double IAd_x, double IAd_y, double F_x, double F_y,
                                                   double Fd_x, double Fd_y, double Tq, double T_d, double start_lon, Rcp rM, Rcp rI) {
  if (p.dem_beam_test > 0) dem_beam_test_load(p, start_lon, F_y, Fd_y);
  IA_x = IA_x + F_x * rM; IA_y = IA_y + F_y * rM;
  IAd_x = IAd_x + Fd_x * rM; IAd_y = IAd_y + Fd_y * rM;
  return DemAccel{IA_x, IA_y, IAd_x, IAd_y, (Tq + T_d) * rI};
}
// Then the accelerations from the sums (loc_dx: speed_limit_dx of the berg's cell, or -1 to look it up)
struct InnerAccel { double axn, ayn, ax1, ay1; };
__device__ __forceinline__ InnerAccel explicit_inner_accel(const DevGrid &g, const kid_params &p, const MtsDev &m, double IA_x, double IA_y,
                                                           double IAd_x, double IAd_y, double gdrag, double u, double v, double u_star, double v_star,
                                                           int i, int j, double dt, double loc_dx) {
  double axn = IA_x + IAd_x, ayn = IA_y + IAd_y;
  double ax1 = 0.5 * (axn + 0.), ay1 = 0.5 * (ayn + 0.);
  double ul = u_star + dt * ax1, vl = v_star + dt * ay1;
  speed_limit(g, p, m, i, j, dt, ul, vl, loc_dx);
  if (p.override_iceberg_velocities) { ax1 = 0.; ay1 = 0.; axn = 0.; ayn = 0.; }
  if (p.short_step_mts_grounding) {
    axn = axn + u * gdrag; ayn = ayn + v * gdrag;
    ax1 = 0.5 * axn; ay1 = 0.5 * ayn;
  }
  return InnerAccel{axn, ayn, ax1, ay1};
}

// PART 3 per sub-step.  POST: the tail of the previous sub-step (IB:6972-7044) fused in front of the position update
// of this one (IB:6786-6833): both touch only the berg's own row.
template <bool POST, bool POS>
__global__ void __launch_bounds__(256) mts_substep_own_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                              const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (!mts_active(b, k)) return;
  const double dt = m.mts_fast_dt, dt_2 = 0.5 * dt;
  if (POST) {
    MF(KID_B_UVEL_OLD, k) = MF(KID_B_UVEL, k); MF(KID_B_VVEL_OLD, k) = MF(KID_B_VVEL, k);
    double gdrag = 0.;
    if (p.use_grounding_torque) {
      const double gf = groundfrac_of(p, MF(KID_B_OD, k), MF(KID_B_THICKNESS, k));
      if (gf > 0.0) {
        const Element e = element_of(p, b, k);
        gdrag = -p.cdrag_grounding * gf * p.pi * kid_pow(e.R, 2.) / e.M;
      }
    }
    if (p.dem) {
      double w = MF(KID_B_ANG_VEL, k) + dt * MF(KID_B_ANG_ACCEL, k);
      w = w * kid_rcp(1. - gdrag * dt);
      MF(KID_B_ANG_VEL, k) = w;
      MF(KID_B_ROT, k) = MF(KID_B_ROT, k) + dt * w;
    }
    if (p.force_convergence) {
      MF(KID_B_AXN, k) = MF(KID_B_AXN_FAST, k); MF(KID_B_AYN, k) = MF(KID_B_AYN_FAST, k);
      MF(KID_B_BXN, k) = MF(KID_B_BXN_FAST, k); MF(KID_B_BYN, k) = MF(KID_B_BYN_FAST, k);
    }
  }
  if (POS) {
    const double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k);
    const double axn = MF(KID_B_AXN_FAST, k), ayn = MF(KID_B_AYN_FAST, k), bxn = MF(KID_B_BXN_FAST, k), byn = MF(KID_B_BYN_FAST, k);
    const UV old = mts_old_velocity(uvel1, vvel1, axn, ayn, bxn, dt_2);
    MF(KID_B_UVEL_OLD, k) = old.u; MF(KID_B_VVEL_OLD, k) = old.v;
    const LonLat q = verlet_position(g, p, MF(KID_B_LON, k), MF(KID_B_LAT, k), uvel1, vvel1, axn, ayn, bxn, byn, dt);
    MF(KID_B_LON, k) = q.lon; MF(KID_B_LAT, k) = q.lat; MF(KID_B_LON_OLD, k) = q.lon; MF(KID_B_LAT_OLD, k) = q.lat;
  }
}

// velocity sweep of a sub-step (IB:6848-6946), one lane per berg; reads neighbours' *_old state and the bond records
// left by bond_pass_kernel, writes only its own row
__global__ void __launch_bounds__(256) mts_velocity_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                           const MtsDev *__restrict__ mt, const long long n, const int jj) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (!mts_active(b, k)) return;
  const double dt = m.mts_fast_dt, dt_2 = 0.5 * dt;
  const double latn = MF(KID_B_LAT, k), lonn = MF(KID_B_LON, k);
  double axn = MF(KID_B_AXN_FAST, k), ayn = MF(KID_B_AYN_FAST, k), bxn = MF(KID_B_BXN_FAST, k), byn = MF(KID_B_BYN_FAST, k);
  double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k);
  const int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k);
  axn = axn + bxn; ayn = ayn + byn;
  const double uvel3 = uvel1 + (dt_2 * axn), vvel3 = vvel1 + (dt_2 * ayn);
  double ax1, ay1;
  if (p.explicit_inner_mts) {  // accel_explicit_inner_mts IB:1710-1947
    const double u_star = uvel1 + (axn * (dt / 2.)), v_star = vvel1 + (ayn * (dt / 2.));
    double IA_x = 0., IA_y = 0., IAd_x = 0., IAd_y = 0., F_x = 0., F_y = 0., Tq = 0., Fd_x = 0., Fd_y = 0., T_d = 0.;
    if (p.iceberg_bonds_on) {
      const int cnt = m.bcount[k];
      if (p.dem) {
        // all slots' records are fetched up front (slots past the list's end are allocated, just unused), so the ~50
        // loads of a berg are in flight together instead of one dependent chain per slot
        int o_[KID_MAX_BONDS], br_[KID_MAX_BONDS];
        double fx_[KID_MAX_BONDS], fy_[KID_MAX_BONDS], fdx_[KID_MAX_BONDS], fdy_[KID_MAX_BONDS], t_[KID_MAX_BONDS], td_[KID_MAX_BONDS];
#pragma unroll
        for (int s = 0; s < KID_MAX_BONDS; ++s) {
          const int sc = s < m.mb ? s : 0;
          o_[s] = m.bother_row[MB_S(sc, k)]; br_[s] = m.bbroken[MB_S(sc, k)];
          fx_[s] = MBD(KID_BOND_F_X, sc, k); fy_[s] = MBD(KID_BOND_F_Y, sc, k); fdx_[s] = MBD(KID_BOND_FD_X, sc, k); fdy_[s] = MBD(KID_BOND_FD_Y, sc, k);
          t_[s] = MBD(KID_BOND_T, sc, k); td_[s] = MBD(KID_BOND_T_D, sc, k);
        }
#pragma unroll
        for (int s = 0; s < KID_MAX_BONDS; ++s) {
          if (s >= cnt) continue;
          const int o = o_[s];
          if (o < 0) { unsafeAtomicAdd(m.red + MR_NERR, 1.); continue; }
          if (br_[s] == 1) unbonded_dem_force(g, p, b, m, dem_rec_main(b, k), dem_rec_main(b, o), k, o, IA_x, IA_y, IAd_x, IAd_y, uvel1, vvel1, uvel1, vvel1);
          else {
            F_x = F_x + fx_[s]; F_y = F_y + fy_[s]; Fd_x = Fd_x + fdx_[s]; Fd_y = Fd_y + fdy_[s];
            Tq = Tq + t_[s]; T_d = T_d + td_[s];
            if (br_[s] == 3) m.bbroken[MB_S(s, k)] = 1;  // fractured on this sweep: from the next one on it is a contact
          }
        }
      }
      for (int s = 0; s < (p.dem ? 0 : cnt); ++s) {
        const int o = m.bother_row[MB_S(s, k)];
        if (o < 0) { unsafeAtomicAdd(m.red + MR_NERR, 1.); continue; }
        {
          IaSum S{0., 0., 0., 0., 0., 0., 0., 0.};
          calculate_force(g, p, b, k, o, S, uvel1, vvel1, uvel1, vvel1, true, -1);
          IA_x += S.IA_x; IA_y += S.IA_y;
          const double du = MF(KID_B_UVEL_OLD, o) - MF(KID_B_UVEL_OLD, k), dv = MF(KID_B_VVEL_OLD, o) - MF(KID_B_VVEL_OLD, k);
          IAd_x = IAd_x + S.P11 * du + S.P12 * dv;
          IAd_y = IAd_y + S.P12 * du + S.P22 * dv;
        }
      }
      bool run_contact;
      if (p.iceberg_bonds_on && p.dem) run_contact = !((MI(KID_BI_N_BONDS, k) == p.max_bonds) || p.use_broken_bonds_for_substep_contact);
      else run_contact = true;
      if (run_contact && p.dem) {
        // The same search with the DEM contact law.  As written in the reference it is, per candidate, a chain of dependent
        // loads (the row, its conglomerate and bond count, then the records inside the force routine): ~100 us per sweep
        // for an element with 80 candidates around it.  Here what the berg itself contributes is read once, candidates go
        // four at a time with their loads issued together, and a candidate that is certainly out of reach -- the routine
        // would return without touching the sums -- never reaches it (dem_out_of_reach; the routine decides the close calls).
        const int j0 = max(j - 1, g.jsd + 1), j1 = min(j + 1, g.jed), i0 = max(i - 1, g.isd + 1), i1 = min(i + 1, g.ied);
        const int conglom_k = MI(KID_BI_CONGLOM_ID, k);
        const DemRec Kr = dem_rec_main(b, k);
        const double A1 = p.constant_interaction_LW ? 0. : MF(KID_B_LENGTH, k) * MF(KID_B_WIDTH, k);
        const int pcnt = (p.use_broken_bonds_for_substep_contact || m.mb == 0) ? 0 : m.bcount[k];   // bond partners are marked, IB:1796
        int prow[KID_MAX_BONDS];
#pragma unroll
        for (int s = 0; s < KID_MAX_BONDS; ++s) prow[s] = (s < pcnt) ? m.bother_row[MB_S(s, k)] : -1;
        for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi) {
          const int c = g.idx(gi, gj);
          const int q0 = m.cell_start[c], q1 = m.cell_start[c + 1];
          for (int qb = q0; qb < q1; qb += 4) {
            int o_[4], cg_[4], nb_[4]; double lo_[4], la_[4], A2_[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) o_[t] = m.order[(qb + t < q1) ? qb + t : q0];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              cg_[t] = MI(KID_BI_CONGLOM_ID, o_[t]); nb_[t] = MI(KID_BI_N_BONDS, o_[t]);
              lo_[t] = MF(KID_B_LON_OLD, o_[t]); la_[t] = MF(KID_B_LAT_OLD, o_[t]);
              A2_[t] = p.constant_interaction_LW ? 0. : MF(KID_B_LENGTH, o_[t]) * MF(KID_B_WIDTH, o_[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (qb + t >= q1) continue;
              bool marked = false;
#pragma unroll
              for (int s = 0; s < KID_MAX_BONDS; ++s) marked = marked || (prow[s] == o_[t]);
              if (marked || cg_[t] != conglom_k || nb_[t] >= p.max_bonds) continue;
              if (dem_out_of_reach(g, p, m, Kr.lon, Kr.lat, lo_[t], la_[t], A1, A2_[t])) continue;
              unbonded_dem_force(g, p, b, m, Kr, dem_rec_main(b, o_[t]), k, o_[t], IA_x, IA_y, IAd_x, IAd_y, uvel1, vvel1, uvel1, vvel1);
            }
          }
        }
      } else if (run_contact) {
        const int j0 = max(j - 1, g.jsd + 1), j1 = min(j + 1, g.jed), i0 = max(i - 1, g.isd + 1), i1 = min(i + 1, g.ied);
        for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi) {
          const int c = g.idx(gi, gj);
          for (int q = m.cell_start[c]; q < m.cell_start[c + 1]; ++q) {
            const int o = m.order[q];
            const bool unmarked = p.use_broken_bonds_for_substep_contact ? true : !is_partner(m, k, o);
            if (unmarked && MI(KID_BI_CONGLOM_ID, o) == MI(KID_BI_CONGLOM_ID, k) && MI(KID_BI_N_BONDS, o) < p.max_bonds) {
              {
                IaSum S{0., 0., 0., 0., 0., 0., 0., 0.};
                calculate_force(g, p, b, k, o, S, uvel1, vvel1, uvel1, vvel1, false, 1);
                IA_x += S.IA_x; IA_y += S.IA_y;
                const double du = MF(KID_B_UVEL_OLD, o) - MF(KID_B_UVEL_OLD, k), dv = MF(KID_B_VVEL_OLD, o) - MF(KID_B_VVEL_OLD, k);
                IAd_x = IAd_x + S.P11 * du + S.P12 * dv;
                IAd_y = IAd_y + S.P12 * du + S.P22 * dv;
              }
            }
          }
        }
      }
    }
    if (p.dem) {
      const Element e = element_of(p, b, k);
      const DemAccel d = dem_bond_accel(p, IA_x, IA_y, IAd_x, IAd_y, F_x, F_y, Fd_x, Fd_y, Tq, T_d, p.dem_beam_test > 0 ? MF(KID_B_START_LON, k) : 0.,
                                        kid_rcp(e.M), kid_rcp(0.5 * e.M * kid_pow(e.R, 2.)));
      IA_x = d.IA_x; IA_y = d.IA_y; IAd_x = d.IAd_x; IAd_y = d.IAd_y;
      MF(KID_B_ANG_ACCEL, k) = d.ang_accel;
    }
    double gdrag = 0.;
    if (p.short_step_mts_grounding) {
      const double gf = groundfrac_of(p, MF(KID_B_OD, k), MF(KID_B_THICKNESS, k));
      if (gf > 0.0) {
        const Element e = element_of(p, b, k);
        gdrag = -p.cdrag_grounding * gf * e.A / e.M;
      }
    }
    const InnerAccel a = explicit_inner_accel(g, p, m, IA_x, IA_y, IAd_x, IAd_y, gdrag, uvel1, vvel1, u_star, v_star, i, j, dt, -1.);
    axn = a.axn; ayn = a.ayn; ax1 = a.ax1; ay1 = a.ay1;
    bxn = 0.; byn = 0.;
  } else {
    double u0 = uvel1, v0 = vvel1, fx = 0., fy = 0.;
    accel_mts(g, p, b, m, k, 3, true, i, j, latn, uvel1, vvel1, u0, v0, dt, ax1, ay1, axn, ayn, bxn, byn, fx, fy);
  }
  const UV vn = verlet_velocity(g, p, lonn, latn, uvel3, vvel3, ax1, ay1, dt);
  if (p.force_convergence && !p.explicit_inner_mts) {  // rare configuration: one atomic per lane is acceptable here
    const double uo_ = MF(KID_B_UVEL_OLD, k), vo_ = MF(KID_B_VVEL_OLD, k);
    if (jj == 1) unsafeAtomicAdd(m.red + MR_USUM, uo_ * uo_ + vo_ * vo_);
    unsafeAtomicAdd(m.red + MR_USUM1, vn.u * vn.u + vn.v * vn.v);
    unsafeAtomicAdd(m.red + MR_USUM2, (vn.u - uo_) * (vn.u - uo_) + (vn.v - vo_) * (vn.v - vo_));
  }
  MF(KID_B_AXN_FAST, k) = axn; MF(KID_B_AYN_FAST, k) = ayn; MF(KID_B_BXN_FAST, k) = bxn; MF(KID_B_BYN_FAST, k) = byn;
  // a neighbour may still be reading uvel_old/vvel_old of this berg, never uvel/vvel: safe to write in place
  MF(KID_B_UVEL, k) = vn.u; MF(KID_B_VVEL, k) = vn.v;
}
// ---------------------------------------------------------------------------------------------------------------------
// The whole sub-step loop of PART 3 (IB:6788-7050) in ONE launch, for the configuration the DEM tests run (explicit inner steps,
// DEM bonds, broken bonds as the only sub-step contacts).  As three launches per sub-step the loop is bound by the latency of
// ~50 k-lane kernels (bond pass 14 us + velocity sweep 14 us + own-row update 6 us at 224x224 elements, profiles/r01_config4_*);
// here the 90 sub-steps of a step run inside one launch:
//   * One lane per berg, at most one wave per SIMD (the grid is ceil(n/256) workgroups of 256): everything a berg carries from
//     one sub-step to the next -- its row of the state, its copies of its bonds' state, what does not change about its pairs
//     (masses, radii, damping: pair_const) -- stays in registers for the whole loop; nothing of the berg's own is re-read.
//   * Each berg evaluates ALL of its bonds, in its bond-list order, in the orientation of the pair's primary side (the side
//     the reference's sweep reaches first, rank[]), so both sides get bit-identical forces (the partner's copies are the
//     negatives, IB:1190-1204): a pair is computed twice but no lane writes another berg's records, and the sums over the
//     bond list (IB:1793-1811) need nothing from anybody else.
//   * What bergs read of each other is six doubles (DemRec), kept as one 64-byte record per berg in three copies
//     (MtsDev::rec).  The records are read and written with device-coherent 16-byte accesses (sc1: the per-XCD L2s are not
//     coherent with each other, and an agent-scope release + acquire -- L2 write-back + invalidate -- per sub-step cost
//     ~60 us each when tried), all of a berg's neighbours in one round trip.
//   * There is no grid barrier: a record carries its own "written" state (every word of a record that is not there yet holds
//     MTS_REC_EMPTY) and a berg waits for its own neighbours only -- store -> load, ~0.7 us (tools/profiling/p2p_probe.hip),
//     where a barrier is store -> arrival counter(s) -> poll -> load (tools/profiling/barrier_probe.hip: 2.5 us at 196
//     workgroups for a two-level counter, 4.1 us for a flat one, before the loads).  Sub-step j reads the neighbours'
//     records of j-1 in copy (j-1)%3, THEN marks its own record in copy (j+1)%3 (sub-step j-2's: the records just read
//     prove every neighbour is done with it) as empty, and writes its record of j into copy j%3 after the mark has reached
//     memory.  The polls are bounded: bergs whose neighbours never write (a grid that is not co-resident) give up with an
//     error instead of hanging the device; the launch is cooperative so that the runtime checks co-residency.
// ---------------------------------------------------------------------------------------------------------------------
// device-coherent accesses to the 64-byte records (global_load/store_dwordx4 sc1 = what a relaxed agent-scope atomic access
// compiles to on gfx950, 16 bytes at a time): four records in one round trip / one record out
typedef double kid_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void rec_load4(const double *p0, const double *p1, const double *p2, const double *p3, DemRec (&r)[4]) {
  kid_d2 a0, a1, a2, b0, b1, b2, c0, c1, c2, d0, d1, d2;
  asm volatile("global_load_dwordx4 %0, %12, off sc1\n\tglobal_load_dwordx4 %1, %12, off offset:16 sc1\n\tglobal_load_dwordx4 %2, %12, off offset:32 sc1\n\t"
               "global_load_dwordx4 %3, %13, off sc1\n\tglobal_load_dwordx4 %4, %13, off offset:16 sc1\n\tglobal_load_dwordx4 %5, %13, off offset:32 sc1\n\t"
               "global_load_dwordx4 %6, %14, off sc1\n\tglobal_load_dwordx4 %7, %14, off offset:16 sc1\n\tglobal_load_dwordx4 %8, %14, off offset:32 sc1\n\t"
               "global_load_dwordx4 %9, %15, off sc1\n\tglobal_load_dwordx4 %10, %15, off offset:16 sc1\n\tglobal_load_dwordx4 %11, %15, off offset:32 sc1\n\t"
               "s_waitcnt vmcnt(0)"
               : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(d0), "=&v"(d1), "=&v"(d2)
               : "v"(p0), "v"(p1), "v"(p2), "v"(p3) : "memory");
  r[0] = DemRec{a0.x, a0.y, a1.x, a1.y, a2.x, a2.y}; r[1] = DemRec{b0.x, b0.y, b1.x, b1.y, b2.x, b2.y};
  r[2] = DemRec{c0.x, c0.y, c1.x, c1.y, c2.x, c2.y}; r[3] = DemRec{d0.x, d0.y, d1.x, d1.y, d2.x, d2.y};
}
// "not yet written": a NaN no computation produces, the same in both halves (the host fills the copies with hipMemsetD32Async)
#define MTS_REC_EMPTY_BITS 0xfff7c0defff7c0deull
#define MTS_REC_EMPTY_D __longlong_as_double((long long)MTS_REC_EMPTY_BITS)
enum { MTS_POLL_LIMIT = 400000 };
#ifndef MTS_POLL_SLEEP
#define MTS_PRE_POLL_SLEEP 32   // before the first poll of a sub-step (64-cycle units)
#define MTS_POLL_SLEEP 8   // between polls: with 2 the polling itself held the stores up (2.29 ms per config-4 step against 1.51)
#endif
__device__ __forceinline__ bool rec_written(const DemRec &r) {
  const unsigned long long e = MTS_REC_EMPTY_BITS;
  return (unsigned long long)__double_as_longlong(r.lon) != e && (unsigned long long)__double_as_longlong(r.lat) != e && (unsigned long long)__double_as_longlong(r.u) != e &&
         (unsigned long long)__double_as_longlong(r.v) != e && (unsigned long long)__double_as_longlong(r.w) != e && (unsigned long long)__double_as_longlong(r.rot) != e;
}
__device__ __forceinline__ void rec_store(double *q, const DemRec &r) {
  const kid_d2 a{r.lon, r.lat}, bq{r.u, r.v}, c{r.w, r.rot};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\tglobal_store_dwordx4 %0, %2, off offset:16 sc1\n\tglobal_store_dwordx4 %0, %3, off offset:32 sc1"
               :: "v"(q), "v"(a), "v"(bq), "v"(c) : "memory");
}

#ifndef MTS_FUSED_BS
#define MTS_FUSED_BS 256   // workgroup size of mts_substeps_kernel
#endif
template <int MB>   // MB: bond slots a lane carries (4 or 8, >= MtsDev::mb)
__global__ void __launch_bounds__(MTS_FUSED_BS) mts_substeps_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                           const MtsDev *__restrict__ mt, const long long n, const int nsub, const int poll_limit, int *timeouts) {
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  const double dt = m.mts_fast_dt, dt_2 = 0.5 * dt;
  const long long k = (long long)blockIdx.x * (long long)MTS_FUSED_BS + threadIdx.x;
  bool gave_up = false;
  const bool in = k < n;
  const long long kk = in ? k : 0;
  const bool act_k = in && mts_active(b, kk);
  const int cnt = in ? m.bcount[kk] : 0;
  // ---- what does not change over the sub-steps: the bond list, who is swept, which side a pair is evaluated from ----
  int o[MB], br[MB]; bool pair[MB], prim[MB], sweep[MB]; double t1[MB], t2[MB], rr[MB]; PairConst pc[MB];
#pragma unroll
  for (int s = 0; s < MB; ++s) {
    const bool has = s < m.mb && s < cnt;
    o[s] = has ? m.bother_row[MB_S(s, kk)] : -2;                       // -2: past the end of the list, -1: partner not found
    br[s] = has ? m.bbroken[MB_S(s, kk)] : 0;
    pair[s] = o[s] >= 0;
    const long long os = pair[s] ? o[s] : kk;
    const bool act_o = pair[s] && mts_active(b, os);
    prim[s] = act_k && !(act_o && m.rank[os] < m.rank[kk]);
    sweep[s] = pair[s] && (act_k || act_o);
    t1[s] = 0.; t2[s] = 0.; rr[s] = 0.;
    if (pair[s]) { t1[s] = MBD(KID_BOND_TANGD1, s, kk); t2[s] = MBD(KID_BOND_TANGD2, s, kk); rr[s] = MBD(KID_BOND_REL_ROTATION, s, kk); }
    pc[s] = prim[s] ? pair_const(p, b, m, kk, os) : pair_const(p, b, m, os, kk);
  }
  // ---- the berg's own row ----
  DemRec own = dem_rec_main(b, kk);
  double lon = 0., lat = 0., uvel = 0., vvel = 0., axf = 0., ayf = 0., bxf = 0., byf = 0., M = 1., I_rot = 1., gdrag = 0., gdrag_t = 0., ang_accel = 0.;
  int ci_ = 0, cj_ = 0; double loc_dx = 0., start_lon = 0.;
  if (act_k) {
    lon = MF(KID_B_LON, kk); lat = MF(KID_B_LAT, kk); uvel = MF(KID_B_UVEL, kk); vvel = MF(KID_B_VVEL, kk);
    axf = MF(KID_B_AXN_FAST, kk); ayf = MF(KID_B_AYN_FAST, kk); bxf = MF(KID_B_BXN_FAST, kk); byf = MF(KID_B_BYN_FAST, kk);
    ci_ = MI(KID_BI_INE, kk); cj_ = MI(KID_BI_JNE, kk);
    if (p.dem_beam_test > 0) start_lon = MF(KID_B_START_LON, kk);
    if ((p.speed_limit > 0.) || (p.speed_limit == -1.)) loc_dx = speed_limit_dx(g, ci_, cj_);
    const Element e = element_of(p, b, kk);
    M = e.M;
    I_rot = 0.5 * M * kid_pow(e.R, 2.);
    if (p.short_step_mts_grounding || p.use_grounding_torque) {
      const double gf = groundfrac_of(p, MF(KID_B_OD, kk), MF(KID_B_THICKNESS, kk));
      if (gf > 0.0) {
        if (p.short_step_mts_grounding) gdrag = -p.cdrag_grounding * gf * e.A / M;
        if (p.use_grounding_torque) gdrag_t = -p.cdrag_grounding * gf * p.pi * kid_pow(e.R, 2.) / M;
      }
    }
  }
  const Rcp rM = kid_rcp(M), rI = kid_rcp(I_rot), rw = kid_rcp(1. - gdrag_t * dt);
  // Three copies of the records: sub-step j reads the neighbours' records of sub-step j-1 in copy (j-1)%3, writes its own
  // into copy j%3 and marks its record in copy (j+1)%3 -- sub-step j-2's, which every neighbour has finished with: their
  // records of sub-step j-1 are here -- as not yet written (MTS_REC_EMPTY in every word).  A reader polls until none of the
  // six words of a record is the mark: that is all the synchronisation there is between bergs (no grid barrier: a berg
  // waits for its own neighbours only, store -> load, instead of store -> two counters -> poll -> load).
  double *const rec[3] = {m.rec, m.rec + 8 * (size_t)n, m.rec + 16 * (size_t)n};
  const DemRec empty{MTS_REC_EMPTY_D, MTS_REC_EMPTY_D, MTS_REC_EMPTY_D, MTS_REC_EMPTY_D, MTS_REC_EMPTY_D, MTS_REC_EMPTY_D};
  if (in) rec_store(rec[0] + 8 * kk, own);   // (the host has marked all three copies)
  KID_TICK_ANY(-1);
  for (int sub = 1; sub <= nsub; ++sub) {
    const double *cur = rec[(sub - 1) % 3]; double *nxt = rec[sub % 3];
    // ---- the neighbours' records, one round trip when they are there (a slot without a partner reads the berg's own: any valid address) ----
    DemRec nb[MB];
    // a record takes ~0.7 us from its store to being visible and a poll ~1 us to come back: a first poll sent right away
    // finds nothing and costs a second one (config 4: 1.37 -> 1.32 ms/step with the pause, flat between 32 and 64 units)
    __builtin_amdgcn_s_sleep(MTS_PRE_POLL_SLEEP);
    for (int spins = 0;; ++spins) {
#pragma unroll
      for (int s0 = 0; s0 < MB; s0 += 4) {
        DemRec q[4];
        rec_load4(cur + 8 * (pair[s0] ? (long long)o[s0] : kk), cur + 8 * (pair[s0 + 1] ? (long long)o[s0 + 1] : kk),
                  cur + 8 * (pair[s0 + 2] ? (long long)o[s0 + 2] : kk), cur + 8 * (pair[s0 + 3] ? (long long)o[s0 + 3] : kk), q);
        nb[s0] = q[0]; nb[s0 + 1] = q[1]; nb[s0 + 2] = q[2]; nb[s0 + 3] = q[3];
      }
      bool ready = true;
#pragma unroll
      for (int s = 0; s < MB; ++s) if (pair[s]) ready = ready && rec_written(nb[s]);
      if (__builtin_amdgcn_ballot_w64(!ready) == 0ull) break;
      if (spins > poll_limit) {   // a neighbour that never wrote (a grid that is not co-resident, a lane that gave up): an error, not a hang
        // The wave stops here, but not in mid-air: it leaves the loop and writes back the state of the last sub-step it did
        // complete (every field of a row from the same sub-step), counts itself in `timeouts` -- which the host reads at its
        // next synchronisation and turns into KID_EHIP: the step is incomplete -- and its neighbours time out in turn.
        if (!ready) { unsafeAtomicAdd(m.red + MR_NERR, 1.); atomicAdd(timeouts, 1); }
        gave_up = true;
        break;
      }
      __builtin_amdgcn_s_sleep(MTS_POLL_SLEEP);
    }
    if (gave_up) break;
    KID_TICK_ANY(0);
    if (in) rec_store(rec[(sub + 1) % 3] + 8 * kk, empty);   // sub-step j-2's record: the neighbours' records of j-1 just read say they are done with it
    const bool last = sub == nsub;
    // ---- bond pass (IB:1757-1795 via calculate_force_dem) + the berg's sums over its list, in list order (IB:1804-1809) ----
    double F_x = 0., F_y = 0., Fd_x = 0., Fd_y = 0., Tq = 0., T_d = 0.;
    int fresh = 0;   // slots that fractured on this sweep: their forces still count, contacts from the next sub-step on
    // all of the berg's pairs piece by piece (a slot that is not evaluated this sweep is computed on its own record and ignored)
    PairOut rs[MB];
    {
      PairMid mid[MB]; double th[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        const double sg = prim[s] ? 1. : -1.;
        mid[s] = pair_geom(g, p, m, pc[s], prim[s] ? own : nb[s], prim[s] ? nb[s] : own, sg * t1[s], sg * t2[s], sg * rr[s], dt);
      }
      // the sines of the relative rotations: small angles (bonds break long before a radian) by their series, straight-line
      // code the scheduler can interleave with the rest; anything else through sin() (-DKID_EXACT_MATH: always)
      bool small = !p.orig_dem_moment_of_inertia;
#ifdef KID_EXACT_MATH
      small = false;
#endif
#pragma unroll
      for (int s = 0; s < MB; ++s) small = small && (!(in && pair[s]) || fabs(mid[s].arg) < 0.25);   // only slots that count: a slot without a partner, or a lane
                                                                                                      // past the last berg, reads a record nobody waited for (the empty mark is a NaN)
      if (__ballot(!small) == 0ull) {
#pragma unroll
        for (int s = 0; s < MB; ++s) th[s] = kid_sin_series15(mid[s].arg);   // x - x^3/3! + ... - x^15/15!
      } else {
#pragma unroll
        for (int s = 0; s < MB; ++s) th[s] = pair_theta(p, mid[s].arg);
      }
#pragma unroll
      for (int s = 0; s < MB; ++s) rs[s] = pair_finish(p, pc[s], mid[s], th[s]);
    }
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      double fx = 0., fy = 0., fdx = 0., fdy = 0., tq = 0., tdq = 0.;
#ifdef KID_EXP_MTS_NOPAIR   // measurement only: the loop without the pair evaluations (what the record exchange + the own row cost)
      if (false) {
#else
      if (sweep[s] && br[s] == 0) {
#endif
        const double sg = prim[s] ? 1. : -1.;                           // the partner's copies of the bond state are the negatives of the primary's
        const PairOut &r = rs[s];
        if (r.status == 1) {
          if (last) { MBD(KID_BOND_F_X, s, kk) = 0.; MBD(KID_BOND_F_Y, s, kk) = 0.; MBD(KID_BOND_FD_X, s, kk) = 0.; MBD(KID_BOND_FD_Y, s, kk) = 0.;
                      MBD(KID_BOND_T, s, kk) = 0.; MBD(KID_BOND_T_D, s, kk) = 0.; }
        } else if (r.status == 2) {
          if (last) MBD(KID_BOND_LENGTH, s, kk) = r.len;
          if (prim[s]) unsafeAtomicAdd(m.red + MR_NERR, 1.);             // FATAL IB:1054
        } else {
          if (r.status == 3 && prim[s]) unsafeAtomicAdd(m.red + MR_NERR, 1.);   // FATAL IB:1206
          fx = sg * r.Fx; fy = sg * r.Fy; fdx = sg * r.Fdx; fdy = sg * r.Fdy; tq = prim[s] ? r.Tq : r.To_q; tdq = sg * r.Tdq;
          t1[s] = sg * r.tg1; t2[s] = sg * r.tg2; rr[s] = sg * r.relrot;
          if (last || r.broke) {   // the records (savestress, save_bond_forces) are what the last evaluation of the bond left
            MBD(KID_BOND_LENGTH, s, kk) = r.len;
            MBD(KID_BOND_TANGD1, s, kk) = t1[s]; MBD(KID_BOND_TANGD2, s, kk) = t2[s];
            MBD(KID_BOND_SSTRESS, s, kk) = r.sstress; MBD(KID_BOND_REL_ROTATION, s, kk) = rr[s]; MBD(KID_BOND_NSTRESS, s, kk) = r.nstress;
            MBD(KID_BOND_F_X, s, kk) = fx; MBD(KID_BOND_F_Y, s, kk) = fy; MBD(KID_BOND_FD_X, s, kk) = fdx; MBD(KID_BOND_FD_Y, s, kk) = fdy;
            MBD(KID_BOND_T, s, kk) = tq; MBD(KID_BOND_T_D, s, kk) = tdq;
          }
          if (r.broke) {   // each side marks its own record (1 also on a berg that is not swept, as in calculate_force_dem: labelling and downloads see the reference's mark)
            fresh |= 1 << s;
            br[s] = 1;
            m.bbroken[MB_S(s, kk)] = br[s];
            m.red[MR_BREAK] = 1.;
            if (p.use_broken_bonds_for_substep_contact) atomicSub(&MI(KID_BI_N_BONDS, kk), 1);
            unsafeAtomicAdd(m.red + MR_NBROKEN, 1.);
          }
        }
      } else if (pair[s] && br[s] == 3 && act_k) {   // a mark left by a step in which this berg was not swept: the stored forces once, then a contact
        fx = MBD(KID_BOND_F_X, s, kk); fy = MBD(KID_BOND_F_Y, s, kk); fdx = MBD(KID_BOND_FD_X, s, kk); fdy = MBD(KID_BOND_FD_Y, s, kk);
        tq = MBD(KID_BOND_T, s, kk); tdq = MBD(KID_BOND_T_D, s, kk);
        fresh |= 1 << s; br[s] = 1; m.bbroken[MB_S(s, kk)] = 1;
      }
      if (pair[s] && (br[s] != 1 || ((fresh >> s) & 1))) {
        F_x = F_x + fx; F_y = F_y + fy; Fd_x = Fd_x + fdx; Fd_y = Fd_y + fdy; Tq = Tq + tq; T_d = T_d + tdq;
      }
    }
    KID_TICK_ANY(1);
    if (act_k) {
      // ---- the rest of the velocity sweep of this berg (mts_velocity_kernel, explicit inner step with DEM bonds) ----
      const double axn = axf + bxf, ayn = ayf + byf;
      const double uvel3 = uvel + (dt_2 * axn), vvel3 = vvel + (dt_2 * ayn);
      const double u_star = uvel + (axn * (dt / 2.)), v_star = vvel + (ayn * (dt / 2.));
      double IA_x = 0., IA_y = 0., IAd_x = 0., IAd_y = 0.;
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        if (o[s] == -2) continue;                                               // past the end of the bond list
        if (o[s] < 0) { unsafeAtomicAdd(m.red + MR_NERR, 1.); continue; }
        if (br[s] == 1 && !((fresh >> s) & 1)) unbonded_dem_force(g, p, b, m, own, nb[s], kk, o[s], IA_x, IA_y, IAd_x, IAd_y, uvel, vvel, uvel, vvel);
      }
      const DemAccel d = dem_bond_accel(p, IA_x, IA_y, IAd_x, IAd_y, F_x, F_y, Fd_x, Fd_y, Tq, T_d, start_lon, rM, rI);
      ang_accel = d.ang_accel;
      const InnerAccel a = explicit_inner_accel(g, p, m, d.IA_x, d.IA_y, d.IAd_x, d.IAd_y, gdrag, uvel, vvel, u_star, v_star, ci_, cj_, dt, loc_dx);
      const UV vn = verlet_velocity(g, p, lon, lat, uvel3, vvel3, a.ax1, a.ay1, dt);
      axf = a.axn; ayf = a.ayn; bxf = 0.; byf = 0.; uvel = vn.u; vvel = vn.v;   // (bxn = byn = 0 in the explicit inner step)
      // ---- the berg's own-row tail of this sub-step (IB:6972-7044) and the position update of the next (IB:6786-6833) ----
      double w = own.w + dt * ang_accel;
      w = w * rw;
      own.w = w; own.rot = own.rot + dt * w;
      if (!last) {
        const LonLat q = verlet_position(g, p, lon, lat, vn.u, vn.v, a.axn, a.ayn, 0., 0., dt);
        lon = q.lon; lat = q.lat;
        own.lon = q.lon; own.lat = q.lat;
        const UV old = mts_old_velocity(vn.u, vn.v, a.axn, a.ayn, 0., dt_2);
        own.u = old.u; own.v = old.v;
      } else { own.u = vn.u; own.v = vn.v; }   // after the last sub-step only the tail: uvel_old = uvel (IB:6974), positions unchanged
    }
    KID_TICK_ANY(2);
    if (last) break;                                  // nobody reads the records of the last sub-step
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the mark set above is in memory before the record that lets the neighbours go on
    if (in) rec_store(nxt + 8 * kk, own);             // (a berg that is not swept copies its record along)
    KID_TICK_ANY(3);
  }
  KID_TICK_ANY(99);
  // ---- the state goes back to the berg arrays ----
  if (act_k) {
    MF(KID_B_LON, kk) = lon; MF(KID_B_LAT, kk) = lat; MF(KID_B_UVEL, kk) = uvel; MF(KID_B_VVEL, kk) = vvel;
    MF(KID_B_AXN_FAST, kk) = axf; MF(KID_B_AYN_FAST, kk) = ayf; MF(KID_B_BXN_FAST, kk) = bxf; MF(KID_B_BYN_FAST, kk) = byf;
    MF(KID_B_ANG_ACCEL, kk) = ang_accel;
    if (p.force_convergence) { MF(KID_B_AXN, kk) = axf; MF(KID_B_AYN, kk) = ayf; MF(KID_B_BXN, kk) = bxf; MF(KID_B_BYN, kk) = byf; }   // IB:7038-7043
    MF(KID_B_LON_OLD, kk) = own.lon; MF(KID_B_LAT_OLD, kk) = own.lat; MF(KID_B_UVEL_OLD, kk) = own.u; MF(KID_B_VVEL_OLD, kk) = own.v;
    MF(KID_B_ANG_VEL, kk) = own.w; MF(KID_B_ROT, kk) = own.rot;
  }
}

// IB:6949-6963 (force_convergence, implicit inner iteration not yet converged)
__global__ void __launch_bounds__(256) mts_inner_retry_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (!mts_active(b, k)) return;
  const double dt_2 = 0.5 * m.mts_fast_dt;
  const double u = MF(KID_B_UVEL, k), v = MF(KID_B_VVEL, k);
  MF(KID_B_UVEL_OLD, k) = u; MF(KID_B_VVEL_OLD, k) = v;
  MF(KID_B_UVEL, k) = u - dt_2 * (MF(KID_B_AXN_FAST, k) + MF(KID_B_BXN_FAST, k)) - dt_2 * (MF(KID_B_AXN, k) + MF(KID_B_BXN, k));
  MF(KID_B_VVEL, k) = v - dt_2 * (MF(KID_B_AYN_FAST, k) + MF(KID_B_BYN_FAST, k)) - dt_2 * (MF(KID_B_AYN, k) + MF(KID_B_BYN, k));
  MF(KID_B_AXN_FAST, k) = MF(KID_B_AXN, k); MF(KID_B_AYN_FAST, k) = MF(KID_B_AYN, k);
  MF(KID_B_BXN_FAST, k) = MF(KID_B_BXN, k); MF(KID_B_BYN_FAST, k) = MF(KID_B_BYN, k);
}

// final index update (IB:7053-7075)
__global__ void __launch_bounds__(256) mts_adjust_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                         const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  if (!(MF(KID_B_STATIC_BERG, k) < 0.5 && MF(KID_B_HALO_BERG, k) < 1)) return;
  MF(KID_B_UVEL_OLD, k) = MF(KID_B_UVEL, k); MF(KID_B_VVEL_OLD, k) = MF(KID_B_VVEL, k);
  double lonn = MF(KID_B_LON, k), latn = MF(KID_B_LAT, k), xi = MF(KID_B_XI, k), yj = MF(KID_B_YJ, k);
  int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k), err = 0;
  bool bail = false;
  adjust_index_and_ground<false>(g, p, nullptr, lonn, latn, i, j, xi, yj, err, bail);
  if (err) unsafeAtomicAdd(m.red + MR_NERR, 1.);
  MF(KID_B_LON, k) = lonn; MF(KID_B_LAT, k) = latn; MF(KID_B_LON_OLD, k) = lonn; MF(KID_B_LAT_OLD, k) = latn;
  MI(KID_BI_INE, k) = i; MI(KID_BI_JNE, k) = j; MF(KID_B_XI, k) = xi; MF(KID_B_YJ, k) = yj;
  if (i < g.isc || i > g.iec || j < g.jsc || j > g.jec) MI(KID_BI_ALIVE, k) = 0;  // leaves the PE, FW:3024-3041
}

// ---- break_bonds_dem FW:4713-4799 -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) break_mark_kernel(const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt,
                                                         const long long n, const int only_if_detected) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (only_if_detected && m.red[MR_BREAK] == 0.) return;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  double tn = p.frac_thres_n, tt = p.frac_thres_t;
  if (tn <= 0.0 && tt <= 0.0) return;
  if (tn <= 0.0) tn = HUGE_VAL;
  if (tt <= 0.0) tt = HUGE_VAL;
  const int cnt = m.bcount[k];
  for (int s = 0; s < cnt; ++s)
    if (MBD(KID_BOND_NSTRESS, s, k) > tn || MBD(KID_BOND_SSTRESS, s, k) > tt) {
      m.bbroken[MB_S(s, k)] = 2;   // other_id = -1 in the reference
      const int o = m.bother_row[MB_S(s, k)], so = m.bother_slot[MB_S(s, k)];
      if (o >= 0 && so >= 0) m.bbroken[MB_S(so, o)] = 2;
    }
}
// delete the bonds tagged 2, keeping list order (second loop of break_bonds_dem); also used after
// remove_broken_bonds_between_congloms, which tags with 2 as well
__global__ void __launch_bounds__(256) bond_delete_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n,
                                                          const int only_if_detected, const int count_as_break) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (only_if_detected && m.red[MR_BREAK] == 0.) return;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  const int cnt = m.bcount[k];
  int w = 0, dropped = 0;
  for (int s = 0; s < cnt; ++s) {
    if (m.bbroken[MB_S(s, k)] == 2) { ++dropped; continue; }
    if (w != s) {
      m.bother_id[MB_S(w, k)] = m.bother_id[MB_S(s, k)]; m.bbroken[MB_S(w, k)] = m.bbroken[MB_S(s, k)];
      m.bother_row[MB_S(w, k)] = m.bother_row[MB_S(s, k)];
      for (int f = 0; f < KID_NBOND_F64; ++f) MBD(f, w, k) = MBD(f, s, k);
    }
    ++w;
  }
  m.bcount[k] = w;
  if (dropped && count_as_break) {
    MI(KID_BI_N_BONDS, k) = MI(KID_BI_N_BONDS, k) - dropped;
    unsafeAtomicAdd(m.red + MR_NBROKEN, (double)dropped);
  }
}
// the matching-bond slot of every bond (the reference's other_bond pointer), after lists changed
__global__ void __launch_bounds__(256) bond_slots_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  const int cnt = m.bcount[k];
  for (int s = 0; s < cnt; ++s) {
    const int o = m.bother_row[MB_S(s, k)];
    int slot = -1;
    if (o >= 0) {
      const int co = m.bcount[o];
      for (int t = 0; t < co; ++t) if (m.bother_id[MB_S(t, o)] == b.id[k]) { slot = t; break; }
    }
    m.bother_slot[MB_S(s, k)] = slot;
  }
}
// orig_bond_length FW:4589-4614
__global__ void __launch_bounds__(256) bond_length_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  const int cnt = m.bcount[k];
  for (int s = 0; s < cnt; ++s) {
    const int o = m.bother_row[MB_S(s, k)];
    if (o < 0) continue;
    const double dx = MF(KID_B_LON, k) - MF(KID_B_LON, o), dy = MF(KID_B_LAT, k) - MF(KID_B_LAT, o);
    MBD(KID_BOND_LENGTH, s, k) = sqrt(kid_pow(dx, 2.) + kid_pow(dy, 2.));
  }
}

// ---- set_conglom_ids FW:2601-2646: connected components over unbroken bonds, numbered by first member ------------
__global__ void __launch_bounds__(256) conglom_init_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  m.label[k] = (MI(KID_BI_ALIVE, k) != 0) ? m.rank[k] : 0x7fffffff;
  MI(KID_BI_CONGLOM_ID, k) = 0;
}
__global__ void __launch_bounds__(256) conglom_propagate_kernel(const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt; const kid_params &p = *pp;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  int lab = m.label[k];
  const int lab0 = lab;
  const int cnt = m.mb ? m.bcount[k] : 0;
  for (int s = 0; s < cnt; ++s) {
    if (p.dem && m.bbroken[MB_S(s, k)] == 1) continue;
    const int o = m.bother_row[MB_S(s, k)];
    if (o >= 0) lab = min(lab, m.label[o]);
  }
  lab = min(lab, m.label[m.order[lab]]);  // pointer jumping: the label is the rank of a berg of the same conglomerate
  if (lab != lab0) { atomicMin(&m.label[k], lab); m.red[MR_CHANGED] = 1.; }
}
__global__ void __launch_bounds__(256) conglom_roots_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  m.root_flag[m.rank[k]] = (m.label[k] == m.rank[k]) ? 1 : 0;
}
__global__ void __launch_bounds__(256) conglom_assign_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  MI(KID_BI_CONGLOM_ID, k) = m.root_scan[m.label[k]] + 1;
}
// remove_broken_bonds_between_congloms FW:2689-2731: tag, then bond_delete_kernel + bond_slots_kernel
__global__ void __launch_bounds__(256) conglom_prune_kernel(const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt; const kid_params &p = *pp;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  if (!(MI(KID_BI_N_BONDS, k) < p.max_bonds)) return;
  const int cnt = m.bcount[k];
  for (int s = 0; s < cnt; ++s) {
    const int o = m.bother_row[MB_S(s, k)];
    if (m.bbroken[MB_S(s, k)] == 1 && o >= 0 && MI(KID_BI_CONGLOM_ID, o) != MI(KID_BI_CONGLOM_ID, k)) {
      m.bbroken[MB_S(s, k)] = 2;
      const int so = m.bother_slot[MB_S(s, k)];
      if (so >= 0) m.bbroken[MB_S(so, o)] = 2;
    }
  }
}

// ---- traversal order (SURVEY A13): keys for the LSD radix passes ------------------------------------------------
__global__ void __launch_bounds__(256) mts_key_f64_kernel(const double *__restrict__ fld, const int *__restrict__ rows, unsigned long long *__restrict__ keys, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const unsigned long long u = (unsigned long long)__double_as_longlong(fld[rows[q]]);
  keys[q] = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);  // order-preserving map of IEEE doubles
}
__global__ void __launch_bounds__(256) mts_key_i32_kernel(const int32_t *__restrict__ fld, const int *__restrict__ rows, unsigned long long *__restrict__ keys, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  keys[q] = (unsigned long long)((long long)fld[rows[q]] + 0x80000000ll);
}
__device__ __forceinline__ unsigned long long mts_cell_key(const DevGrid &g, const BergPtrs &b, long long k) {
  return (MI(KID_BI_ALIVE, k) != 0) ? (unsigned long long)g.idx(MI(KID_BI_INE, k), MI(KID_BI_JNE, k)) : 0xffffffffffffffffull;
}
__global__ void __launch_bounds__(256) mts_key_cell_kernel(const DevGrid g, const BergPtrs *__restrict__ bt, const int *__restrict__ rows, unsigned long long *__restrict__ keys,
                                                           unsigned long long *__restrict__ last_key, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const int k = rows[q];
  const unsigned long long key = mts_cell_key(g, *bt, k);
  keys[q] = key; last_key[k] = key;
}
// Has anything the conglomerate labelling reads of a berg changed since the last call -- alive, its bond list (partners' rows,
// broken marks) or its bond count?  One 64-bit signature per berg, compared and renewed.
__global__ void __launch_bounds__(256) bond_signature_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, unsigned long long *__restrict__ sig,
                                                             int *__restrict__ flag, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  unsigned long long h = 0xcbf29ce484222325ull;
  auto mix = [&h](unsigned long long v) { h = (h ^ v) * 0x100000001b3ull; h ^= h >> 29; };
  mix((unsigned long long)(unsigned)MI(KID_BI_ALIVE, k)); mix((unsigned long long)(unsigned)MI(KID_BI_N_BONDS, k));
  const int cnt = m.mb ? m.bcount[k] : 0;
  mix((unsigned long long)(unsigned)cnt);
  for (int s = 0; s < cnt; ++s) { mix((unsigned long long)(unsigned)m.bother_row[MB_S(s, k)]); mix((unsigned long long)(unsigned)m.bbroken[MB_S(s, k)]); }
  if (sig[k] != h) { sig[k] = h; *flag = 1; }
}
// has any row changed its cell (or died) since the order was built?
__global__ void __launch_bounds__(256) mts_key_check_kernel(const DevGrid g, const BergPtrs *__restrict__ bt, const unsigned long long *__restrict__ last_key, int *__restrict__ flag, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  if (mts_cell_key(g, *bt, k) != last_key[k]) *flag = 1;
}
__global__ void __launch_bounds__(256) mts_iota_kernel(int *__restrict__ rows, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q < n) rows[q] = (int)q;
}
// rank[row], cell_start[] from the sorted order (cell keys are in `keys`)
__global__ void __launch_bounds__(256) mts_rank_kernel(const int *__restrict__ order, const unsigned long long *__restrict__ keys, int32_t *__restrict__ rank,
                                                       int32_t *__restrict__ cell_start, const long long n, const int ncell) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  rank[order[q]] = (int)q;
  const unsigned long long c = keys[q];
  const unsigned long long prev = (q == 0) ? 0ull : keys[q - 1] + 1ull;   // cells (prev .. c] start at q
  if (c == 0xffffffffffffffffull) {  // first dead row closes every remaining cell
    if (q == 0 || keys[q - 1] != c) for (unsigned long long cc = (q == 0 ? 0ull : keys[q - 1] + 1ull); cc <= (unsigned long long)ncell; ++cc) cell_start[cc] = (int)q;
    return;
  }
  if (q == 0) { for (unsigned long long cc = 0; cc <= c; ++cc) cell_start[cc] = 0; }
  else if (keys[q - 1] != c) { for (unsigned long long cc = prev; cc <= c; ++cc) cell_start[cc] = (int)q; }
  if (q == n - 1) for (unsigned long long cc = c + 1ull; cc <= (unsigned long long)ncell; ++cc) cell_start[cc] = (int)n;
}

// quad_interp_from_agrid FW:7163-7252 applied to ocean_depth + ssh (IB:4894), one lane per berg
__global__ void __launch_bounds__(256) mts_depth_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                        const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0 || MF(KID_B_HALO_BERG, k) >= 0.5) return;
  const int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k);
  if (i < g.isc || i > g.iec || j < g.jsc || j > g.jec) return;
  const double x = MF(KID_B_LON, k), y = MF(KID_B_LAT, k), xi = MF(KID_B_XI, k), yj = MF(KID_B_YJ, k);
  const int mind = p.rev_mind ? 0 : 1;
  int is, ie, js, je;
  const int mi = ((i % 2) + 2) % 2, mj = ((j % 2) + 2) % 2;
  if (mi == mind) { if (xi >= 0.5) { is = i; ie = i + 2; } else { is = i - 2; ie = i; } } else { is = i - 1; ie = i + 1; }
  if (mj == mind) { if (yj >= 0.5) { js = j; je = j + 2; } else { js = j - 2; je = j; } } else { js = j - 1; je = j + 1; }
  if (is < g.isd || ie > g.ied || js < g.jsd || je > g.jed) { unsafeAtomicAdd(m.red + MR_NERR, 1.); return; }
  double x1 = m.lonc[g.idx(is, js)], y1 = m.latc[g.idx(is, js)];
  const double x2 = m.lonc[g.idx(ie, js)], y2 = m.latc[g.idx(ie, js)];
  const double x3 = m.lonc[g.idx(ie, je)], y3 = m.latc[g.idx(ie, je)];
  const double x4 = m.lonc[g.idx(is, je)], y4 = m.latc[g.idx(is, je)];
  double xloc, yloc;
  if (!g.latlon && g.regular) {
    const double dx = fabs(x3 - x4), dy = fabs(y3 - y2);
    x1 = x3 - (dx / 2); y1 = y3 - (dy / 2);
    const double Delta_x = mod_around(x, x1, g.Lx) - x1;
    xloc = ((Delta_x) / dx) + 0.5; yloc = ((y - y1) / dy) + 0.5;
  } else if ((dmax(dmax(y1, y2), dmax(y3, y4)) < 89.999) || !g.latlon) {
    (void)calc_xiyj(x1, x2, x3, x4, y1, y2, y3, y4, x, y, xloc, yloc, g.Lx);
  } else {
    const double pi_180 = p.pi / 180.;
    const double xx = (90. - y) * cos(x * pi_180), yy = (90. - y) * sin(x * pi_180);
    const double l1 = m.glon[g.idx(is, js)], l23 = m.glon[g.idx(ie, je)], l4 = m.glon[g.idx(is, je)];
    (void)calc_xiyj((90. - y1) * cos(l1 * pi_180), (90. - y2) * cos(l23 * pi_180), (90. - y3) * cos(l23 * pi_180), (90. - y4) * cos(l4 * pi_180),
                    (90. - y1) * sin(l1 * pi_180), (90. - y2) * sin(l23 * pi_180), (90. - y3) * sin(l23 * pi_180), (90. - y4) * sin(l4 * pi_180),
                    xx, yy, xloc, yloc, g.Lx);
  }
  xloc = xloc * 2 - 1; yloc = yloc * 2 - 1;
  const double xb[3] = {0.5 * xloc * (xloc - 1), (1 + xloc) * (1 - xloc), 0.5 * xloc * (xloc + 1)};
  const double yb[3] = {0.5 * yloc * (yloc - 1), (1 + yloc) * (1 - yloc), 0.5 * yloc * (yloc + 1)};
  double sum = 0.;
  for (int bb = 0; bb < 3; ++bb) for (int a = 0; a < 3; ++a) {
    const int c = g.idx(is + a, js + bb);
    sum = sum + xb[a] * yb[bb] * (g.ocean_depth[c] + g.ssh[c]);
  }
  MF(KID_B_OD, k) = sum;
}

// counters kept in red[] join the step's scalar block (KID_S_*), which the gather folds into the running totals
__global__ void mts_fold_kernel(const MtsDev *__restrict__ mt, double *__restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double *red = mt->red;
  scal[KID_S_NSPEEDING_TICKETS] += red[MR_NTICKETS]; scal[KID_S_ERROR_COUNT] += red[MR_NERR]; scal[KID_S_NBONDS_BROKEN] += red[MR_NBROKEN];
  red[MR_NTICKETS] = 0.; red[MR_NERR] = 0.; red[MR_NBROKEN] = 0.;
}

__global__ void __launch_bounds__(256) cell_conglom_kernel(const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const int ncell) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncell) return;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  int id = -1;
  const int q0 = m.cell_start[c], q1 = m.cell_start[c + 1];
  if (q1 > q0) {
    id = MI(KID_BI_CONGLOM_ID, m.order[q0]);
    for (int q = q0 + 1; q < q1; ++q) if (MI(KID_BI_CONGLOM_ID, m.order[q]) != id) { id = -1; break; }
  }
  m.cell_conglom[c] = id;
}

// ---- single-time-step scheme with interacting bergs (interactive_icebergs_on, mts=.false.), Verlet and RK4 ----------
// Both integrators are two sweeps of one lane per berg (evolve_icebergs IB:7081-7200).  The first sweep reads of OTHER bergs only
// what the second sweep writes (lon_old, lat_old, uvel_old, vvel_old), what no sweep writes (thickness, length, width, mass, id,
// fl_k, conglom_id) and the cell tables of mts_prologue, so neither depends on the order of the rows:
//   Verlet  sts_ia_velocity_kernel (velocities), sts_ia_position_kernel (update_verlet_position, the *_old copies)
//   RK4     sts_ia_rk4_kernel (Runge_Kutta_stepping: four accel calls, position and velocity), sts_ia_rk4_old_kernel (the *_old copies)
// accel IB:1950-2442 with the interactive terms
__device__ __noinline__ void accel_sts_ia(const DevGrid &g, const kid_params &p, const BergPtrs &b, const MtsDev &m, long long k, const Env &e,
                                          int i, int j, double lat, double uvel, double vvel, double uvel0, double vvel0, double dt,
                                          double &ax, double &ay, double &axn, double &ayn, double &bxn, double &byn) {
  const double pi_180 = p.pi / 180.;
  const double Cr0 = 0.06;
  const bool RK = p.Runge_not_Verlet != 0;
  const double alpha = RK ? 0.0 : 1.0, beta = 1.0, C_N = RK ? 0.0 : 1.0;
  const bool new_pc = RK ? (p.use_new_predictive_corrective != 0) : true;
  const double u_star = uvel0 + (axn * (dt / 2.)), v_star = vvel0 + (ayn * (dt / 2.));
  const double uo = e.uo, vo = e.vo, ui = e.ui, vi = e.vi, ua = e.ua, va = e.va, ssh_x = e.ssh_x, ssh_y = e.ssh_y, od = e.od;
  double hi = e.hi;
  double f_cori;
  if (g.latlon && !p.use_f_plane) f_cori = (2. * p.omega) * sin(pi_180 * lat);
  else f_cori = (2. * p.omega) * sin(pi_180 * p.lat_ref);
  const double M = MF(KID_B_MASS, k), T = MF(KID_B_THICKNESS, k);
  const double D = (p.rho_bergs / RHO_SEAWATER) * T, F = T - D;
  const double W = MF(KID_B_WIDTH, k), L = MF(KID_B_LENGTH, k);
  axn = 0.; ayn = 0.; bxn = 0.; byn = 0.;
  hi = dmin(hi, D);
  const double D_hi = dmax(0., D - hi);
  double groundfrac;
  if (p.h_to_init_grounding > 0.0) { groundfrac = 1.0 - (od - D) / p.h_to_init_grounding; groundfrac = dmax(groundfrac, 0.0); groundfrac = dmin(groundfrac, 1.0); }
  else groundfrac = (D > od) ? 1.0 : 0.0;
  const double c_gnd = (groundfrac > 0.0) ? (p.cdrag_grounding * W * L * groundfrac) / M : 0.0;
  double uwave = ua - uo, vwave = va - vo;
  double wmod = uwave * uwave + vwave * vwave;
  const double ampl = 0.5 * 0.02025 * wmod, Lwavelength = 0.32 * wmod, Lcutoff = 0.125 * Lwavelength, Ltop = 0.25 * Lwavelength;
  const double Cr = Cr0 * dmin(dmax(0., (L - Lcutoff) / ((Ltop - Lcutoff) + 1.e-30)), 1.);
  double wave_rad = 0.5 * RHO_SEAWATER / M * Cr * GRAVITY * ampl * dmin(ampl, F) * (2. * W * L) / (W + L);
  wmod = sqrt(ua * ua + va * va);
  if (wmod != 0.) { uwave = ua / wmod; vwave = va / wmod; } else { uwave = 0.; vwave = 0.; wave_rad = 0.; }
  double dragfrac = 1.0;
  if (p.iceberg_bonds_on && p.internal_bergs_for_drag) {
    double N_bonds = 0., N_max = 4.0;
    if (p.hexagonal_icebergs) N_max = 6.0;
    const int cnt = m.bcount[k];
    for (int s = 0; s < cnt; ++s) {
      if (p.dem) { if (m.bbroken[MB_S(s, k)] != 1) N_bonds = N_bonds + 1.0; } else N_bonds = N_bonds + 1.0;
    }
    dragfrac = ((N_max - N_bonds) / N_max);
  }
  const double c_ocn = RHO_SEAWATER / M * p.ocean_drag_scale * (0.5 * CD_WV * dragfrac * W * (D_hi) + CD_WH * W * L);
  const double c_atm = RHO_AIR / M * (0.5 * CD_AV * dragfrac * W * F + CD_AH * W * L);
  double c_ice = (fabs(hi) == 0.) ? 0. : RHO_ICE / M * (0.5 * CD_IV * dragfrac * W * hi);
  if (fabs(ui) + fabs(vi) == 0.) c_ice = 0.;
  if (!RK) { axn = -GRAVITY * ssh_x + wave_rad * uwave; ayn = -GRAVITY * ssh_y + wave_rad * vwave; }
  else { bxn = -GRAVITY * ssh_x + wave_rad * uwave; byn = -GRAVITY * ssh_y + wave_rad * vwave; }
  IaSum S{0., 0., 0., 0., 0., 0., 0., 0.};
  const bool ia_on = p.interactive_icebergs_on != 0;
  if (ia_on) {
    interactive_force(g, p, b, m, k, 0, S, uvel0, vvel0, uvel0, vvel0);
    if (!RK) { axn = axn + S.IA_x; ayn = ayn + S.IA_y; } else { bxn = bxn + S.IA_x; byn = byn + S.IA_y; }
  }
  if (alpha > 0.) {
    if (C_N > 0.) { axn = axn + f_cori * v_star; ayn = ayn - f_cori * u_star; }
    else { bxn = bxn + f_cori * v_star; byn = byn - f_cori * u_star; }
  } else { bxn = bxn + f_cori * vvel; byn = byn - f_cori * uvel; }
  double uveln = new_pc ? uvel0 : uvel, vveln = new_pc ? vvel0 : vvel;
  double us = uvel0, vs = vvel0;
#pragma unroll 1
  for (int itloop = 1; itloop <= 2; ++itloop) {
    if (itloop == 2) { us = uveln; vs = vveln; }
    double drag_ocn, drag_atm, drag_ice;
    if (new_pc) {
      drag_ocn = c_ocn * 0.5 * (sqrt((uveln - uo) * (uveln - uo) + (vveln - vo) * (vveln - vo)) + sqrt((uvel0 - uo) * (uvel0 - uo) + (vvel0 - vo) * (vvel0 - vo)));
      drag_atm = c_atm * 0.5 * (sqrt((uveln - ua) * (uveln - ua) + (vveln - va) * (vveln - va)) + sqrt((uvel0 - ua) * (uvel0 - ua) + (vvel0 - va) * (vvel0 - va)));
      drag_ice = c_ice * 0.5 * (sqrt((uveln - ui) * (uveln - ui) + (vveln - vi) * (vveln - vi)) + sqrt((uvel0 - ui) * (uvel0 - ui) + (vvel0 - vi) * (vvel0 - vi)));
    } else {
      us = 0.5 * (uveln + uvel); vs = 0.5 * (vveln + vvel);
      drag_ocn = c_ocn * sqrt((us - uo) * (us - uo) + (vs - vo) * (vs - vo));
      drag_atm = c_atm * sqrt((us - ua) * (us - ua) + (vs - va) * (vs - va));
      drag_ice = c_ice * sqrt((us - ui) * (us - ui) + (vs - vi) * (vs - vi));
    }
    const double drag_gnd = c_gnd;
    double RHS_x = (axn / 2) + bxn, RHS_y = (ayn / 2) + byn;
    RHS_x = RHS_x - drag_ocn * (u_star - uo) - drag_atm * (u_star - ua) - drag_ice * (u_star - ui) - drag_gnd * u_star;  // beta = 1
    RHS_y = RHS_y - drag_ocn * (v_star - vo) - drag_atm * (v_star - va) - drag_ice * (v_star - vi) - drag_gnd * v_star;
    if (ia_on) {
      if (itloop > 1) interactive_force(g, p, b, m, k, 0, S, uvel0, vvel0, us, vs);
      RHS_x = RHS_x - (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
      RHS_y = RHS_y - (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
    }
    double A11, A12, A21, A22;
    if (p.only_interactive_forces) {
      RHS_x = (S.IA_x / 2) - (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
      RHS_y = (S.IA_y / 2) - (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
      A11 = 1 + (dt * S.P11); A12 = (dt * S.P12); A21 = (dt * S.P21); A22 = 1 + (dt * S.P22);
    } else {
      const double lambda = drag_ocn + drag_atm + drag_ice + drag_gnd;
      A11 = 1. + beta * dt * lambda; A22 = 1. + beta * dt * lambda;
      A12 = -alpha * dt * f_cori; A21 = alpha * dt * f_cori;
      if (C_N > 0.) { A12 = A12 / 2.; A21 = A21 / 2.; }
      if (ia_on) { A11 = A11 + (dt * S.P11); A12 = A12 + (dt * S.P12); A21 = A21 + (dt * S.P21); A22 = A22 + (dt * S.P22); }
    }
    const double detA = 1. / ((A11 * A22) - (A12 * A21));
    ax = detA * (A22 * RHS_x - A12 * RHS_y); ay = detA * (A11 * RHS_y - A21 * RHS_x);
    uveln = u_star + dt * ax; vveln = v_star + dt * ay;
  }
  if (p.only_interactive_forces) { axn = S.IA_x; ayn = S.IA_y; }
  else {
    axn = 0.; ayn = 0.;
    if (!RK) {
      axn = -GRAVITY * ssh_x + wave_rad * uwave; ayn = -GRAVITY * ssh_y + wave_rad * vwave;
      if (ia_on) { axn = axn + S.IA_x; ayn = ayn + S.IA_y; }
    }
    if (C_N > 0.) { axn = axn + f_cori * vveln; ayn = ayn - f_cori * uveln; }
  }
  bxn = ax - (axn / 2); byn = ay - (ayn / 2);
  speed_limit(g, p, m, i, j, dt, uveln, vveln);
  if (p.override_iceberg_velocities) { ax = 0.; ay = 0.; axn = 0.; ayn = 0.; bxn = 0.; byn = 0.; }
}

// first sweep of evolve_icebergs (IB:7103-7177) with verlet_stepping (IB:7203-7328): velocities only
__global__ void __launch_bounds__(256) sts_ia_velocity_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                              const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0 || !(MF(KID_B_STATIC_BERG, k) < 0.5)) return;
  if (MF(KID_B_HALO_BERG, k) >= 0.5) return;   // a neighbour tile's berg (kid_halo_bergs.inc): a force source, its owner steps it
  const double dt = p.dt, dt_2 = 0.5 * dt;
  const double lonn = MF(KID_B_LON, k), latn = MF(KID_B_LAT, k);
  double axn = MF(KID_B_AXN, k), ayn = MF(KID_B_AYN, k), bxn = MF(KID_B_BXN, k), byn = MF(KID_B_BYN, k);
  const double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k);
  const int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k);
  MF(KID_B_UVEL_PREV, k) = uvel1 - dt_2 * bxn; MF(KID_B_VVEL_PREV, k) = vvel1 - dt_2 * byn;
  const double uvel3 = uvel1 + (dt_2 * axn), vvel3 = vvel1 + (dt_2 * ayn);
  Env e;
  if (p.old_interp_flds_order) interp_flds(p, GlbCell{g, g.idx(i, j)}, MF(KID_B_XI, k), MF(KID_B_YJ, k), e);
  else {
    e.uo = MF(KID_B_UO, k); e.vo = MF(KID_B_VO, k); e.ui = MF(KID_B_UI, k); e.vi = MF(KID_B_VI, k); e.ua = MF(KID_B_UA, k); e.va = MF(KID_B_VA, k);
    e.ssh_x = MF(KID_B_SSH_X, k); e.ssh_y = MF(KID_B_SSH_Y, k); e.sst = MF(KID_B_SST, k); e.sss = MF(KID_B_SSS, k); e.cn = MF(KID_B_CN, k);
    e.hi = MF(KID_B_HI, k); e.od = MF(KID_B_OD, k);
  }
  double ax1, ay1;
  accel_sts_ia(g, p, b, m, k, e, i, j, latn, uvel1, vvel1, uvel1, vvel1, dt, ax1, ay1, axn, ayn, bxn, byn);
  const UV vn = verlet_velocity(g, p, lonn, latn, uvel3, vvel3, ax1, ay1, dt);
  double uveln = vn.u, vveln = vn.v;
  if (p.override_iceberg_velocities) { uveln = p.u_override; vveln = p.v_override; }
  MF(KID_B_AXN, k) = axn; MF(KID_B_AYN, k) = ayn; MF(KID_B_BXN, k) = bxn; MF(KID_B_BYN, k) = byn;
  // neighbours read uvel_old / vvel_old, never uvel / vvel: safe to write in place
  MF(KID_B_UVEL, k) = uveln; MF(KID_B_VVEL, k) = vveln;
}
// second sweep (IB:7180-7198): update_verlet_position (IB:7684-7764) and the *_old copies
__global__ void __launch_bounds__(256) sts_ia_position_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                              const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  // a halo row has served (the velocity sweep is done): retired, never moved, and its cell put back inside as the emigrant
  // packer does with a packed row, so that nothing takes it for a leaver waiting to be packed
  if (MF(KID_B_HALO_BERG, k) >= 0.5) { MI(KID_BI_ALIVE, k) = 0; MI(KID_BI_INE, k) = g.isc; MI(KID_BI_JNE, k) = g.jsc; return; }
  if (!(MF(KID_B_STATIC_BERG, k) < 0.5)) return;
  const double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k);
  const LonLat q = verlet_position(g, p, MF(KID_B_LON, k), MF(KID_B_LAT, k), uvel1, vvel1, MF(KID_B_AXN, k), MF(KID_B_AYN, k), MF(KID_B_BXN, k), MF(KID_B_BYN, k), p.dt);
  double lonn = q.lon, latn = q.lat;
  int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k), err = 0;
  double xi = MF(KID_B_XI, k), yj = MF(KID_B_YJ, k);
  bool bail = false;
  adjust_index_and_ground<false>(g, p, nullptr, lonn, latn, i, j, xi, yj, err, bail);
  if (err) unsafeAtomicAdd(m.red + MR_NERR, 1.);
  MF(KID_B_LON, k) = lonn; MF(KID_B_LAT, k) = latn; MI(KID_BI_INE, k) = i; MI(KID_BI_JNE, k) = j; MF(KID_B_XI, k) = xi; MF(KID_B_YJ, k) = yj;
  MF(KID_B_UVEL_OLD, k) = uvel1; MF(KID_B_VVEL_OLD, k) = vvel1; MF(KID_B_LON_OLD, k) = lonn; MF(KID_B_LAT_OLD, k) = latn;
  if (i < g.isc || i > g.iec || j < g.jsc || j > g.jec) MI(KID_BI_ALIVE, k) = 0;
}

// first sweep of evolve_icebergs (IB:7106-7179) with Runge_Kutta_stepping (IB:7331-7683) and accel_sts_ia as its acceleration.
// The four stages are one rolled body, as in the general build of rk4_step (kid_device.hpp), with the reference's own
// arithmetic: the partial sums A = q1 (+ q4), B = q2 (+ q3) give (q1 + q4) + 2 (q2 + q3) of IB:7597-7616 in its association.
// What a pair force reads of a berg -- *_old, the sizes, id, fl_k, conglom_id, the cell tables -- no lane writes here; what the
// lane writes at its end is read by nobody else.  interactive_force centres its search on ine, jne of the ROW, the berg's cell
// at the start of the step (the lists are not re-linked between stages): they are written after the last stage.
__global__ void __launch_bounds__(256) sts_ia_rk4_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                         const MtsDev *__restrict__ mt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  if (MI(KID_BI_ALIVE, k) == 0 || !(MF(KID_B_STATIC_BERG, k) < 0.5)) return;
  if (MF(KID_B_HALO_BERG, k) >= 0.5) return;
  const double dt = p.dt, dt_2 = 0.5 * dt, dt_6 = dt / 6.;
  const int i1 = MI(KID_BI_INE, k), j1 = MI(KID_BI_JNE, k);
  const double xi1 = MF(KID_B_XI, k), yj1 = MF(KID_B_YJ, k), lon1 = MF(KID_B_LON, k), lat1 = MF(KID_B_LAT, k);
  const double uvel1 = MF(KID_B_UVEL, k), vvel1 = MF(KID_B_VVEL, k), axn0 = MF(KID_B_AXN, k), ayn0 = MF(KID_B_AYN, k);
  const bool on_tang = (lat1 > 89.) && g.latlon;   // IB:7393
  const double dydl = g.latlon ? (180. / p.pi) / p.Rearth : 1.;
  Env e;
  if (!p.old_interp_flds_order) {
    e.uo = MF(KID_B_UO, k); e.vo = MF(KID_B_VO, k); e.ui = MF(KID_B_UI, k); e.vi = MF(KID_B_VI, k); e.ua = MF(KID_B_UA, k); e.va = MF(KID_B_VA, k);
    e.ssh_x = MF(KID_B_SSH_X, k); e.ssh_y = MF(KID_B_SSH_Y, k); e.sst = MF(KID_B_SST, k); e.sss = MF(KID_B_SSS, k); e.cn = MF(KID_B_CN, k);
    e.hi = MF(KID_B_HI, k); e.od = MF(KID_B_OD, k);
  }
  double bxn = 0., byn = 0.;
  double x1 = 0., y1 = 0., xdot1 = 0., ydot1 = 0.;
  if (on_tang) { rotpos_to_tang(p, lon1, lat1, x1, y1); rotvec_to_tang(p, lon1, uvel1, vvel1, xdot1, ydot1); }
  double Au = 0., Bu = 0., Av = 0., Bv = 0., Aax = 0., Bax = 0., Aay = 0., Bay = 0., Aaxn = 0., Baxn = 0., Aayn = 0., Bayn = 0.;
  double lon_s = lon1, lat_s = lat1, uvel_s = uvel1, vvel_s = vvel1, xdot_s = xdot1, ydot_s = ydot1;
  int i = i1, j = j1, err = 0; double xi = xi1, yj = yj1;
  bool bail = false;
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    if (s > 0) { i = i1; j = j1; xi = xi1; yj = yj1; adjust_index_and_ground<false>(g, p, nullptr, lon_s, lat_s, i, j, xi, yj, err, bail); }  // IB:7430-7431
    const double dxdl = g.latlon ? (180. / p.pi) / (p.Rearth * cos((lat_s) * (p.pi / 180.))) : 1.;
    double qu = uvel_s * dxdl, qv = vvel_s * dydl;
    if (p.old_interp_flds_order) interp_flds(p, GlbCell{g, g.idx(i, j)}, xi, yj, e);
    double axn_s = axn0, ayn_s = ayn0, ax, ay;
    accel_sts_ia(g, p, b, m, k, e, i, j, lat_s, uvel_s, vvel_s, uvel1, vvel1, (s < 2) ? dt_2 : dt, ax, ay, axn_s, ayn_s, bxn, byn);
    double qax = ax, qay = ay, qaxn = axn_s, qayn = ayn_s;
    if (on_tang) {
      qu = xdot_s; qv = ydot_s;
      rotvec_to_tang(p, lon_s, ax, ay, qax, qay);
      rotvec_to_tang(p, lon_s, axn_s, ayn_s, qaxn, qayn);
    }
    if (s == 0)      { Au = qu; Av = qv; Aax = qax; Aay = qay; Aaxn = qaxn; Aayn = qayn; }
    else if (s == 1) { Bu = qu; Bv = qv; Bax = qax; Bay = qay; Baxn = qaxn; Bayn = qayn; }
    else if (s == 2) { Bu = Bu + qu; Bv = Bv + qv; Bax = Bax + qax; Bay = Bay + qay; Baxn = Baxn + qaxn; Bayn = Bayn + qayn; }
    else             { Au = Au + qu; Av = Av + qv; Aax = Aax + qax; Aay = Aay + qay; Aaxn = Aaxn + qaxn; Aayn = Aayn + qayn; }
    if (s < 3) {  // X_{k+1} = X1 + c V_k ; V_{k+1} = V1 + c A_k   (c = dt/2, dt/2, dt)
      const double c = (s < 2) ? dt_2 : dt;
      if (on_tang) {
        const double xs = x1 + c * qu, ys = y1 + c * qv;
        xdot_s = xdot1 + c * qax; ydot_s = ydot1 + c * qay;
        rotpos_from_tang(p, xs, ys, lon_s, lat_s);
        rotvec_from_tang(p, lon_s, xdot_s, ydot_s, uvel_s, vvel_s);
      } else {
        lon_s = lon1 + c * qu; lat_s = lat1 + c * qv;
        uvel_s = uvel1 + c * ax; vvel_s = vvel1 + c * ay;
      }
    }
  }
  double lonn, latn, uveln, vveln, axn, ayn;
  if (on_tang) {
    const double xn = x1 + dt_6 * (Au + 2. * Bu), yn = y1 + dt_6 * (Av + 2. * Bv);
    const double xdotn = xdot1 + dt_6 * (Aax + 2. * Bax), ydotn = ydot1 + dt_6 * (Aay + 2. * Bay);
    const double xddotn = (Aaxn + 2. * Baxn) / 6., yddotn = (Aayn + 2. * Bayn) / 6.;
    rotpos_from_tang(p, xn, yn, lonn, latn);
    rotvec_from_tang(p, lonn, xdotn, ydotn, uveln, vveln);
    rotvec_from_tang(p, lonn, xddotn, yddotn, axn, ayn);   // bxn, byn stay as the 4th accel call left them
  } else {
    lonn = lon1 + dt_6 * (Au + 2. * Bu); latn = lat1 + dt_6 * (Av + 2. * Bv);
    uveln = uvel1 + dt_6 * (Aax + 2. * Bax); vveln = vvel1 + dt_6 * (Aay + 2. * Bay);
    axn = (Aaxn + 2. * Baxn) / 6.; ayn = (Aayn + 2. * Bayn) / 6.;
    bxn = ((Aax + 2. * Bax) / 6) - (axn / 2); byn = ((Aay + 2. * Bay) / 6) - (ayn / 2);
  }
  i = i1; j = j1; xi = xi1; yj = yj1;
  adjust_index_and_ground<false>(g, p, nullptr, lonn, latn, i, j, xi, yj, err, bail);
  if (err) unsafeAtomicAdd(m.red + MR_NERR, 1.);
  if (p.override_iceberg_velocities) { uveln = p.u_override; vveln = p.v_override; }   // IB:7151-7154
  MF(KID_B_AXN, k) = axn; MF(KID_B_AYN, k) = ayn; MF(KID_B_BXN, k) = bxn; MF(KID_B_BYN, k) = byn;
  MF(KID_B_UVEL, k) = uveln; MF(KID_B_VVEL, k) = vveln; MF(KID_B_LON, k) = lonn; MF(KID_B_LAT, k) = latn;
  MF(KID_B_XI, k) = xi; MF(KID_B_YJ, k) = yj; MI(KID_BI_INE, k) = i; MI(KID_BI_JNE, k) = j;
}
// second sweep under RK4 (IB:7182-7197): nothing moves, the *_old members the next step's pair forces read take the new state
__global__ void __launch_bounds__(256) sts_ia_rk4_old_kernel(const DevGrid g, const BergPtrs *__restrict__ bt, const long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt;
  if (MI(KID_BI_ALIVE, k) == 0) return;
  if (MF(KID_B_HALO_BERG, k) >= 0.5) { MI(KID_BI_ALIVE, k) = 0; MI(KID_BI_INE, k) = g.isc; MI(KID_BI_JNE, k) = g.jsc; return; }   // as sts_ia_position_kernel
  if (!(MF(KID_B_STATIC_BERG, k) < 0.5)) return;
  MF(KID_B_UVEL_OLD, k) = MF(KID_B_UVEL, k); MF(KID_B_VVEL_OLD, k) = MF(KID_B_VVEL, k);
  MF(KID_B_LON_OLD, k) = MF(KID_B_LON, k); MF(KID_B_LAT_OLD, k) = MF(KID_B_LAT, k);
  const int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k);
  if (i < g.isc || i > g.iec || j < g.jsc || j > g.jec) MI(KID_BI_ALIVE, k) = 0;
}

// find_orientation_using_iceberg_bonds IB:3829-3892, one lane per berg (radians out, read as degrees by the hexagon code)
__global__ void __launch_bounds__(256) bond_orientation_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                               const MtsDev *__restrict__ mt, const long long n, double *__restrict__ orient) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  double orientation = p.initial_orientation;
  const int ine = MI(KID_BI_INE, k), jne = MI(KID_BI_JNE, k);
  if (MI(KID_BI_ALIVE, k) != 0 && (ine > g.isd) && (ine < g.ied) && (jne >= g.jsd) && (jne <= g.jed)) {
    double bond_count = 0., Average_angle = 0.;
    const double lat1 = MF(KID_B_LAT, k), lon1 = MF(KID_B_LON, k);
    const int cnt = m.bcount[k];
    for (int s = 0; s < cnt; ++s) {
      const int o = m.bother_row[MB_S(s, k)];
      if (o < 0) continue;
      const double lat2 = MF(KID_B_LAT, o), lon2 = MF(KID_B_LON, o);
      double dx_dlon, dy_dlat; grid_to_meters(g, p, 0.5 * (lat1 + lat2), dx_dlon, dy_dlat);
      const double rx = (lon2 - lon1) * dx_dlon, ry = (lat2 - lat1) * dy_dlat;
      double angle;
      if (rx == 0.) angle = p.pi / 2.;
      else {
        angle = atan(ry / rx);
        angle = ((p.pi / 2.) - (orientation * (p.pi / 180.))) - angle;
        angle = f_modulo(angle, p.pi / 3.);
      }
      bond_count = bond_count + 1.;
      Average_angle = Average_angle + angle;
    }
    if (bond_count > 0) Average_angle = Average_angle / bond_count; else Average_angle = 0.;
    orientation = f_modulo(Average_angle, p.pi / 3.);
  }
  orient[k] = orientation;
}
