/* kid_oracle_mts.c -- CPU restatement (ORACLE, test infrastructure) of the multiple-time-stepping / DEM path.
 *   evolve_icebergs_mts                        /root/reference/src/icebergs.F90:6576-7078
 *   accel_mts                                  IB:1278-1706
 *   accel_explicit_inner_mts                   IB:1710-1947
 *   interactive_force, calculate_force         IB:480-804
 *   calculate_unbonded_same_conglom_dem_force  IB:807-955
 *   calculate_force_dem                        IB:959-1242
 *   break_bonds_dem                            /root/reference/src/icebergs_framework.F90:4713-4799
 *   set_conglom_ids, label_conglomerates, remove_broken_bonds_between_congloms   FW:2601-2731
 *   orig_bond_length                           FW:4589-4614
 *   quad_interp_from_agrid                     FW:7163-7252
 *
 * One PE, whole conglomerates resident (the reference replicates whole conglomerates per PE, IB:6602-6609): there are
 * no halo bergs, so transfer_mts_bergs (FW:2136-2216) reduces to set_conglom_ids.  save_bond_forces=.true. (the
 * module default, FW:53): each bond pair is evaluated once per sub-step, by whichever of its two bergs comes first in
 * the traversal order (j outer, i inner, list order inside a cell), and mirrored to the other side.
 * Not restated: print_fracture, dem_beam_test = 3 (the angular-velocity test), A68_test, skip_first_outer_mts_step, no_frac_first_ts (both one-shot
 * module flags, default F), STS interactive bergs (the non-MTS second sweep of evolve_icebergs).
 * PARITY UNPINNED: the reference tree holds no recorded vector for this path that can be recomputed here (its DEM
 * regression numbers depend on netCDF restarts made by Python/netCDF4 tooling that is not in the image).
 */
#include "kid_oracle.h"
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define RHO_SEAWATER 1025.0
#define RHO_AIR 1.1
#define RHO_ICE 916.7
#define GRAVITY 9.8
#define CD_AV 1.3
#define CD_AH 0.0055
#define CD_WV 0.9
#define CD_WH 0.0012
#define CD_IV 0.9
#define NI(g) ((g)->d.ied - (g)->d.isd + 1)
#define NJ(g) ((g)->d.jed - (g)->d.jsd + 1)
#define GIDX(g, i, j) ((size_t)((i) - (g)->d.isd) + (size_t)((j) - (g)->d.jsd) * (size_t)NI(g))
#define GS(g, F, i, j) ((g)->stat[F][GIDX(g, i, j)])
#define GF(g, F, i, j) ((g)->forc[F][GIDX(g, i, j)])

void ko_meters_to_grid(const ko_grid *g, const kid_params *p, double lat_ref, double *dlon_dx, double *dlat_dy);
void ko_rotpos_to_tang(const kid_params *p, double lon, double lat, double *x, double *y);
void ko_rotpos_from_tang(const kid_params *p, double x, double y, double *lon, double *lat);
void ko_rotvec_to_tang(const kid_params *p, double lon, double uvel, double vvel, double *xdot, double *ydot);
void ko_rotvec_from_tang(const kid_params *p, double lon, double xdot, double ydot, double *uvel, double *vvel);

static inline double dmin(double a, double b) { return a < b ? a : b; }
static inline double dmax(double a, double b) { return a > b ? a : b; }

typedef struct mts_ctx {
  const ko_grid *g; const kid_params *p; kid_berg_soa *b; kid_bond_soa *bd;
  int64_t n; int mb;
  int64_t *perm; int64_t nperm;   /* alive rows in traversal order */
  int64_t *cell_start;            /* [ncell+1] into perm */
  int64_t *other_row;             /* [mb*n] row of the bond's other berg (-1: not resident) */
  int32_t *other_slot;            /* [mb*n] slot of the matching bond on the other berg */
  unsigned char *mark;            /* [mb*n] "other_id<0": the matching side has already evaluated this pair */
  int mts_part, only_interactive;
  double constant_area, constant_radius, dem_K_damp, mts_fast_dt;
  double *scalars;
  int bond_break_detected;
} mts_ctx;

#define BF(f, k) (c->b->f64[f][k])
#define BI(f, k) (c->b->i32[f][k])
#define BS(s, k) ((size_t)(s) * (size_t)c->n + (size_t)(k))
#define BD(f, s, k) (c->bd->f64[f][BS(s, k)])

/* IB:444-459 */
static void grid_to_meters(const mts_ctx *c, double lat_ref, double *dx_dlon, double *dy_dlat) {
  if (c->g->d.grid_is_latlon) {
    *dx_dlon = (c->p->pi / 180.) * c->p->Rearth * cos((lat_ref) * (c->p->pi / 180.));
    *dy_dlat = (c->p->pi / 180.) * c->p->Rearth;
  } else { *dx_dlon = 1.; *dy_dlat = 1.; }
}

static void derived_params(mts_ctx *c) { /* FW:1436, 1453-1463, 1301 */
  const kid_params *p = c->p;
  c->dem_K_damp = 2. * p->dem_spring_coef / (3. * (1. - pow(p->poisson, 2.)));
  c->constant_area = p->constant_length * p->constant_width;
  if (p->hexagonal_icebergs) c->constant_radius = sqrt(c->constant_area / (2. * sqrt(3.)));
  else if (p->iceberg_bonds_on) c->constant_radius = 0.5 * sqrt(c->constant_area);
  else c->constant_radius = sqrt(c->constant_area / p->pi);
  c->mts_fast_dt = p->dt / (double)p->mts_sub_steps;
}

/* ---- index maps: traversal order, cell lists, bond partners (connect_all_bonds FW:4963-5125) ---- */
typedef struct idrow { int64_t id, row; } idrow;
static int cmp_idrow(const void *a, const void *b) {
  const idrow *x = (const idrow *)a, *y = (const idrow *)b;
  return x->id < y->id ? -1 : (x->id > y->id ? 1 : 0);
}
static int ctx_init(mts_ctx *c, const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars) {
  memset(c, 0, sizeof(*c));
  c->g = g; c->p = p; c->b = b; c->bd = bd; c->n = b->n; c->mb = bd ? bd->max_bonds : 0; c->scalars = scalars;
  derived_params(c);
  const size_t n = (size_t)(b->n > 0 ? b->n : 1), ncell = (size_t)NI(g) * (size_t)NJ(g);
  int64_t *all = (int64_t *)malloc(n * sizeof(int64_t));
  c->perm = (int64_t *)malloc(n * sizeof(int64_t));
  ko_reference_order(b, all);
  c->nperm = 0;
  for (int64_t q = 0; q < b->n; ++q) if (BI(KID_BI_ALIVE, all[q]) != 0) c->perm[c->nperm++] = all[q];
  free(all);
  c->cell_start = (int64_t *)calloc(ncell + 1, sizeof(int64_t));
  for (int64_t q = 0; q < c->nperm; ++q) c->cell_start[GIDX(g, BI(KID_BI_INE, c->perm[q]), BI(KID_BI_JNE, c->perm[q])) + 1]++;
  for (size_t q = 0; q < ncell; ++q) c->cell_start[q + 1] += c->cell_start[q];
  if (c->mb > 0) {
    const size_t nb = (size_t)c->mb * n;
    c->other_row = (int64_t *)malloc(nb * sizeof(int64_t));
    c->other_slot = (int32_t *)malloc(nb * sizeof(int32_t));
    c->mark = (unsigned char *)calloc(nb, 1);
    idrow *tab = (idrow *)malloc(n * sizeof(idrow));
    int64_t nt = 0;
    for (int64_t k = 0; k < b->n; ++k) if (BI(KID_BI_ALIVE, k) != 0) { tab[nt].id = b->id[k]; tab[nt].row = k; ++nt; }
    qsort(tab, (size_t)nt, sizeof(idrow), cmp_idrow);
    for (int64_t k = 0; k < b->n; ++k)
      for (int s = 0; s < c->mb; ++s) {
        c->other_row[BS(s, k)] = -1; c->other_slot[BS(s, k)] = -1;
        if (BI(KID_BI_ALIVE, k) == 0 || s >= bd->count[k]) continue;
        idrow key; key.id = bd->other_id[BS(s, k)]; key.row = 0;
        const idrow *hit = (const idrow *)bsearch(&key, tab, (size_t)nt, sizeof(idrow), cmp_idrow);
        if (hit) c->other_row[BS(s, k)] = hit->row;
      }
    for (int64_t k = 0; k < b->n; ++k)
      for (int s = 0; s < c->mb; ++s) {
        const int64_t o = c->other_row[BS(s, k)];
        if (o < 0) continue;
        for (int t = 0; t < bd->count[o]; ++t) if (bd->other_id[BS(t, o)] == b->id[k]) { c->other_slot[BS(s, k)] = t; break; }
      }
    free(tab);
  }
  return 0;
}
static void ctx_free(mts_ctx *c) { free(c->perm); free(c->cell_start); free(c->other_row); free(c->other_slot); free(c->mark); }

static int is_partner(const mts_ctx *c, int64_t k, int64_t o) { /* the id-negation mark of IB:537, 1772, 1797 */
  if (c->mb == 0) return 0;
  for (int s = 0; s < c->bd->count[k]; ++s) if (c->other_row[BS(s, k)] == o) return 1;
  return 0;
}

/* interaction radius of an element of footprint A (Stern et al 2017 eq 4), IB:693-705 */
static double radius_of(const kid_params *p, double A) {
  if (p->hexagonal_icebergs) return sqrt(A / (2. * sqrt(3.)));
  if (p->iceberg_bonds_on) return 0.5 * sqrt(A);
  return sqrt(A / p->pi);
}

typedef struct ia_sum { double IA_x, IA_y, P11, P12, P21, P22, Ptu_x, Ptu_y; } ia_sum;

/* IB:611-804.  c_crit_dist: -1 absent, 0 .false., 1 .true. */
static void calculate_force(const mts_ctx *c, int64_t k, int64_t o, ia_sum *S, double u0, double v0, double u1, double v1,
                            int bonded, int c_crit_dist) {
  const kid_params *p = c->p;
  if (!(c->b->id[k] != c->b->id[o] && BF(KID_B_FL_K, k) != -1 && BF(KID_B_FL_K, o) != -1)) return;
  const double T1 = BF(KID_B_THICKNESS, k), lon1 = BF(KID_B_LON_OLD, k), lat1 = BF(KID_B_LAT_OLD, k);
  const double T2 = BF(KID_B_THICKNESS, o), lon2 = BF(KID_B_LON_OLD, o), lat2 = BF(KID_B_LAT_OLD, o);
  const double u2 = BF(KID_B_UVEL_OLD, o), v2 = BF(KID_B_VVEL_OLD, o);
  double A1, M1, A2, M2;
  if (p->constant_interaction_LW && p->mts && bonded) {
    A1 = p->constant_length * p->constant_width; M1 = A1 * T1 * p->rho_bergs; A2 = A1; M2 = A2 * T2 * p->rho_bergs;
  } else {
    M1 = BF(KID_B_MASS, k); A1 = BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k);
    M2 = BF(KID_B_MASS, o); A2 = BF(KID_B_LENGTH, o) * BF(KID_B_WIDTH, o);
  }
  const double dlon = lon1 - lon2, dlat = lat1 - lat2;
  double dx_dlon, dy_dlat; grid_to_meters(c, 0.5 * (lat1 + lat2), &dx_dlon, &dy_dlat);
  const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
  const double r_dist = sqrt((rx * rx) + (ry * ry));
  const double R1 = radius_of(p, A1), R2 = radius_of(p, A2);
  const double M_min = dmin(M1, M2);
  double crit_dist, spring_coef;
  if (bonded) { crit_dist = R1 + R2; spring_coef = p->spring_coef; }
  else {
    spring_coef = p->contact_spring_coef;
    if (c_crit_dist == 1) { crit_dist = R1 + R2; spring_coef = p->spring_coef; }
    else crit_dist = dmax(R1 + R2, p->contact_distance);
  }
  double radial = p->radial_damping_coef, tang = p->tangental_damping_coef;
  if (p->critical_interaction_damping_on) {
    radial = 2. * sqrt(spring_coef);
    if (p->tang_crit_int_damp_on) tang = (2. * sqrt(spring_coef)) / 4;
  }
  int tbonded = bonded;
  if (bonded && !(p->mts || (p->contact_distance > 0.) || (p->contact_spring_coef != p->spring_coef)))
    if (!(r_dist > crit_dist)) tbonded = 0;
  if ((r_dist > 0.) && (tbonded || (r_dist < crit_dist && !bonded))) {
    const double accel_spring = spring_coef * (M_min / M1) * (crit_dist - r_dist);
    S->IA_x = S->IA_x + (accel_spring * (rx / r_dist));
    S->IA_y = S->IA_y + (accel_spring * (ry / r_dist));
    double P_11 = (rx * rx) / (r_dist * r_dist), P_12 = (rx * ry) / (r_dist * r_dist);
    double P_21 = (rx * ry) / (r_dist * r_dist), P_22 = (ry * ry) / (r_dist * r_dist);
    double coef = radial * (M_min / M1);
    if (p->scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    S->P11 += coef * P_11; S->P12 += coef * P_12; S->P21 += coef * P_21; S->P22 += coef * P_22;
    S->Ptu_x = S->Ptu_x + (coef * ((P_11 * u2) + (P_12 * v2)));
    S->Ptu_y = S->Ptu_y + (coef * ((P_12 * u2) + (P_22 * v2)));
    P_11 = 1 - P_11; P_12 = -P_12; P_21 = -P_21; P_22 = 1 - P_22;
    coef = tang * (M_min / M1);
    if (p->scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    S->P11 += coef * P_11; S->P12 += coef * P_12; S->P21 += coef * P_21; S->P22 += coef * P_22;
    S->Ptu_x = S->Ptu_x + (coef * ((P_11 * u2) + (P_12 * v2)));
    S->Ptu_y = S->Ptu_y + (coef * ((P_12 * u2) + (P_22 * v2)));
  }
}

/* IB:480-607 */
static void interactive_force(const mts_ctx *c, int64_t k, ia_sum *S, double u0, double v0, double u1, double v1) {
  const kid_params *p = c->p; const ko_grid *g = c->g;
  memset(S, 0, sizeof(*S));
  if (BF(KID_B_FL_K, k) == -1) return;
  const int ine = BI(KID_BI_INE, k), jne = BI(KID_BI_JNE, k);
  const int nc_x = p->contact_cells_lon, nc_y = p->contact_cells_lat;
  if (p->mts || (p->contact_distance > 0.) || (p->contact_spring_coef != p->spring_coef)) {
    if (!p->mts || (p->mts && c->mts_part == 3)) {
      if (p->iceberg_bonds_on) {
        for (int s = 0; s < c->bd->count[k]; ++s) {
          const int64_t o = c->other_row[BS(s, k)];
          if (o >= 0) calculate_force(c, k, o, S, u0, v0, u1, v1, 1, -1);
        }
        const int j0 = jne - 2 > g->d.jsd + 1 ? jne - 2 : g->d.jsd + 1, j1 = jne + 2 < g->d.jed ? jne + 2 : g->d.jed;
        const int i0 = ine - 2 > g->d.isd + 1 ? ine - 2 : g->d.isd + 1, i1 = ine + 2 < g->d.ied ? ine + 2 : g->d.ied;
        for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi)
          for (int64_t q = c->cell_start[GIDX(g, gi, gj)]; q < c->cell_start[GIDX(g, gi, gj) + 1]; ++q) {
            const int64_t o = c->perm[q];
            if (!is_partner(c, k, o) && BI(KID_BI_CONGLOM_ID, o) == BI(KID_BI_CONGLOM_ID, k))
              calculate_force(c, k, o, S, u0, v0, u1, v1, 0, 1);
          }
      }
    }
    if (!(p->mts && c->mts_part == 3)) {
      const int j0 = jne - nc_y > g->d.jsd ? jne - nc_y : g->d.jsd, j1 = jne + nc_y < g->d.jed ? jne + nc_y : g->d.jed;
      const int i0 = ine - nc_x > g->d.isd ? ine - nc_x : g->d.isd, i1 = ine + nc_x < g->d.ied ? ine + nc_x : g->d.ied;
      for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi)
        for (int64_t q = c->cell_start[GIDX(g, gi, gj)]; q < c->cell_start[GIDX(g, gi, gj) + 1]; ++q) {
          const int64_t o = c->perm[q];
          if (BI(KID_BI_CONGLOM_ID, o) != BI(KID_BI_CONGLOM_ID, k)) calculate_force(c, k, o, S, u0, v0, u1, v1, 0, -1);
        }
    }
  } else {
    for (int gj = jne - 1; gj <= jne + 1; ++gj) for (int gi = ine - 1; gi <= ine + 1; ++gi)
      for (int64_t q = c->cell_start[GIDX(g, gi, gj)]; q < c->cell_start[GIDX(g, gi, gj) + 1]; ++q)
        calculate_force(c, k, c->perm[q], S, u0, v0, u1, v1, 0, -1);
    if (p->iceberg_bonds_on)
      for (int s = 0; s < c->bd->count[k]; ++s) {
        const int64_t o = c->other_row[BS(s, k)];
        if (o >= 0) calculate_force(c, k, o, S, u0, v0, u1, v1, 1, -1);
      }
  }
}

/* IB:807-955 */
static void unbonded_same_conglom_dem_force(const mts_ctx *c, int64_t k, int64_t o, double *IA_x, double *IA_y,
                                            double *IAd_x, double *IAd_y, double u0, double v0, double u1, double v1) {
  const kid_params *p = c->p;
  if (!(c->b->id[k] != c->b->id[o] && BF(KID_B_FL_K, k) != -1 && BF(KID_B_FL_K, o) != -1)) return;
  const double dlon = BF(KID_B_LON_OLD, k) - BF(KID_B_LON_OLD, o), dlat = BF(KID_B_LAT_OLD, k) - BF(KID_B_LAT_OLD, o);
  double dx_dlon, dy_dlat; grid_to_meters(c, 0.5 * (BF(KID_B_LAT_OLD, k) + BF(KID_B_LAT_OLD, o)), &dx_dlon, &dy_dlat);
  const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
  double r_dist = (rx * rx) + (ry * ry);
  double R1, R2, M1, M2;
  if (p->constant_interaction_LW) {
    if (pow(2 * c->constant_radius, 2.) <= r_dist) return;
    R1 = c->constant_radius;
    M1 = c->constant_area * BF(KID_B_THICKNESS, k) * p->rho_bergs;
    M2 = c->constant_area * BF(KID_B_THICKNESS, o) * p->rho_bergs;
    R2 = R1;
  } else {
    const double A1 = BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k), A2 = BF(KID_B_LENGTH, o) * BF(KID_B_WIDTH, o);
    R1 = radius_of(p, A1); R2 = radius_of(p, A2);
    if (pow(R1 + R2, 2.) <= r_dist) return;
    M1 = BF(KID_B_MASS, k); M2 = BF(KID_B_MASS, o);
  }
  r_dist = sqrt(r_dist);
  const double u2 = BF(KID_B_UVEL_OLD, o), v2 = BF(KID_B_VVEL_OLD, o);
  const double M_min = dmin(M1, M2), crit_dist = R1 + R2, spring_coef = p->spring_coef;
  double radial = p->radial_damping_coef, tang = p->tangental_damping_coef;
  if (p->critical_interaction_damping_on) {
    radial = 2. * sqrt(spring_coef);
    if (p->tang_crit_int_damp_on) tang = (2. * sqrt(spring_coef)) / 4;
  }
  if ((r_dist > 0.) && (r_dist < crit_dist)) {
    const double accel_spring = spring_coef * (M_min / M1) * (crit_dist - r_dist);
    *IA_x = *IA_x + (accel_spring * (rx / r_dist));
    *IA_y = *IA_y + (accel_spring * (ry / r_dist));
    double P_11 = (rx * rx) / (r_dist * r_dist), P_12 = (rx * ry) / (r_dist * r_dist), P_22 = (ry * ry) / (r_dist * r_dist);
    double coef = radial * (M_min / M1);
    if (p->scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    double Pia11 = coef * P_11, Pia12 = coef * P_12, Pia22 = coef * P_22;
    P_11 = 1 - P_11; P_12 = -P_12; P_22 = 1 - P_22;
    coef = tang * (M_min / M1);
    if (p->scale_damping_by_pmag) {
      const double a1 = (P_11 * (u2 - u1)) + (P_12 * (v2 - v1)), a2 = (P_12 * (u2 - u1)) + (P_22 * (v2 - v1));
      const double b1 = (P_11 * (u2 - u0)) + (P_12 * (v2 - v0)), b2 = (P_12 * (u2 - u0)) + (P_22 * (v2 - v0));
      coef = coef * (0.5 * (sqrt((a1 * a1) + (a2 * a2)) + sqrt((b1 * b1) + (b2 * b2))));
    }
    Pia11 = Pia11 + coef * P_11; Pia12 = Pia12 + coef * P_12; Pia22 = Pia22 + coef * P_22;
    const double du = BF(KID_B_UVEL_OLD, o) - BF(KID_B_UVEL_OLD, k), dv = BF(KID_B_VVEL_OLD, o) - BF(KID_B_VVEL_OLD, k);
    *IAd_x = *IAd_x + Pia11 * du + Pia12 * dv;
    *IAd_y = *IAd_y + Pia12 * du + Pia22 * dv;
  }
}

typedef struct dem_sum { double F_x, F_y, T, Fd_x, Fd_y, T_d; } dem_sum;

/* IB:959-1242 with savestress=.true., save_bond_forces=.true.; (k,s) is the bond being processed */
static void calculate_force_dem(mts_ctx *c, int64_t k, int s, double dt, dem_sum *D) {
  const kid_params *p = c->p;
  const int64_t o = c->other_row[BS(s, k)];
  const int so = c->other_slot[BS(s, k)];
  if (!(c->b->id[k] != c->b->id[o] && BF(KID_B_FL_K, k) != -1 && BF(KID_B_FL_K, o) != -1)) return;
  const double hexdenom = 1. / (2. * sqrt(3.));
  double M1, M2, R1, R2, Rmin, l0, T_Rmin;
  if (p->constant_interaction_LW) {
    M1 = c->constant_area * BF(KID_B_THICKNESS, k) * p->rho_bergs;
    M2 = c->constant_area * BF(KID_B_THICKNESS, o) * p->rho_bergs;
    R1 = c->constant_radius; R2 = R1; Rmin = R1; l0 = 2 * R1; T_Rmin = BF(KID_B_THICKNESS, o);
  } else {
    M1 = BF(KID_B_MASS, k); M2 = BF(KID_B_MASS, o);
    const double A1 = BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k), A2 = BF(KID_B_LENGTH, o) * BF(KID_B_WIDTH, o);
    if (p->hexagonal_icebergs) { R1 = sqrt(A1 * hexdenom); R2 = sqrt(A2 * hexdenom); }
    else { R1 = 0.5 * sqrt(A1); R2 = 0.5 * sqrt(A2); }
    if (R1 < R2) { Rmin = R1; T_Rmin = BF(KID_B_THICKNESS, k); } else { Rmin = R2; T_Rmin = BF(KID_B_THICKNESS, o); }
    l0 = R1 + R2;
  }
  double dx_dlon, dy_dlat; grid_to_meters(c, 0.5 * (BF(KID_B_LAT_OLD, k) + BF(KID_B_LAT_OLD, o)), &dx_dlon, &dy_dlat);
  const double rx = (BF(KID_B_LON_OLD, k) - BF(KID_B_LON_OLD, o)) * dx_dlon;
  const double ry = (BF(KID_B_LAT_OLD, k) - BF(KID_B_LAT_OLD, o)) * dy_dlat;
  const double len = sqrt((rx * rx) + (ry * ry));
  BD(KID_BOND_LENGTH, s, k) = len;
  if (len == 0) { c->scalars[KID_S_ERROR_COUNT] += 1.; return; } /* FATAL IB:1054 */
  const double n1 = rx / len, n2 = ry / len;
  const double half_delta = 0.5 * (l0 - len);
  const double RR1 = R1 - half_delta, RR2 = R2 - half_delta;
  const double RR1x = RR1 * n1, RR1y = RR1 * n2, RR2x = RR2 * n1, RR2y = RR2 * n2;
  const double L = 2.0 * (Rmin + (Rmin - half_delta) * fabs(R1 - R2) / len);
  const double Thick = T_Rmin + (Rmin - half_delta) * fabs(BF(KID_B_THICKNESS, k) - BF(KID_B_THICKNESS, o)) / len;
  double Fn_x = p->dem_spring_coef * Thick * 2. * half_delta * L / l0;
  const double Fn_y = Fn_x * n2; Fn_x = Fn_x * n1;
  const double ur = BF(KID_B_UVEL_OLD, k) - BF(KID_B_UVEL_OLD, o), vr = BF(KID_B_VVEL_OLD, k) - BF(KID_B_VVEL_OLD, o);
  { /* savestress */
    const double t1 = BD(KID_BOND_TANGD1, s, k), t2 = BD(KID_BOND_TANGD2, s, k);
    const double tmag = t1 * t1 + t2 * t2;
    const double tangdotnt = t1 * n1 + t2 * n2;
    double tangd1p = t1 - tangdotnt * n1, tangd2p = t2 - tangdotnt * n2;
    const double tmagp = tangd1p * tangd1p + tangd2p * tangd2p;
    if (tmagp > 0.) { const double t_rat = sqrt(tmag / tmagp); tangd1p = t_rat * tangd1p; tangd2p = t_rat * tangd2p; }
    else { tangd1p = 0.; tangd2p = 0.; }
    const double rotu = RR1y * BF(KID_B_ANG_VEL, k) + RR2y * BF(KID_B_ANG_VEL, o);
    const double rotv = -(RR1x * BF(KID_B_ANG_VEL, k) + RR2x * BF(KID_B_ANG_VEL, o));
    const double ur2 = ur + rotu, vr2 = vr + rotv;
    double up = ur2 * n1 + vr2 * n2; const double vp = up * n2; up = up * n1;
    BD(KID_BOND_TANGD1, s, k) = tangd1p + (ur2 - up) * dt; BD(KID_BOND_TANGD2, s, k) = tangd2p + (vr2 - vp) * dt;
  }
  double ss_factor = -L * Thick * p->dem_spring_coef / (l0 * 2.0 * (1.0 + p->poisson));
  if (p->ignore_tangential_force) ss_factor = 0.;
  const double Fs_x = ss_factor * BD(KID_BOND_TANGD1, s, k), Fs_y = ss_factor * BD(KID_BOND_TANGD2, s, k);
  BD(KID_BOND_SSTRESS, s, k) = sqrt(Fs_x * Fs_x + Fs_y * Fs_y) / (L * Thick);
  const double Ts = -(RR1x * Fs_y - RR1y * Fs_x);
  BD(KID_BOND_REL_ROTATION, s, k) = BD(KID_BOND_REL_ROTATION, s, k) + (BF(KID_B_ANG_VEL, k) - BF(KID_B_ANG_VEL, o)) * dt;
  double theta, Tr;
  if (!p->orig_dem_moment_of_inertia) {
    theta = sin(BF(KID_B_ROT, k) - BF(KID_B_ROT, o));
    Tr = -p->dem_spring_coef * pow(L, 3.) * Thick * theta / (12. * l0);
  } else {
    theta = BF(KID_B_ROT, k) - BF(KID_B_ROT, o);
    Tr = -(p->dem_spring_coef / l0) * (2. / 3.) * pow(0.5 * L, 3.) * Thick * theta;
  }
  BD(KID_BOND_NSTRESS, s, k) = (p->dem_spring_coef / l0) * (-2 * half_delta + fabs(theta * 0.5 * L));
  const double nstress = BD(KID_BOND_NSTRESS, s, k), sstress = BD(KID_BOND_SSTRESS, s, k);
  double damping_coef = 0.;
#define MIRROR_STATE() do { if (so >= 0) { \
    BD(KID_BOND_NSTRESS, so, o) = nstress; BD(KID_BOND_SSTRESS, so, o) = sstress; \
    BD(KID_BOND_REL_ROTATION, so, o) = -BD(KID_BOND_REL_ROTATION, s, k); \
    BD(KID_BOND_TANGD1, so, o) = -BD(KID_BOND_TANGD1, s, k); BD(KID_BOND_TANGD2, so, o) = -BD(KID_BOND_TANGD2, s, k); \
    BD(KID_BOND_LENGTH, so, o) = len; } } while (0)
  if (p->break_bonds_on_sub_steps) {
    if (p->fracture_criterion_stress) {
      if (nstress > p->frac_thres_n || sstress > p->frac_thres_t) {
        c->bond_break_detected = 1;
        if (c->bd->broken[BS(s, k)] != 1) { c->bd->broken[BS(s, k)] = 1; c->scalars[KID_S_NBONDS_BROKEN] += 1.; }
        if (nstress < 0) {
          damping_coef = p->dem_damping_coef * sqrt(c->dem_K_damp * M1 * M2 / (M1 + M2));
          D->Fd_x = D->Fd_x - damping_coef * ur; D->Fd_y = D->Fd_y - damping_coef * vr;
          D->F_x = D->F_x + Fn_x; D->F_y = D->F_y + Fn_y;
        }
        if (p->use_broken_bonds_for_substep_contact) BI(KID_BI_N_BONDS, k) = BI(KID_BI_N_BONDS, k) - 1;
        BD(KID_BOND_T, s, k) = 0.; BD(KID_BOND_T_D, s, k) = 0.;
        if (nstress < 0) {
          BD(KID_BOND_F_X, s, k) = Fn_x; BD(KID_BOND_F_Y, s, k) = Fn_y;
          BD(KID_BOND_FD_X, s, k) = -damping_coef * ur; BD(KID_BOND_FD_Y, s, k) = -damping_coef * vr;
        } else {
          BD(KID_BOND_F_X, s, k) = 0.; BD(KID_BOND_F_Y, s, k) = 0.; BD(KID_BOND_FD_X, s, k) = 0.; BD(KID_BOND_FD_Y, s, k) = 0.;
        }
        if (so >= 0) {
          BD(KID_BOND_F_X, so, o) = -BD(KID_BOND_F_X, s, k); BD(KID_BOND_F_Y, so, o) = -BD(KID_BOND_F_Y, s, k);
          BD(KID_BOND_FD_X, so, o) = -BD(KID_BOND_FD_X, s, k); BD(KID_BOND_FD_Y, so, o) = -BD(KID_BOND_FD_Y, s, k);
          BD(KID_BOND_T, so, o) = 0.; BD(KID_BOND_T_D, so, o) = 0.;
          MIRROR_STATE();
          if (c->bd->broken[BS(so, o)] != 1) c->scalars[KID_S_NBONDS_BROKEN] += 1.;
          c->bd->broken[BS(so, o)] = 1;
          c->mark[BS(so, o)] = 1;
          if (p->use_broken_bonds_for_substep_contact) BI(KID_BI_N_BONDS, o) = BI(KID_BI_N_BONDS, o) - 1;
        }
        return;
      }
    } else { c->scalars[KID_S_ERROR_COUNT] += 1.; return; } /* FATAL IB:1206 */
  }
  damping_coef = p->dem_damping_coef * sqrt(c->dem_K_damp * M1 * M2 / (M1 + M2));
  BD(KID_BOND_F_X, s, k) = Fn_x + Fs_x; BD(KID_BOND_F_Y, s, k) = Fn_y + Fs_y;
  BD(KID_BOND_FD_X, s, k) = -damping_coef * ur; BD(KID_BOND_FD_Y, s, k) = -damping_coef * vr;
  BD(KID_BOND_T, s, k) = Ts + Tr;
  BD(KID_BOND_T_D, s, k) = -damping_coef * (BF(KID_B_ANG_VEL, k) - BF(KID_B_ANG_VEL, o));
  if (so >= 0) {
    BD(KID_BOND_F_X, so, o) = -BD(KID_BOND_F_X, s, k); BD(KID_BOND_F_Y, so, o) = -BD(KID_BOND_F_Y, s, k);
    BD(KID_BOND_FD_X, so, o) = -BD(KID_BOND_FD_X, s, k); BD(KID_BOND_FD_Y, so, o) = -BD(KID_BOND_FD_Y, s, k);
    BD(KID_BOND_T, so, o) = Ts - Tr; BD(KID_BOND_T_D, so, o) = -BD(KID_BOND_T_D, s, k);
    MIRROR_STATE();
    c->mark[BS(so, o)] = 1;
  }
  D->Fd_x = D->Fd_x - damping_coef * ur; D->Fd_y = D->Fd_y - damping_coef * vr;
  D->T_d = D->T_d - damping_coef * (BF(KID_B_ANG_VEL, k) - BF(KID_B_ANG_VEL, o));
  D->T = D->T + (Ts + Tr);
  D->F_x = D->F_x + Fn_x + Fs_x; D->F_y = D->F_y + Fn_y + Fs_y;
#undef MIRROR_STATE
}

/* calculate_force_dem above for ONE pair given by value, on a context of two bergs with one bond each (tests/test_dem_pair_cpu.py
 * holds it to a 50-digit restatement of IB:959-1242).  Berg 0 evaluates, berg 1 is its partner.
 *   id[2];  x[KO_DEM_PAIR_NIN] = {fl_k, thickness, mass, length, width, lon_old, lat_old, uvel_old, vvel_old, ang_vel, rot} of berg 0,
 *   the same eleven of berg 1, then tangd1, tangd2, rel_rotation of berg 0's side of the bond, and dt;
 *   out[KO_DEM_PAIR_NOUT] = berg 0's bond {length, tangd1, tangd2, nstress, sstress, rel_rotation, F_x, F_y, Fd_x, Fd_y, T, T_d}
 *   (the order of KID_BOND_*), the same twelve of berg 1's side, the sums the caller accumulates {F_x, F_y, T, Fd_x, Fd_y, T_d},
 *   broken of the two sides, n_bonds of the two bergs (2 going in), error_count, nbonds_broken, bond_break_detected, and the derived
 *   constant_area, constant_radius, dem_K_damp. */
enum { KO_DEM_PAIR_NIN = 26, KO_DEM_PAIR_NOUT = 2 * KID_NBOND_F64 + 6 + 10 };
void ko_dem_pair(const kid_params *p, int latlon, const int64_t *id, const double *x, double *out) {
  static const int fld[11] = {KID_B_FL_K, KID_B_THICKNESS, KID_B_MASS, KID_B_LENGTH, KID_B_WIDTH, KID_B_LON_OLD, KID_B_LAT_OLD,
                              KID_B_UVEL_OLD, KID_B_VVEL_OLD, KID_B_ANG_VEL, KID_B_ROT};
  double bf[KID_NB_F64][2]; int32_t bi[KID_NB_I32][2]; int64_t ids[2] = {id[0], id[1]};
  double df[KID_NBOND_F64][2]; int32_t count[2] = {1, 1}, broken[2] = {0, 0}; int64_t other_id[2] = {id[1], id[0]};
  double scalars[KID_NSCALAR];
  int64_t other_row[2] = {1, 0}; int32_t other_slot[2] = {0, 0}; unsigned char mark[2] = {0, 0};
  memset(bf, 0, sizeof(bf)); memset(bi, 0, sizeof(bi)); memset(df, 0, sizeof(df)); memset(scalars, 0, sizeof(scalars));
  kid_berg_soa b; kid_bond_soa bd; ko_grid g; mts_ctx c;
  memset(&b, 0, sizeof(b)); memset(&bd, 0, sizeof(bd)); memset(&g, 0, sizeof(g)); memset(&c, 0, sizeof(c));
  b.n = 2; b.id = ids;
  for (int f = 0; f < KID_NB_F64; ++f) b.f64[f] = bf[f];
  for (int f = 0; f < KID_NB_I32; ++f) b.i32[f] = bi[f];
  for (int k = 0; k < 2; ++k) {
    for (int q = 0; q < 11; ++q) bf[fld[q]][k] = x[11 * k + q];
    bi[KID_BI_ALIVE][k] = 1; bi[KID_BI_N_BONDS][k] = 2;
  }
  bd.n = 2; bd.max_bonds = 1; bd.count = count; bd.other_id = other_id; bd.broken = broken;
  for (int f = 0; f < KID_NBOND_F64; ++f) bd.f64[f] = df[f];
  df[KID_BOND_TANGD1][0] = x[22]; df[KID_BOND_TANGD2][0] = x[23]; df[KID_BOND_REL_ROTATION][0] = x[24];
  df[KID_BOND_TANGD1][1] = -x[22]; df[KID_BOND_TANGD2][1] = -x[23]; df[KID_BOND_REL_ROTATION][1] = -x[24];
  g.d.grid_is_latlon = latlon ? 1 : 0;
  c.g = &g; c.p = p; c.b = &b; c.bd = &bd; c.n = 2; c.mb = 1; c.scalars = scalars;
  c.other_row = other_row; c.other_slot = other_slot; c.mark = mark;
  derived_params(&c);
  dem_sum D = {0., 0., 0., 0., 0., 0.};
  calculate_force_dem(&c, 0, 0, x[25], &D);
  int q = 0;
  for (int k = 0; k < 2; ++k) for (int f = 0; f < KID_NBOND_F64; ++f) out[q++] = df[f][k];
  out[q++] = D.F_x; out[q++] = D.F_y; out[q++] = D.T; out[q++] = D.Fd_x; out[q++] = D.Fd_y; out[q++] = D.T_d;
  out[q++] = (double)broken[0]; out[q++] = (double)broken[1];
  out[q++] = (double)bi[KID_BI_N_BONDS][0]; out[q++] = (double)bi[KID_BI_N_BONDS][1];
  out[q++] = scalars[KID_S_ERROR_COUNT]; out[q++] = scalars[KID_S_NBONDS_BROKEN]; out[q++] = (double)c.bond_break_detected;
  out[q++] = c.constant_area; out[q++] = c.constant_radius; out[q++] = c.dem_K_damp;
}

/* the speed limit block shared by accel_mts and accel_explicit_inner_mts (IB:1542-1563, 1918-1939) */
static void speed_limit(const mts_ctx *c, int i, int j, double dt, double *uveln, double *vveln) {
  const kid_params *p = c->p; const ko_grid *g = c->g;
  if ((p->speed_limit > 0.) || (p->speed_limit == -1.)) {
    const double speed = sqrt(*uveln * *uveln + *vveln * *vveln);
    if (speed > 0.) {
      const double loc_dx = dmin(0.5 * (GS(g, KID_G_DX, i, j) + GS(g, KID_G_DX, i, j - 1)), 0.5 * (GS(g, KID_G_DY, i, j) + GS(g, KID_G_DY, i - 1, j)));
      const double new_speed = loc_dx / dt * p->speed_limit;
      if (new_speed < speed && p->speed_limit > 0.) {
        *uveln = *uveln * (new_speed / speed); *vveln = *vveln * (new_speed / speed);
        c->scalars[KID_S_NSPEEDING_TICKETS] += 1.;
      }
    }
  }
}

/* IB:1278-1706 */
static void accel_mts(mts_ctx *c, int64_t k, int i, int j, double lat, double *uvel, double *vvel, double *uvel0, double *vvel0,
                      double dt, double *ax, double *ay, double *axn, double *ayn, double *bxn, double *byn,
                      double *Fdc_x, double *Fdc_y) {
  const kid_params *p = c->p; const ko_grid *g = c->g;
  const double pi_180 = p->pi / 180.;
  const double scaling = 0.5, Cr0 = 0.06;
  double u_star = *uvel0 + (*axn * (dt / 2.)), v_star = *vvel0 + (*ayn * (dt / 2.));
  if (c->mts_part == 1) {
    u_star = BF(KID_B_UVEL, k); v_star = BF(KID_B_VVEL, k);
    *uvel0 = BF(KID_B_UVEL, k); *vvel0 = BF(KID_B_VVEL, k);
    *uvel = BF(KID_B_UVEL, k); *vvel = BF(KID_B_VVEL, k);
  }
  *axn = 0.; *ayn = 0.; *bxn = 0.; *byn = 0.;
  ia_sum S; memset(&S, 0, sizeof(S));
  double uo = 0, vo = 0, ua = 0, va = 0, ui = 0, vi = 0, ssh_x = 0, ssh_y = 0, f_cori = 0, c_ocn = 0, c_atm = 0, c_ice = 0, c_gnd = 0;
  double wave_rad = 0, uwave = 0, vwave = 0;
  const int ia_on = p->interactive_icebergs_on;
  if (!c->only_interactive) {
    uo = BF(KID_B_UO, k); vo = BF(KID_B_VO, k); ua = BF(KID_B_UA, k); va = BF(KID_B_VA, k); ui = BF(KID_B_UI, k); vi = BF(KID_B_VI, k);
    ssh_x = BF(KID_B_SSH_X, k); ssh_y = BF(KID_B_SSH_Y, k);
    double hi = BF(KID_B_HI, k); const double od = BF(KID_B_OD, k);
    if (g->d.grid_is_latlon && !p->use_f_plane) f_cori = (2. * p->omega) * sin(pi_180 * lat);
    else f_cori = (2. * p->omega) * sin(pi_180 * p->lat_ref);
    const double M = BF(KID_B_MASS, k), T = BF(KID_B_THICKNESS, k);
    const double D = (p->rho_bergs / RHO_SEAWATER) * T, F = T - D;
    const double W = BF(KID_B_WIDTH, k), L = BF(KID_B_LENGTH, k);
    hi = dmin(hi, D);
    const double D_hi = dmax(0., D - hi);
    double L2, W2;
    if (p->dem && p->hexagonal_icebergs && p->radius_based_drag) { L2 = 2. * sqrt(L * W / (2. * sqrt(3.))); W2 = L2; }
    else { L2 = L; W2 = W; }
    double groundfrac;
    if (p->h_to_init_grounding > 0.0) { groundfrac = 1.0 - (od - D) / p->h_to_init_grounding; groundfrac = dmax(groundfrac, 0.0); groundfrac = dmin(groundfrac, 1.0); }
    else groundfrac = (D > od) ? 1.0 : 0.0;
    c_gnd = (groundfrac > 0.0) ? (p->cdrag_grounding * W * L * groundfrac) / M : 0.0;
    if (p->short_step_mts_grounding) c_gnd = 0.;
    uwave = ua - uo; vwave = va - vo;
    double wmod = uwave * uwave + vwave * vwave;
    const double ampl = 0.5 * 0.02025 * wmod, Lwavelength = 0.32 * wmod, Lcutoff = 0.125 * Lwavelength, Ltop = 0.25 * Lwavelength;
    const double Cr = Cr0 * dmin(dmax(0., (L2 - Lcutoff) / ((Ltop - Lcutoff) + 1.e-30)), 1.);
    wave_rad = 0.5 * RHO_SEAWATER / M * Cr * GRAVITY * ampl * dmin(ampl, F) * (2. * W2 * L2) / (W2 + L2);
    wmod = sqrt(ua * ua + va * va);
    if (wmod != 0.) { uwave = ua / wmod; vwave = va / wmod; } else { uwave = 0.; vwave = 0.; wave_rad = 0.; }
    double dragfrac = 1.0;
    if (p->iceberg_bonds_on && p->internal_bergs_for_drag) {
      double N_bonds = 0., N_max = 4.0;
      if (p->hexagonal_icebergs) N_max = 6.0;
      for (int s = 0; s < c->bd->count[k]; ++s) {
        if (p->dem) { if (c->bd->broken[BS(s, k)] != 1) N_bonds = N_bonds + 1.0; } else N_bonds = N_bonds + 1.0;
      }
      dragfrac = ((N_max - N_bonds) / N_max);
    }
    c_ocn = RHO_SEAWATER / M * p->ocean_drag_scale * (0.5 * CD_WV * dragfrac * W2 * (D_hi) + CD_WH * W * L);
    c_atm = RHO_AIR / M * (0.5 * CD_AV * dragfrac * W2 * F + CD_AH * W * L);
    if (fabs(hi) == 0.) c_ice = 0.; else c_ice = RHO_ICE / M * (0.5 * CD_IV * dragfrac * W2 * hi);
    if (fabs(ui) + fabs(vi) == 0.) c_ice = 0.;
    *axn = -GRAVITY * ssh_x + wave_rad * uwave; *ayn = -GRAVITY * ssh_y + wave_rad * vwave;
    if (ia_on) { interactive_force(c, k, &S, *uvel0, *vvel0, *uvel0, *vvel0); *axn = *axn + S.IA_x; *ayn = *ayn + S.IA_y; }
    *axn = *axn + f_cori * v_star; *ayn = *ayn - f_cori * u_star;
  } else {
    if (ia_on) interactive_force(c, k, &S, *uvel0, *vvel0, *uvel0, *vvel0);
  }
  double uveln = *uvel0, vveln = *vvel0, us, vs;
  double RHS_x = 0, RHS_y = 0, A11 = 1, A12 = 0, A21 = 0, A22 = 1;
  for (int itloop = 1; itloop <= 2; ++itloop) {
    if (itloop == 2) { us = uveln; vs = vveln; } else { us = *uvel0; vs = *vvel0; }
    if (c->only_interactive) {
      if (ia_on) {
        if (itloop > 1) interactive_force(c, k, &S, *uvel0, *vvel0, us, vs);
        RHS_x = (S.IA_x / 2) - scaling * (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
        RHS_y = (S.IA_y / 2) - scaling * (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
        A11 = 1 + (scaling * dt * S.P11); A22 = 1 + (scaling * dt * S.P22);
        A12 = (scaling * dt * S.P12); A21 = (scaling * dt * S.P21);
      }
    } else {
      const double drag_ocn = c_ocn * 0.5 * (sqrt((uveln - uo) * (uveln - uo) + (vveln - vo) * (vveln - vo)) + sqrt((*uvel0 - uo) * (*uvel0 - uo) + (*vvel0 - vo) * (*vvel0 - vo)));
      const double drag_atm = c_atm * 0.5 * (sqrt((uveln - ua) * (uveln - ua) + (vveln - va) * (vveln - va)) + sqrt((*uvel0 - ua) * (*uvel0 - ua) + (*vvel0 - va) * (*vvel0 - va)));
      const double drag_ice = c_ice * 0.5 * (sqrt((uveln - ui) * (uveln - ui) + (vveln - vi) * (vveln - vi)) + sqrt((*uvel0 - ui) * (*uvel0 - ui) + (*vvel0 - vi) * (*vvel0 - vi)));
      const double drag_gnd = c_gnd;
      RHS_x = (*axn / 2) + scaling * (-drag_ocn * (u_star - uo) - drag_atm * (u_star - ua) - drag_ice * (u_star - ui) - drag_gnd * u_star);
      RHS_y = (*ayn / 2) + scaling * (-drag_ocn * (v_star - vo) - drag_atm * (v_star - va) - drag_ice * (v_star - vi) - drag_gnd * v_star);
      if (ia_on) {
        if (itloop > 1) interactive_force(c, k, &S, *uvel0, *vvel0, us, vs);
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
    *ax = detA * (A22 * RHS_x - A12 * RHS_y); *ay = detA * (A11 * RHS_y - A21 * RHS_x);
    uveln = u_star + dt * *ax; vveln = v_star + dt * *ay;
  }
  if (c->only_interactive) { *axn = S.IA_x; *ayn = S.IA_y; }
  else {
    *axn = -GRAVITY * ssh_x + wave_rad * uwave; *ayn = -GRAVITY * ssh_y + wave_rad * vwave;
    if (ia_on) { *axn = *axn + S.IA_x; *ayn = *ayn + S.IA_y; }
    *axn = *axn + f_cori * vveln; *ayn = *ayn - f_cori * uveln;
  }
  *bxn = 2 * *ax - *axn; *byn = 2 * *ay - *ayn;
  if (c->mts_part == 1 && Fdc_x && Fdc_y) {
    *Fdc_x = BF(KID_B_MASS, k) * (S.Ptu_x - (S.P11 * uveln + S.P12 * vveln));
    *Fdc_y = BF(KID_B_MASS, k) * (S.Ptu_y - (S.P21 * uveln + S.P22 * vveln));
  }
  speed_limit(c, i, j, dt, &uveln, &vveln);
  if (p->override_iceberg_velocities) { *ax = 0.; *ay = 0.; *axn = 0.; *ayn = 0.; *bxn = 0.; *byn = 0.; }
}

/* IB:1710-1947 */
static void accel_explicit_inner_mts(mts_ctx *c, int64_t k, int i, int j, double uvel0, double vvel0, double dt,
                                     double *ax, double *ay, double *axn, double *ayn) {
  const kid_params *p = c->p; const ko_grid *g = c->g;
  const double u_star = uvel0 + (*axn * (dt / 2.)), v_star = vvel0 + (*ayn * (dt / 2.));
  *axn = 0.; *ayn = 0.;
  double bxn = 0., byn = 0., IA_x = 0., IA_y = 0., IAd_x = 0., IAd_y = 0.;
  dem_sum D; memset(&D, 0, sizeof(D));
  if (p->iceberg_bonds_on) {
    for (int s = 0; s < c->bd->count[k]; ++s) {
      int matched = 0;
      const int64_t o = c->other_row[BS(s, k)];
      if (p->dem && c->mark[BS(s, k)]) {
        c->mark[BS(s, k)] = 0;
        matched = 1;
        D.F_x += BD(KID_BOND_F_X, s, k); D.F_y += BD(KID_BOND_F_Y, s, k);
        D.Fd_x += BD(KID_BOND_FD_X, s, k); D.Fd_y += BD(KID_BOND_FD_Y, s, k);
        D.T += BD(KID_BOND_T, s, k); D.T_d += BD(KID_BOND_T_D, s, k);
      }
      if (!matched) {
        if (o < 0) { c->scalars[KID_S_ERROR_COUNT] += 1.; continue; } /* FATAL IB:1783 */
        if (p->dem) {
          if (c->bd->broken[BS(s, k)] == 1) unbonded_same_conglom_dem_force(c, k, o, &IA_x, &IA_y, &IAd_x, &IAd_y, uvel0, vvel0, uvel0, vvel0);
          else calculate_force_dem(c, k, s, dt, &D);
        } else {
          ia_sum S; memset(&S, 0, sizeof(S));
          calculate_force(c, k, o, &S, uvel0, vvel0, uvel0, vvel0, 1, -1);
          IA_x += S.IA_x; IA_y += S.IA_y;
          const double du = BF(KID_B_UVEL_OLD, o) - BF(KID_B_UVEL_OLD, k), dv = BF(KID_B_VVEL_OLD, o) - BF(KID_B_VVEL_OLD, k);
          IAd_x = IAd_x + S.P11 * du + S.P12 * dv;
          IAd_y = IAd_y + S.P12 * du + S.P22 * dv;
        }
      }
    }
    int run_contact;
    if (p->iceberg_bonds_on && p->dem) run_contact = !((BI(KID_BI_N_BONDS, k) == p->max_bonds) || p->use_broken_bonds_for_substep_contact);
    else run_contact = 1;
    if (run_contact) {
      const int ine = BI(KID_BI_INE, k), jne = BI(KID_BI_JNE, k);
      const int j0 = jne - 1 > g->d.jsd + 1 ? jne - 1 : g->d.jsd + 1, j1 = jne + 1 < g->d.jed ? jne + 1 : g->d.jed;
      const int i0 = ine - 1 > g->d.isd + 1 ? ine - 1 : g->d.isd + 1, i1 = ine + 1 < g->d.ied ? ine + 1 : g->d.ied;
      for (int gj = j0; gj <= j1; ++gj) for (int gi = i0; gi <= i1; ++gi)
        for (int64_t q = c->cell_start[GIDX(g, gi, gj)]; q < c->cell_start[GIDX(g, gi, gj) + 1]; ++q) {
          const int64_t o = c->perm[q];
          /* `other_berg%id>0`: bond partners carry the negated-id mark unless use_broken_bonds_for_substep_contact */
          const int unmarked = p->use_broken_bonds_for_substep_contact ? 1 : !is_partner(c, k, o);
          if (unmarked && BI(KID_BI_CONGLOM_ID, o) == BI(KID_BI_CONGLOM_ID, k) && BI(KID_BI_N_BONDS, o) < p->max_bonds) {
            if (p->dem) unbonded_same_conglom_dem_force(c, k, o, &IA_x, &IA_y, &IAd_x, &IAd_y, uvel0, vvel0, uvel0, vvel0);
            else {
              ia_sum S; memset(&S, 0, sizeof(S));
              calculate_force(c, k, o, &S, uvel0, vvel0, uvel0, vvel0, 0, 1);
              IA_x += S.IA_x; IA_y += S.IA_y;
              const double du = BF(KID_B_UVEL_OLD, o) - BF(KID_B_UVEL_OLD, k), dv = BF(KID_B_VVEL_OLD, o) - BF(KID_B_VVEL_OLD, k);
              IAd_x = IAd_x + S.P11 * du + S.P12 * dv;
              IAd_y = IAd_y + S.P12 * du + S.P22 * dv;
            }
          }
        }
    }
  }
  if (p->dem) {
    if (p->dem_beam_test > 0) {  /* IB:1861-1877: the loads of the beam tests of Wang (2020), sections 3.1 and 3.2 */
      const double sl = BF(KID_B_START_LON, k);
      if (p->dem_beam_test == 1) {        /* simply supported beam: no vertical load on the ends, a point load at the centre */
        if (sl == p->dem_tests_start_lon || sl == p->dem_tests_end_lon) { D.F_y = 0.0; D.Fd_y = 0.0; }
        else if (sl == 0.5 * (p->dem_tests_start_lon + p->dem_tests_end_lon)) D.F_y = D.F_y - 1.5e5;
      } else if (p->dem_beam_test == 2) { /* cantilever beam: the load on the free end */
        if (sl == p->dem_tests_end_lon) D.F_y = D.F_y - 1.5e10 / 3.;
      }
    }
    double M, R1;
    if (p->constant_interaction_LW) {
      M = p->constant_length * p->constant_width * BF(KID_B_THICKNESS, k) * p->rho_bergs;
      R1 = radius_of(p, p->constant_length * p->constant_width);
    } else {
      M = BF(KID_B_MASS, k);
      R1 = radius_of(p, BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k));
    }
    IA_x = IA_x + D.F_x / M; IA_y = IA_y + D.F_y / M;
    IAd_x = IAd_x + D.Fd_x / M; IAd_y = IAd_y + D.Fd_y / M;
    BF(KID_B_ANG_ACCEL, k) = (D.T + D.T_d) / (0.5 * M * pow(R1, 2.));
  }
  *axn = IA_x + IAd_x; *ayn = IA_y + IAd_y;
  *ax = 0.5 * (*axn + bxn); *ay = 0.5 * (*ayn + byn);
  double uveln = u_star + dt * *ax, vveln = v_star + dt * *ay;
  speed_limit(c, i, j, dt, &uveln, &vveln);
  if (p->override_iceberg_velocities) { *ax = 0.; *ay = 0.; *axn = 0.; *ayn = 0.; }
}

/* FW:4713-4799 */
static void break_bonds_dem(mts_ctx *c) {
  const kid_params *p = c->p;
  double tn = p->frac_thres_n, tt = p->frac_thres_t;
  if (tn <= 0.0 && tt <= 0.0) return;
  if (tn <= 0.0) tn = HUGE_VAL;
  if (tt <= 0.0) tt = HUGE_VAL;
  if (!p->fracture_criterion_stress) { c->scalars[KID_S_ERROR_COUNT] += 1.; return; }
  /* pass 1: mark (other_id = -1 in the reference; here `broken = 2`), both sides */
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    for (int s = 0; s < c->bd->count[k]; ++s) {
      if (c->bd->broken[BS(s, k)] == 2) continue;
      if (BD(KID_BOND_NSTRESS, s, k) > tn || BD(KID_BOND_SSTRESS, s, k) > tt) {
        c->bd->broken[BS(s, k)] = 2;
        const int64_t o = c->other_row[BS(s, k)]; const int so = c->other_slot[BS(s, k)];
        if (o >= 0 && so >= 0) c->bd->broken[BS(so, o)] = 2;
      }
    }
  }
  /* pass 2: delete the marked bonds, keeping list order */
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    int w = 0;
    const int cnt = c->bd->count[k];
    for (int s = 0; s < cnt; ++s) {
      if (c->bd->broken[BS(s, k)] == 2) { BI(KID_BI_N_BONDS, k) = BI(KID_BI_N_BONDS, k) - 1; c->scalars[KID_S_NBONDS_BROKEN] += 1.; continue; }
      if (w != s) {
        c->bd->other_id[BS(w, k)] = c->bd->other_id[BS(s, k)]; c->bd->broken[BS(w, k)] = c->bd->broken[BS(s, k)];
        for (int f = 0; f < KID_NBOND_F64; ++f) BD(f, w, k) = BD(f, s, k);
        c->other_row[BS(w, k)] = c->other_row[BS(s, k)]; c->mark[BS(w, k)] = c->mark[BS(s, k)];
      }
      ++w;
    }
    c->bd->count[k] = w;
  }
  /* the matching-bond slots moved */
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    for (int s = 0; s < c->bd->count[k]; ++s) {
      const int64_t o = c->other_row[BS(s, k)];
      c->other_slot[BS(s, k)] = -1;
      if (o < 0) continue;
      for (int t = 0; t < c->bd->count[o]; ++t) if (c->bd->other_id[BS(t, o)] == c->b->id[k]) { c->other_slot[BS(s, k)] = t; break; }
    }
  }
}

/* grounding drag factor used on the sub-steps, IB:6880-6906 / 6983-7028 */
static double groundfrac_of(const kid_params *p, double od, double thickness) {
  const double D = (p->rho_bergs / RHO_SEAWATER) * thickness;
  double gf;
  if (p->h_to_init_grounding > 0.0) { gf = 1.0 - (od - D) / p->h_to_init_grounding; gf = dmax(gf, 0.0); gf = dmin(gf, 1.0); }
  else gf = (D > od) ? 1.0 : 0.0;
  return gf;
}

/* IB:6576-7078 */
void ko_evolve_icebergs_mts(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars) {
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, scalars);
  c->only_interactive = p->only_interactive_forces;
  /* PART 1 */
  c->mts_part = 1;
  double dt = p->dt, dt_2 = 0.5 * dt;
  int ii = 0, finished = 0, had_collision = 0, last_iter = p->force_convergence ? 0 : 1;
  double usum = 0., usum1 = 0., usum2 = 0.;
  while (!finished) {
    ii = ii + 1;
    for (int64_t q = 0; q < c->nperm; ++q) {
      const int64_t k = c->perm[q];
      if (BF(KID_B_STATIC_BERG, k) < 0.5 && (BI(KID_BI_CONGLOM_ID, k) != 0 || p->force_convergence)) {
        if (ii == 1 || BF(KID_B_STATIC_BERG, k) == 0.1) {
          double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k), u0 = uvel1, v0 = vvel1;
          double axn = 0., ayn = 0., bxn = 0., byn = 0., ax1, ay1, Fdc_x = 0., Fdc_y = 0.;
          accel_mts(c, k, BI(KID_BI_INE, k), BI(KID_BI_JNE, k), BF(KID_B_LAT, k), &uvel1, &vvel1, &u0, &v0, dt, &ax1, &ay1,
                    &axn, &ayn, &bxn, &byn, &Fdc_x, &Fdc_y);
          if (Fdc_x != 0. || (Fdc_y != 0. && p->force_convergence)) { had_collision = 1; BF(KID_B_STATIC_BERG, k) = 0.1; }
          BF(KID_B_AXN, k) = axn; BF(KID_B_AYN, k) = ayn; BF(KID_B_BXN, k) = bxn; BF(KID_B_BYN, k) = byn;
          if (p->force_convergence) {
            BF(KID_B_UVEL_PREV, k) = BF(KID_B_UVEL, k) + (dt * ax1); BF(KID_B_VVEL_PREV, k) = BF(KID_B_VVEL, k) + (dt * ay1);
            if (ii == 1) usum = usum + pow(BF(KID_B_UVEL_OLD, k), 2.) + pow(BF(KID_B_VVEL_OLD, k), 2.);
            usum1 = usum1 + pow(BF(KID_B_UVEL_PREV, k), 2.) + pow(BF(KID_B_VVEL_PREV, k), 2.);
            usum2 = usum2 + pow(BF(KID_B_UVEL_PREV, k) - BF(KID_B_UVEL_OLD, k), 2.) + pow(BF(KID_B_VVEL_PREV, k) - BF(KID_B_VVEL_OLD, k), 2.);
          } else {
            BF(KID_B_UVEL, k) = BF(KID_B_UVEL, k) + (dt * ax1); BF(KID_B_VVEL, k) = BF(KID_B_VVEL, k) + (dt * ay1);
            BF(KID_B_UVEL_PREV, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_PREV, k) = BF(KID_B_VVEL, k);
          }
        }
      }
    }
    if (p->force_convergence)
      for (int64_t q = 0; q < c->nperm; ++q) {
        const int64_t k = c->perm[q];
        if (BF(KID_B_STATIC_BERG, k) < 0.5) {
          BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL_PREV, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL_PREV, k);
          if (last_iter && BF(KID_B_STATIC_BERG, k) == 0.1) BF(KID_B_STATIC_BERG, k) = 0.;
        }
      }
    if (p->force_convergence && !last_iter && had_collision) {
      if (ii > 1) {
        const double denom = sqrt(usum) + sqrt(usum1);
        const double normchange = denom > 0 ? 2.0 * sqrt(usum2) / denom : 0.0;
        if (normchange < p->convergence_tolerance) last_iter = 1;
      }
      usum = usum1;
    } else finished = 1;
    if (last_iter) finished = 1;
    usum1 = 0.; usum2 = 0.;
    if (ii > 1000) finished = 1; /* guard; the reference has none */
  }
  if (p->dem && !p->break_bonds_on_sub_steps) break_bonds_dem(c);
  /* PART 2 */
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    if (BF(KID_B_STATIC_BERG, k) < 0.5 && BI(KID_BI_CONGLOM_ID, k) != 0) {
      BF(KID_B_UVEL, k) = BF(KID_B_UVEL_PREV, k); BF(KID_B_VVEL, k) = BF(KID_B_VVEL_PREV, k);
      BF(KID_B_UVEL, k) = BF(KID_B_UVEL, k) + dt_2 * (BF(KID_B_AXN, k) + BF(KID_B_BXN, k));
      BF(KID_B_VVEL, k) = BF(KID_B_VVEL, k) + dt_2 * (BF(KID_B_AYN, k) + BF(KID_B_BYN, k));
      BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
      if (p->force_convergence) {
        BF(KID_B_AXN, k) = BF(KID_B_AXN_FAST, k); BF(KID_B_AYN, k) = BF(KID_B_AYN_FAST, k);
        BF(KID_B_BXN, k) = BF(KID_B_BXN_FAST, k); BF(KID_B_BYN, k) = BF(KID_B_BYN_FAST, k);
      }
    }
  }
  /* PART 3 */
  c->only_interactive = 1;
  c->mts_part = 3;
  dt = c->mts_fast_dt; dt_2 = 0.5 * dt;
  for (int sub = 1; sub <= p->mts_sub_steps; ++sub) {
    for (int64_t q = 0; q < c->nperm; ++q) { /* positions */
      const int64_t k = c->perm[q];
      if (!(BF(KID_B_STATIC_BERG, k) < 0.5 && BI(KID_BI_CONGLOM_ID, k) != 0)) continue;
      const int on_tang = (BF(KID_B_LAT, k) > 89.) && g->d.grid_is_latlon;
      const double lon1 = BF(KID_B_LON, k), lat1 = BF(KID_B_LAT, k);
      double x1 = 0, y1 = 0, dxdl1, dydl;
      if (on_tang) ko_rotpos_to_tang(p, lon1, lat1, &x1, &y1);
      ko_meters_to_grid(g, p, lat1, &dxdl1, &dydl);
      const double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k);
      const double axn = BF(KID_B_AXN_FAST, k), ayn = BF(KID_B_AYN_FAST, k), bxn = BF(KID_B_BXN_FAST, k), byn = BF(KID_B_BYN_FAST, k);
      const double uvel2 = uvel1 + (dt_2 * axn) + (dt_2 * bxn), vvel2 = vvel1 + (dt_2 * ayn) + (dt_2 * byn);
      double xdot2 = 0, ydot2 = 0, lonn, latn;
      if (on_tang) ko_rotvec_to_tang(p, lon1, uvel2, vvel2, &xdot2, &ydot2);
      const double u2 = uvel2 * dxdl1, v2 = vvel2 * dydl;
      if (on_tang) { const double xn = x1 + (dt * xdot2), yn = y1 + (dt * ydot2); ko_rotpos_from_tang(p, xn, yn, &lonn, &latn); }
      else { lonn = lon1 + (dt * u2); latn = lat1 + (dt * v2); }
      BF(KID_B_LON, k) = lonn; BF(KID_B_LAT, k) = latn; BF(KID_B_LON_OLD, k) = lonn; BF(KID_B_LAT_OLD, k) = latn;
      BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k) + dt_2 * (BF(KID_B_AXN_FAST, k) + BF(KID_B_BXN_FAST, k));
      BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k) + dt_2 * (BF(KID_B_AYN_FAST, k) + BF(KID_B_BXN_FAST, k)); /* sic: bxn_fast, IB:6831 */
    }
    int jj = 0;
    usum = 0.; usum1 = 0.; usum2 = 0.;
    finished = 0;
    last_iter = (p->force_convergence && !p->explicit_inner_mts) ? 0 : 1;
    while (!finished) {
      jj = jj + 1;
      c->bond_break_detected = 0;
      for (int64_t q = 0; q < c->nperm; ++q) { /* velocities */
        const int64_t k = c->perm[q];
        if (!(BF(KID_B_STATIC_BERG, k) < 0.5 && BI(KID_BI_CONGLOM_ID, k) != 0)) continue;
        const double latn = BF(KID_B_LAT, k), lonn = BF(KID_B_LON, k);
        double axn = BF(KID_B_AXN_FAST, k), ayn = BF(KID_B_AYN_FAST, k), bxn = BF(KID_B_BXN_FAST, k), byn = BF(KID_B_BYN_FAST, k);
        double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k);
        const int i = BI(KID_BI_INE, k), j = BI(KID_BI_JNE, k);
        axn = axn + bxn; ayn = ayn + byn;
        const double uvel3 = uvel1 + (dt_2 * axn), vvel3 = vvel1 + (dt_2 * ayn);
        double ax1, ay1;
        if (p->explicit_inner_mts) {
          accel_explicit_inner_mts(c, k, i, j, uvel1, vvel1, dt, &ax1, &ay1, &axn, &ayn);
          bxn = 0.; byn = 0.;
          if (p->short_step_mts_grounding) {
            const double gf = groundfrac_of(p, BF(KID_B_OD, k), BF(KID_B_THICKNESS, k));
            double gdrag = 0.;
            if (gf > 0.0) {
              double MM, AA;
              if (p->constant_interaction_LW) { MM = p->constant_length * p->constant_width * BF(KID_B_THICKNESS, k) * p->rho_bergs; AA = p->constant_width * p->constant_length; }
              else { MM = BF(KID_B_MASS, k); AA = BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k); }
              gdrag = -p->cdrag_grounding * gf * AA / MM;
            }
            axn = axn + uvel1 * gdrag; ayn = ayn + vvel1 * gdrag;
            ax1 = 0.5 * axn; ay1 = 0.5 * ayn;
          }
        } else {
          double u0 = uvel1, v0 = vvel1;
          accel_mts(c, k, i, j, latn, &uvel1, &vvel1, &u0, &v0, dt, &ax1, &ay1, &axn, &ayn, &bxn, &byn, NULL, NULL);
        }
        double uveln, vveln;
        const int on_tang = (BF(KID_B_LAT, k) > 89.) && g->d.grid_is_latlon;
        if (on_tang) {
          double xdot3, ydot3, xddot1, yddot1;
          ko_rotvec_to_tang(p, lonn, uvel3, vvel3, &xdot3, &ydot3);
          ko_rotvec_to_tang(p, lonn, ax1, ay1, &xddot1, &yddot1);
          const double xdotn = xdot3 + (dt * xddot1), ydotn = ydot3 + (dt * yddot1);
          ko_rotvec_from_tang(p, lonn, xdotn, ydotn, &uveln, &vveln);
        } else { uveln = uvel3 + (dt * ax1); vveln = vvel3 + (dt * ay1); }
        if (p->force_convergence && !p->explicit_inner_mts) {
          if (jj == 1) usum = usum + pow(BF(KID_B_UVEL_OLD, k), 2.) + pow(BF(KID_B_VVEL_OLD, k), 2.);
          usum1 = usum1 + pow(uveln, 2.) + pow(vveln, 2.);
          usum2 = usum2 + pow(uveln - BF(KID_B_UVEL_OLD, k), 2.) + pow(vveln - BF(KID_B_VVEL_OLD, k), 2.);
        }
        BF(KID_B_AXN_FAST, k) = axn; BF(KID_B_AYN_FAST, k) = ayn; BF(KID_B_BXN_FAST, k) = bxn; BF(KID_B_BYN_FAST, k) = byn;
        BF(KID_B_UVEL, k) = uveln; BF(KID_B_VVEL, k) = vveln;
      }
      if (p->force_convergence && !last_iter) {
        if (jj > 1) {
          const double denom = sqrt(usum) + sqrt(usum1);
          const double normchange = denom > 0 ? 2.0 * sqrt(usum2) / denom : 0.0;
          if (normchange < p->convergence_tolerance) last_iter = 1;
        }
        usum = usum1;
      } else finished = 1;
      if (last_iter) finished = 1;
      if (jj > 1000) finished = 1; /* guard; the reference has none */
      if (p->force_convergence && !finished)
        for (int64_t q = 0; q < c->nperm; ++q) {
          const int64_t k = c->perm[q];
          if (!(BF(KID_B_STATIC_BERG, k) < 0.5 && BI(KID_BI_CONGLOM_ID, k) != 0)) continue;
          BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
          BF(KID_B_UVEL, k) = BF(KID_B_UVEL, k) - dt_2 * (BF(KID_B_AXN_FAST, k) + BF(KID_B_BXN_FAST, k)) - dt_2 * (BF(KID_B_AXN, k) + BF(KID_B_BXN, k));
          BF(KID_B_VVEL, k) = BF(KID_B_VVEL, k) - dt_2 * (BF(KID_B_AYN_FAST, k) + BF(KID_B_BYN_FAST, k)) - dt_2 * (BF(KID_B_AYN, k) + BF(KID_B_BYN, k));
          BF(KID_B_AXN_FAST, k) = BF(KID_B_AXN, k); BF(KID_B_AYN_FAST, k) = BF(KID_B_AYN, k);
          BF(KID_B_BXN_FAST, k) = BF(KID_B_BXN, k); BF(KID_B_BYN_FAST, k) = BF(KID_B_BYN, k);
        }
      usum1 = 0.; usum2 = 0.;
    }
    for (int64_t q = 0; q < c->nperm; ++q) { /* 'old' velocities, rotation */
      const int64_t k = c->perm[q];
      if (!(BF(KID_B_STATIC_BERG, k) < 0.5 && BI(KID_BI_CONGLOM_ID, k) != 0)) continue;
      BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
      double gdrag = 0.;
      if (p->use_grounding_torque) {
        const double gf = groundfrac_of(p, BF(KID_B_OD, k), BF(KID_B_THICKNESS, k));
        if (gf > 0.0) {
          double MM, R1;
          if (p->constant_interaction_LW) { MM = p->constant_length * p->constant_width * BF(KID_B_THICKNESS, k) * p->rho_bergs; R1 = radius_of(p, p->constant_length * p->constant_width); }
          else { MM = BF(KID_B_MASS, k); R1 = radius_of(p, BF(KID_B_LENGTH, k) * BF(KID_B_WIDTH, k)); }
          gdrag = -p->cdrag_grounding * gf * p->pi * pow(R1, 2.) / MM;
        }
      }
      if (p->dem) {
        BF(KID_B_ANG_VEL, k) = BF(KID_B_ANG_VEL, k) + dt * BF(KID_B_ANG_ACCEL, k);
        BF(KID_B_ANG_VEL, k) = BF(KID_B_ANG_VEL, k) / (1. - gdrag * dt);
        BF(KID_B_ROT, k) = BF(KID_B_ROT, k) + dt * BF(KID_B_ANG_VEL, k);
      }
      if (p->force_convergence) {
        BF(KID_B_AXN, k) = BF(KID_B_AXN_FAST, k); BF(KID_B_AYN, k) = BF(KID_B_AYN_FAST, k);
        BF(KID_B_BXN, k) = BF(KID_B_BXN_FAST, k); BF(KID_B_BYN, k) = BF(KID_B_BYN_FAST, k);
      }
    }
    if (p->dem && !p->use_broken_bonds_for_substep_contact)
      if (p->break_bonds_on_sub_steps && c->bond_break_detected) break_bonds_dem(c);
  }
  /* indices */
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    if (BF(KID_B_STATIC_BERG, k) < 0.5 && BF(KID_B_HALO_BERG, k) < 1) {
      BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
      double lonn = BF(KID_B_LON, k), latn = BF(KID_B_LAT, k), xi = BF(KID_B_XI, k), yj = BF(KID_B_YJ, k);
      int i = BI(KID_BI_INE, k), j = BI(KID_BI_JNE, k), bounced = 0, err = 0;
      ko_adjust_index_and_ground(g, p, &lonn, &latn, &i, &j, &xi, &yj, &bounced, &err);
      if (err) scalars[KID_S_ERROR_COUNT] += 1.;
      BF(KID_B_LON, k) = lonn; BF(KID_B_LAT, k) = latn; BF(KID_B_LON_OLD, k) = lonn; BF(KID_B_LAT_OLD, k) = latn;
      BI(KID_BI_INE, k) = i; BI(KID_BI_JNE, k) = j; BF(KID_B_XI, k) = xi; BF(KID_B_YJ, k) = yj;
      if (i < g->d.isc || i > g->d.iec || j < g->d.jsc || j > g->d.jec) BI(KID_BI_ALIVE, k) = 0; /* leaves the PE, FW:3024-3041 */
    }
  }
  ctx_free(c);
}

/* ---- the single-time-step scheme with interacting bergs (interactive_icebergs_on, mts=.false.) ------------------
 * accel IB:1950-2442 with the interactive terms; evolve_icebergs IB:7081-7200 (first sweep: velocities, second sweep:
 * update_verlet_position + the *_old copies the next step's interactive_force reads).  Verlet only. */
static void accel_sts_ia(mts_ctx *c, int64_t k, int i, int j, double xi, double yj, double lat, double uvel, double vvel,
                         double uvel0, double vvel0, double dt, double *ax, double *ay, double *axn, double *ayn, double *bxn, double *byn) {
  const kid_params *p = c->p; const ko_grid *g = c->g;
  const double pi_180 = p->pi / 180.;
  const double Cr0 = 0.06;
  const int RK = p->Runge_not_Verlet;
  const double alpha = RK ? 0.0 : 1.0, beta = 1.0, C_N = RK ? 0.0 : 1.0;
  const int new_pc = RK ? p->use_new_predictive_corrective : 1;
  const double u_star = uvel0 + (*axn * (dt / 2.)), v_star = vvel0 + (*ayn * (dt / 2.));
  double env[13];
  if (p->old_interp_flds_order) ko_interp_flds(g, p, BF(KID_B_LON, k), BF(KID_B_LAT, k), i, j, xi, yj, env);
  else for (int e = 0; e < 13; ++e) env[e] = BF(KID_B_UO + e, k);
  const double uo = env[0], vo = env[1], ui = env[2], vi = env[3], ua = env[4], va = env[5], ssh_x = env[6], ssh_y = env[7];
  double hi = env[11]; const double od = env[12];
  double f_cori;
  if (g->d.grid_is_latlon && !p->use_f_plane) f_cori = (2. * p->omega) * sin(pi_180 * lat);
  else f_cori = (2. * p->omega) * sin(pi_180 * p->lat_ref);
  const double M = BF(KID_B_MASS, k), T = BF(KID_B_THICKNESS, k);
  const double D = (p->rho_bergs / RHO_SEAWATER) * T, F = T - D;
  const double W = BF(KID_B_WIDTH, k), L = BF(KID_B_LENGTH, k);
  *axn = 0.; *ayn = 0.; *bxn = 0.; *byn = 0.;
  hi = dmin(hi, D);
  const double D_hi = dmax(0., D - hi);
  double groundfrac;
  if (p->h_to_init_grounding > 0.0) { groundfrac = 1.0 - (od - D) / p->h_to_init_grounding; groundfrac = dmax(groundfrac, 0.0); groundfrac = dmin(groundfrac, 1.0); }
  else groundfrac = (D > od) ? 1.0 : 0.0;
  const double c_gnd = (groundfrac > 0.0) ? (p->cdrag_grounding * W * L * groundfrac) / M : 0.0;
  double uwave = ua - uo, vwave = va - vo;
  double wmod = uwave * uwave + vwave * vwave;
  const double ampl = 0.5 * 0.02025 * wmod, Lwavelength = 0.32 * wmod, Lcutoff = 0.125 * Lwavelength, Ltop = 0.25 * Lwavelength;
  const double Cr = Cr0 * dmin(dmax(0., (L - Lcutoff) / ((Ltop - Lcutoff) + 1.e-30)), 1.);
  double wave_rad = 0.5 * RHO_SEAWATER / M * Cr * GRAVITY * ampl * dmin(ampl, F) * (2. * W * L) / (W + L);
  wmod = sqrt(ua * ua + va * va);
  if (wmod != 0.) { uwave = ua / wmod; vwave = va / wmod; } else { uwave = 0.; vwave = 0.; wave_rad = 0.; }
  double dragfrac = 1.0;
  if (p->iceberg_bonds_on && p->internal_bergs_for_drag) {
    double N_bonds = 0., N_max = 4.0;
    if (p->hexagonal_icebergs) N_max = 6.0;
    for (int s = 0; s < c->bd->count[k]; ++s) {
      if (p->dem) { if (c->bd->broken[BS(s, k)] != 1) N_bonds = N_bonds + 1.0; } else N_bonds = N_bonds + 1.0;
    }
    dragfrac = ((N_max - N_bonds) / N_max);
  }
  const double c_ocn = RHO_SEAWATER / M * p->ocean_drag_scale * (0.5 * CD_WV * dragfrac * W * (D_hi) + CD_WH * W * L);
  const double c_atm = RHO_AIR / M * (0.5 * CD_AV * dragfrac * W * F + CD_AH * W * L);
  double c_ice = (fabs(hi) == 0.) ? 0. : RHO_ICE / M * (0.5 * CD_IV * dragfrac * W * hi);
  if (fabs(ui) + fabs(vi) == 0.) c_ice = 0.;
  if (!RK) { *axn = -GRAVITY * ssh_x + wave_rad * uwave; *ayn = -GRAVITY * ssh_y + wave_rad * vwave; }
  else { *bxn = -GRAVITY * ssh_x + wave_rad * uwave; *byn = -GRAVITY * ssh_y + wave_rad * vwave; }
  ia_sum S; memset(&S, 0, sizeof(S));
  const int ia_on = p->interactive_icebergs_on;
  if (ia_on) {
    interactive_force(c, k, &S, uvel0, vvel0, uvel0, vvel0);
    if (!RK) { *axn = *axn + S.IA_x; *ayn = *ayn + S.IA_y; } else { *bxn = *bxn + S.IA_x; *byn = *byn + S.IA_y; }
  }
  if (alpha > 0.) {
    if (C_N > 0.) { *axn = *axn + f_cori * v_star; *ayn = *ayn - f_cori * u_star; }
    else { *bxn = *bxn + f_cori * v_star; *byn = *byn - f_cori * u_star; }
  } else { *bxn = *bxn + f_cori * vvel; *byn = *byn - f_cori * uvel; }
  double uveln = new_pc ? uvel0 : uvel, vveln = new_pc ? vvel0 : vvel;
  double us = uvel0, vs = vvel0;
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
    double RHS_x = (*axn / 2) + *bxn, RHS_y = (*ayn / 2) + *byn;
    if (beta > 0.) {
      RHS_x = RHS_x - drag_ocn * (u_star - uo) - drag_atm * (u_star - ua) - drag_ice * (u_star - ui) - drag_gnd * u_star;
      RHS_y = RHS_y - drag_ocn * (v_star - vo) - drag_atm * (v_star - va) - drag_ice * (v_star - vi) - drag_gnd * v_star;
    }
    if (ia_on) {
      if (itloop > 1) interactive_force(c, k, &S, uvel0, vvel0, us, vs);
      RHS_x = RHS_x - (((S.P11 * u_star) + (S.P12 * v_star)) - S.Ptu_x);
      RHS_y = RHS_y - (((S.P21 * u_star) + (S.P22 * v_star)) - S.Ptu_y);
    }
    double A11, A12, A21, A22;
    if (p->only_interactive_forces) {
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
    *ax = detA * (A22 * RHS_x - A12 * RHS_y); *ay = detA * (A11 * RHS_y - A21 * RHS_x);
    uveln = u_star + dt * *ax; vveln = v_star + dt * *ay;
  }
  if (p->only_interactive_forces) { *axn = S.IA_x; *ayn = S.IA_y; }
  else {
    *axn = 0.; *ayn = 0.;
    if (!RK) {
      *axn = -GRAVITY * ssh_x + wave_rad * uwave; *ayn = -GRAVITY * ssh_y + wave_rad * vwave;
      if (ia_on) { *axn = *axn + S.IA_x; *ayn = *ayn + S.IA_y; }
    }
    if (C_N > 0.) { *axn = *axn + f_cori * vveln; *ayn = *ayn - f_cori * uveln; }
  }
  *bxn = *ax - (*axn / 2); *byn = *ay - (*ayn / 2);
  speed_limit(c, i, j, dt, &uveln, &vveln);
  if (p->override_iceberg_velocities) { *ax = 0.; *ay = 0.; *axn = 0.; *ayn = 0.; *bxn = 0.; *byn = 0.; }
}

void ko_evolve_icebergs_interactive(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars) {
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, scalars);
  const double dt = p->dt, dt_2 = 0.5 * dt;
  for (int64_t q = 0; q < c->nperm; ++q) { /* first sweep: verlet_stepping IB:7203-7328 */
    const int64_t k = c->perm[q];
    if (!(BF(KID_B_STATIC_BERG, k) < 0.5)) continue;
    const double lonn = BF(KID_B_LON, k), latn = BF(KID_B_LAT, k);
    double axn = BF(KID_B_AXN, k), ayn = BF(KID_B_AYN, k), bxn = BF(KID_B_BXN, k), byn = BF(KID_B_BYN, k);
    const double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k);
    BF(KID_B_UVEL_PREV, k) = uvel1 - dt_2 * bxn; BF(KID_B_VVEL_PREV, k) = vvel1 - dt_2 * byn;
    const double uvel3 = uvel1 + (dt_2 * axn), vvel3 = vvel1 + (dt_2 * ayn);
    double ax1, ay1;
    accel_sts_ia(c, k, BI(KID_BI_INE, k), BI(KID_BI_JNE, k), BF(KID_B_XI, k), BF(KID_B_YJ, k), latn, uvel1, vvel1, uvel1, vvel1, dt,
                 &ax1, &ay1, &axn, &ayn, &bxn, &byn);
    double uveln, vveln;
    if ((latn > 89.) && g->d.grid_is_latlon) {
      double xdot3, ydot3, xddot1, yddot1;
      ko_rotvec_to_tang(p, lonn, uvel3, vvel3, &xdot3, &ydot3);
      ko_rotvec_to_tang(p, lonn, ax1, ay1, &xddot1, &yddot1);
      ko_rotvec_from_tang(p, lonn, xdot3 + (dt * xddot1), ydot3 + (dt * yddot1), &uveln, &vveln);
    } else { uveln = uvel3 + (dt * ax1); vveln = vvel3 + (dt * ay1); }
    if (p->override_iceberg_velocities) { uveln = p->u_override; vveln = p->v_override; }
    BF(KID_B_AXN, k) = axn; BF(KID_B_AYN, k) = ayn; BF(KID_B_BXN, k) = bxn; BF(KID_B_BYN, k) = byn;
    BF(KID_B_UVEL, k) = uveln; BF(KID_B_VVEL, k) = vveln;
  }
  for (int64_t q = 0; q < c->nperm; ++q) { /* second sweep IB:7180-7198: update_verlet_position IB:7684-7764 + *_old */
    const int64_t k = c->perm[q];
    if (!(BF(KID_B_STATIC_BERG, k) < 0.5)) continue;
    const int on_tang = (BF(KID_B_LAT, k) > 89.) && g->d.grid_is_latlon;
    const double lon1 = BF(KID_B_LON, k), lat1 = BF(KID_B_LAT, k);
    double x1 = 0, y1 = 0, dxdl1, dydl;
    if (on_tang) ko_rotpos_to_tang(p, lon1, lat1, &x1, &y1);
    ko_meters_to_grid(g, p, lat1, &dxdl1, &dydl);
    const double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k);
    const double axn = BF(KID_B_AXN, k), ayn = BF(KID_B_AYN, k), bxn = BF(KID_B_BXN, k), byn = BF(KID_B_BYN, k);
    const double uvel2 = uvel1 + (dt_2 * axn) + (dt_2 * bxn), vvel2 = vvel1 + (dt_2 * ayn) + (dt_2 * byn);
    double xdot2 = 0, ydot2 = 0, lonn, latn;
    if (on_tang) ko_rotvec_to_tang(p, lon1, uvel2, vvel2, &xdot2, &ydot2);
    const double u2 = uvel2 * dxdl1, v2 = vvel2 * dydl;
    if (on_tang) ko_rotpos_from_tang(p, x1 + (dt * xdot2), y1 + (dt * ydot2), &lonn, &latn);
    else { lonn = lon1 + (dt * u2); latn = lat1 + (dt * v2); }
    int i = BI(KID_BI_INE, k), j = BI(KID_BI_JNE, k), bounced = 0, err = 0;
    double xi = BF(KID_B_XI, k), yj = BF(KID_B_YJ, k);
    ko_adjust_index_and_ground(g, p, &lonn, &latn, &i, &j, &xi, &yj, &bounced, &err);
    if (err) scalars[KID_S_ERROR_COUNT] += 1.;
    BF(KID_B_LON, k) = lonn; BF(KID_B_LAT, k) = latn; BI(KID_BI_INE, k) = i; BI(KID_BI_JNE, k) = j; BF(KID_B_XI, k) = xi; BF(KID_B_YJ, k) = yj;
    BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
    BF(KID_B_LON_OLD, k) = lonn; BF(KID_B_LAT_OLD, k) = latn;
    if (i < g->d.isc || i > g->d.iec || j < g->d.jsc || j > g->d.jec) BI(KID_BI_ALIVE, k) = 0;
  }
  ctx_free(c);
}

/* find_orientation_using_iceberg_bonds IB:3829-3892 for every berg (the value is in radians and is then handed to
 * the hexagon code, which reads it as degrees -- as the reference does) */
void ko_find_orientations(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *orientation) {
  double dummy[KID_NSCALAR] = {0};
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, dummy);
  for (int64_t k = 0; k < b->n; ++k) orientation[k] = p->initial_orientation;
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    const int ine = BI(KID_BI_INE, k), jne = BI(KID_BI_JNE, k);
    if (!((ine > g->d.isd) && (ine < g->d.ied) && (jne >= g->d.jsd) && (jne <= g->d.jed))) continue;
    double bond_count = 0., Average_angle = 0.;
    const double lat1 = BF(KID_B_LAT, k), lon1 = BF(KID_B_LON, k);
    for (int s = 0; s < bd->count[k]; ++s) {
      const int64_t o = c->other_row[BS(s, k)];
      if (o < 0) continue;
      const double lat2 = BF(KID_B_LAT, o), lon2 = BF(KID_B_LON, o);
      const double dlat = lat2 - lat1, dlon = lon2 - lon1;
      double dx_dlon, dy_dlat; grid_to_meters(c, 0.5 * (lat1 + lat2), &dx_dlon, &dy_dlat);
      const double rx = dlon * dx_dlon, ry = dlat * dy_dlat;
      double angle;
      if (rx == 0.) angle = p->pi / 2.;
      else {
        angle = atan(ry / rx);
        angle = ((p->pi / 2.) - (orientation[k] * (p->pi / 180.))) - angle;
        angle = ko_modulo(angle, p->pi / 3.);
      }
      bond_count = bond_count + 1.;
      Average_angle = Average_angle + angle;
    }
    if (bond_count > 0) Average_angle = Average_angle / bond_count; else Average_angle = 0.;
    orientation[k] = ko_modulo(Average_angle, p->pi / 3.);
  }
  ctx_free(c);
}
static void gridded_with_orientation(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *acc, double *out) {
  double *orient = NULL;
  if (p->hexagonal_icebergs && p->iceberg_bonds_on && p->rotate_icebergs_for_mass_spreading && bd) {
    orient = (double *)malloc(sizeof(double) * (size_t)(b->n > 0 ? b->n : 1));
    ko_find_orientations(g, p, b, bd, orient);
    ko_set_orientation(orient);
  }
  ko_create_gridded_icebergs_fields(g, p, b, acc, out);
  ko_set_orientation(NULL);
  free(orient);
}

/* icebergs_run with interacting bergs under the single-time-step scheme (IB:5409-5512) */
void ko_run_step_interactive(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, int first_visit,
                             double *acc, double *out, double *scalars) {
  const size_t ncell = (size_t)NI(g) * (size_t)NJ(g);
  const int contact = (p->contact_distance > 0.) || (p->contact_spring_coef != p->spring_coef);
  memset(acc, 0, (size_t)KID_NACC * ncell * sizeof(double));
  if (first_visit) {
    if (contact) ko_set_conglom_ids(g, p, b, bd);                       /* IB:5415-5416 */
    if (p->iceberg_bonds_on && bd) ko_orig_bond_length(g, p, b, bd);    /* IB:5418 */
  }
  if (!p->old_interp_flds_order) ko_interp_gridded_fields_to_bergs(g, p, b);
  if (!p->static_icebergs) ko_evolve_icebergs_interactive(g, p, b, bd, scalars);
  if (contact) ko_set_conglom_ids(g, p, b, bd);                         /* IB:5470-5471 */
  if (!p->old_interp_flds_order) ko_interp_gridded_fields_to_bergs(g, p, b);
  ko_thermodynamics(g, p, b, acc, scalars);
  gridded_with_orientation(g, p, b, bd, acc, out);
  int64_t alive = 0;
  for (int64_t k = 0; k < b->n; ++k) alive += (b->i32[KID_BI_ALIVE][k] != 0);
  scalars[KID_S_NBERGS_ALIVE] = (double)alive;
}

/* set_conglom_ids FW:2601-2646 (+ remove_broken_bonds_between_congloms FW:2689-2731): what transfer_mts_bergs leaves
 * on one PE.  Conglomerates are numbered in traversal order of their first member. */
void ko_set_conglom_ids(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd) {
  double dummy[KID_NSCALAR] = {0};
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, dummy);
  for (int64_t k = 0; k < b->n; ++k) BI(KID_BI_CONGLOM_ID, k) = 0;
  int64_t *stack = (int64_t *)malloc(sizeof(int64_t) * (size_t)(c->nperm > 0 ? c->nperm : 1));
  int32_t newid = 0;
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k0 = c->perm[q];
    if (BI(KID_BI_CONGLOM_ID, k0) != 0) continue;
    newid = newid + 1;
    BI(KID_BI_CONGLOM_ID, k0) = newid;
    int64_t sp = 0; stack[sp++] = k0;
    while (sp > 0) { /* label_conglomerates (recursive in the reference; the labelling is order independent) */
      const int64_t k = stack[--sp];
      if (c->mb == 0) continue;
      for (int s = 0; s < bd->count[k]; ++s) {
        if (p->dem && bd->broken[BS(s, k)] == 1) continue;
        const int64_t o = c->other_row[BS(s, k)];
        if (o >= 0 && BI(KID_BI_CONGLOM_ID, o) != newid) { BI(KID_BI_CONGLOM_ID, o) = newid; stack[sp++] = o; }
      }
    }
  }
  free(stack);
  if (p->use_broken_bonds_for_substep_contact && c->mb > 0) {
    for (int64_t q = 0; q < c->nperm; ++q) {
      const int64_t k = c->perm[q];
      if (!(BI(KID_BI_N_BONDS, k) < p->max_bonds)) continue;
      int s = 0;
      while (s < bd->count[k]) {
        const int64_t o = c->other_row[BS(s, k)];
        if (bd->broken[BS(s, k)] == 1 && o >= 0 && BI(KID_BI_CONGLOM_ID, o) != BI(KID_BI_CONGLOM_ID, k)) {
          /* delete the matching bond on the other berg, then this one */
          for (int t = 0; t < bd->count[o]; ++t)
            if (bd->other_id[BS(t, o)] == b->id[k]) {
              for (int u = t; u + 1 < bd->count[o]; ++u) {
                bd->other_id[BS(u, o)] = bd->other_id[BS(u + 1, o)]; bd->broken[BS(u, o)] = bd->broken[BS(u + 1, o)];
                for (int f = 0; f < KID_NBOND_F64; ++f) BD(f, u, o) = BD(f, u + 1, o);
                c->other_row[BS(u, o)] = c->other_row[BS(u + 1, o)];
              }
              bd->count[o] -= 1;
              break;
            }
          for (int u = s; u + 1 < bd->count[k]; ++u) {
            bd->other_id[BS(u, k)] = bd->other_id[BS(u + 1, k)]; bd->broken[BS(u, k)] = bd->broken[BS(u + 1, k)];
            for (int f = 0; f < KID_NBOND_F64; ++f) BD(f, u, k) = BD(f, u + 1, k);
            c->other_row[BS(u, k)] = c->other_row[BS(u + 1, k)];
          }
          bd->count[k] -= 1;
        } else ++s;
      }
    }
  }
  ctx_free(c);
}

/* FW:4589-4614 (grid units, as the reference has it) */
void ko_orig_bond_length(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd) {
  double dummy[KID_NSCALAR] = {0};
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, dummy);
  for (int64_t q = 0; q < c->nperm; ++q) {
    const int64_t k = c->perm[q];
    for (int s = 0; s < bd->count[k]; ++s) {
      const int64_t o = c->other_row[BS(s, k)];
      if (o < 0) continue;
      const double dist = pow(BF(KID_B_LON, k) - BF(KID_B_LON, o), 2.) + pow(BF(KID_B_LAT, k) - BF(KID_B_LAT, o), 2.);
      BD(KID_BOND_LENGTH, s, k) = sqrt(dist);
    }
  }
  ctx_free(c);
}

/* FW:7163-7252: bi-quadratic Lagrange interpolation of an A-grid field (ocean_depth + ssh) on a 3x3 block of cells */
double ko_quad_interp_depth(const ko_grid *g, const kid_params *p, double x, double y, int i, int j, double xi, double yj) {
  const int mind = p->rev_mind ? 0 : 1;
  int is, ie, js, je;
  const int mi = ((i % 2) + 2) % 2, mj = ((j % 2) + 2) % 2; /* Fortran mod() of the (positive) cell indices */
  if (mi == mind) { if (xi >= 0.5) { is = i; ie = i + 2; } else { is = i - 2; ie = i; } } else { is = i - 1; ie = i + 1; }
  if (mj == mind) { if (yj >= 0.5) { js = j; je = j + 2; } else { js = j - 2; je = j; } } else { js = j - 1; je = j + 1; }
  double x1 = GS(g, KID_G_LONC, is, js), y1 = GS(g, KID_G_LATC, is, js);
  double x2 = GS(g, KID_G_LONC, ie, js), y2 = GS(g, KID_G_LATC, ie, js);
  double x3 = GS(g, KID_G_LONC, ie, je), y3 = GS(g, KID_G_LATC, ie, je);
  double x4 = GS(g, KID_G_LONC, is, je), y4 = GS(g, KID_G_LATC, is, je);
  double xloc, yloc;
  if (!g->d.grid_is_latlon && g->d.grid_is_regular) {
    const double dx = fabs(x3 - x4), dy = fabs(y3 - y2);
    x1 = x3 - (dx / 2); y1 = y3 - (dy / 2);
    const double Delta_x = ko_apply_modulo_around_point(x, x1, g->d.Lx) - x1;
    xloc = ((Delta_x) / dx) + 0.5; yloc = ((y - y1) / dy) + 0.5;
  } else if ((dmax(dmax(y1, y2), dmax(y3, y4)) < 89.999) || !g->d.grid_is_latlon) {
    ko_calc_xiyj(x1, x2, x3, x4, y1, y2, y3, y4, x, y, &xloc, &yloc, g->d.Lx);
  } else {
    const double pi_180 = p->pi / 180.;
    const double xx = (90. - y) * cos(x * pi_180), yy = (90. - y) * sin(x * pi_180);
    const double a1 = (90. - y1) * cos(GS(g, KID_G_LON, is, js) * pi_180), b1 = (90. - y1) * sin(GS(g, KID_G_LON, is, js) * pi_180);
    const double a2 = (90. - y2) * cos(GS(g, KID_G_LON, ie, je) * pi_180), b2 = (90. - y2) * sin(GS(g, KID_G_LON, ie, je) * pi_180);
    const double a3 = (90. - y3) * cos(GS(g, KID_G_LON, ie, je) * pi_180), b3 = (90. - y3) * sin(GS(g, KID_G_LON, ie, je) * pi_180);
    const double a4 = (90. - y4) * cos(GS(g, KID_G_LON, is, je) * pi_180), b4 = (90. - y4) * sin(GS(g, KID_G_LON, is, je) * pi_180);
    ko_calc_xiyj(a1, a2, a3, a4, b1, b2, b3, b4, xx, yy, &xloc, &yloc, g->d.Lx);
  }
  xloc = xloc * 2 - 1; yloc = yloc * 2 - 1;
  const double xb[3] = {0.5 * xloc * (xloc - 1), (1 + xloc) * (1 - xloc), 0.5 * xloc * (xloc + 1)};
  const double yb[3] = {0.5 * yloc * (yloc - 1), (1 + yloc) * (1 - yloc), 0.5 * yloc * (yloc + 1)};
  double sum = 0.;
  for (int b = 0; b < 3; ++b) for (int a = 0; a < 3; ++a) /* Fortran array order: first index fastest */
    sum = sum + xb[a] * yb[b] * (GS(g, KID_G_OCEAN_DEPTH, is + a, js + b) + GF(g, KID_F_SSH, is + a, js + b));
  return sum;
}

/* One icebergs_run() worth of the hot path with mts=.true. (IB:5423-5512).  `first_visit` does what the `Visited`
 * block does once after a restart (IB:5409-5420). */
void ko_run_step_mts(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, int first_visit,
                     double *acc, double *out, double *scalars) {
  const size_t ncell = (size_t)NI(g) * (size_t)NJ(g);
  memset(acc, 0, (size_t)KID_NACC * ncell * sizeof(double));
  if (first_visit) {
    ko_interp_gridded_fields_to_bergs(g, p, b);
    ko_set_conglom_ids(g, p, b, bd);
    if (p->iceberg_bonds_on && bd) ko_orig_bond_length(g, p, b, bd);
  }
  if (!p->static_icebergs) ko_evolve_icebergs_mts(g, p, b, bd, scalars);
  ko_interp_gridded_fields_to_bergs(g, p, b);   /* IB:5458 */
  ko_set_conglom_ids(g, p, b, bd);              /* transfer_mts_bergs, IB:5459 */
  ko_thermodynamics(g, p, b, acc, scalars);
  gridded_with_orientation(g, p, b, bd, acc, out);
  int64_t alive = 0;
  for (int64_t k = 0; k < b->n; ++k) alive += (b->i32[KID_BI_ALIVE][k] != 0);
  scalars[KID_S_NBERGS_ALIVE] = (double)alive;
}
