/* kid_oracle.h -- CPU restatement (ORACLE) of the NOAA-GFDL/icebergs per-berg evolve loop.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ may be imported, linked or executed by the product
 * (icebergs_amd/): only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use it, and
 * there only as the checker.  See oracle/kid_oracle.c for the pinning status.
 */
#ifndef KID_ORACLE_H
#define KID_ORACLE_H
#include "../include/kid_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ko_grid {
  kid_grid_desc d;
  const double *stat[KID_NGRID_STATIC];   /* static grid fields  */
  const double *forc[KID_NFORCING];       /* forcing fields      */
  int32_t *iceberg_counter;               /* grd%iceberg_counter_grd (FW:1017), per cell; may be NULL without footloose */
} ko_grid;

/* geometry (icebergs_framework.F90) */
double ko_modulo(double a, double p);
double ko_apply_modulo_around_point(double x, double y, double Lx);
double ko_bilin(const ko_grid *g, const kid_params *p, const double *fld, int i, int j, double xi, double yj);
int    ko_sum_sign_dot_prod4(double x0, double y0, double x1, double y1, double x2, double y2,
                             double x3, double y3, double x, double y, double Lx);
int    ko_sum_sign_dot_prod5(double x0, double y0, double x1, double y1, double x2, double y2,
                             double x3, double y3, double x4, double y4, double x, double y, double Lx);
int    ko_is_point_in_cell(const ko_grid *g, double x, double y, int i, int j);
int    ko_calc_xiyj(double x1, double x2, double x3, double x4, double y1, double y2, double y3, double y4,
                    double x, double y, double *xi, double *yj, double Lx);
int    ko_pos_within_cell(const ko_grid *g, const kid_params *p, double x, double y, int i, int j,
                          double *xi, double *yj, int *err);

/* environment + momentum (icebergs.F90) */
void ko_interp_flds(const ko_grid *g, const kid_params *p, double x, double y, int i, int j, double xi, double yj,
                    double env[13]);
void ko_accel(const ko_grid *g, const kid_params *p, const double bergstate[], int n_bonds,
              int i, int j, double xi, double yj, double lat, double uvel, double vvel, double uvel0, double vvel0,
              double dt, double *ax, double *ay, double *axn, double *ayn, double *bxn, double *byn,
              int64_t *ntickets);
void ko_adjust_index_and_ground(const ko_grid *g, const kid_params *p, double *lon, double *lat,
                                int *i, int *j, double *xi, double *yj, int *bounced, int *err);

/* thermodynamics helpers */
void   ko_rolling(const kid_params *p, double *Tn, double *Wn, double *Ln);
void   ko_fl_bits_dimensions(const kid_params *p, double thickness, double *L_fl, double *W_fl, double *T_fl);
double ko_find_basal_melt(const kid_grid_desc *gd, const kid_params *p, double dvo, double lat, double salt,
                          double temp, int use_three_eq, double thickness);

/* mass spreading geometry */
void ko_hexagon_into_quadrants(double x0, double y0, double H, double theta, double *Area_hex,
                               double *Q1, double *Q2, double *Q3, double *Q4);
int  ko_point_in_triangle(double Ax, double Ay, double Bx, double By, double Cx, double Cy, double qx, double qy);
void ko_spread_weights(const ko_grid *g, const kid_params *p, int i, int j, double x, double y,
                       double Area, double static_berg, double w[9], double *I_fraction_used);

/* whole phases over a berg population (SoA in, SoA out, in place) */
void ko_interp_gridded_fields_to_bergs(const ko_grid *g, const kid_params *p, kid_berg_soa *b);
void ko_evolve_icebergs(const ko_grid *g, const kid_params *p, kid_berg_soa *b, double *scalars);
void ko_thermodynamics(const ko_grid *g, const kid_params *p, kid_berg_soa *b, double *acc, double *scalars);
void ko_create_gridded_icebergs_fields(const ko_grid *g, const kid_params *p, kid_berg_soa *b,
                                       double *acc, double *out);
void ko_calculate_mass_on_ocean(const ko_grid *g, const kid_params *p, kid_berg_soa *b, double *acc);
void ko_gather_fields(const ko_grid *g, const kid_params *p, double *acc, double *out);
void ko_step_local(const ko_grid *g, const kid_params *p, kid_berg_soa *b, int64_t capacity, double *acc, double *scalars);
/* sharded find_melt_using_spread_mass: two planes (spread_mass_old, spread_mass_tmp) that ko_step_local fills from its shard,
 * the caller sums over the ranks and ko_gather_fields reads; NULL switches back */
void ko_set_spread_mass_buffer(double *two_planes);
void ko_footloose_calving(const ko_grid *g, const kid_params *p, kid_berg_soa *b, int64_t capacity,
                          double *acc, double *scalars);
void ko_meters_to_grid(const ko_grid *g, const kid_params *p, double lat_ref, double *dlon_dx, double *dlat_dy);
void ko_rotpos_to_tang(const kid_params *p, double lon, double lat, double *x, double *y);
void ko_rotpos_from_tang(const kid_params *p, double x, double y, double *lon, double *lat);
void ko_rotvec_to_tang(const kid_params *p, double lon, double uvel, double vvel, double *xdot, double *ydot);
void ko_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double ko_fl_uniform(int32_t seed, int64_t berg_id, int64_t step, int32_t draw);
/* the footloose step (number of footloose_calving calls so far): third counter word of the generator in include/kid_rng.h */
void ko_set_fl_step(int64_t step);
int64_t ko_get_fl_step(void);
/* One icebergs_run() worth of the hot path (IB:5423-5512), accumulators zeroed first.
 * acc: KID_NACC fields of (ied-isd+1)*(jed-jsd+1); out: KID_NOUT fields; scalars: KID_NSCALAR. */
void ko_run_step(const ko_grid *g, const kid_params *p, kid_berg_soa *b, int64_t capacity,
                 double *acc, double *out, double *scalars);
/* bergs_chksum FW:6889-6987 (+ berg_chksum, time_hash, pos_hash, FMS mpp_chksum): chksum, chksum2, chksum3, chksum4, chksum5, # */
void ko_bergs_chksum(const ko_grid *g, const kid_berg_soa *b, int64_t out[6]);
/* reference traversal order: permutation sorted by (jne, ine, inorder-key) */
void ko_reference_order(const kid_berg_soa *b, int64_t *perm);
/* berg migration between sub-domains: send_bergs_to_other_pes FW:2997-3247, pack / unpack FW:3250-3301, 3455-3680 */
int  ko_check_and_find_cell(const ko_grid *g, double x, double y, int *oi, int *oj);
long ko_send_bergs(const ko_grid *g, kid_berg_soa *b, int dir, double *buf);
long ko_unpack_bergs(const ko_grid *g, const kid_params *p, kid_berg_soa *b, const double *buf, long m);

/* multiple time stepping / DEM (oracle/kid_oracle_mts.c) */
void ko_evolve_icebergs_mts(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars);
void ko_set_conglom_ids(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd);
/* calculate_force_dem for one pair given by value: id[2], x[26] in, out[40] (layouts at its definition) */
void ko_dem_pair(const kid_params *p, int latlon, const int64_t *id, const double *x, double *out);
void ko_orig_bond_length(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd);
double ko_quad_interp_depth(const ko_grid *g, const kid_params *p, double x, double y, int i, int j, double xi, double yj);
void ko_run_step_mts(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, int first_visit,
                     double *acc, double *out, double *scalars);

void ko_set_orientation(const double *per_berg);
void ko_find_orientations(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *orientation);
void ko_evolve_icebergs_interactive(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars);
void ko_run_step_interactive(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, int first_visit,
                             double *acc, double *out, double *scalars);
/* calving source (oracle/kid_oracle_calving.c), IB:5203-5231 + accumulate_calving IB:6153 + calve_icebergs IB:6225.
 * All planes cover the data domain; stored_ice / real_calving are KID_NCLASSES consecutive planes. */
typedef struct ko_calving_state {
  double *calving, *calving_hflx;                 /* grd%calving (kg/s after the call: the unused remainder), grd%calving_hflx */
  double *stored_ice, *stored_heat, *real_calving;
  double *rmean_calving, *rmean_calving_hflx;
  int32_t first_call, rmean_calving_initialized, rmean_calving_hflx_initialized, pad;
} ko_calving_state;
int ko_calving(const ko_grid *g, const kid_params *p, const kid_calving_params *cp, const double *calving_in,
               const double *calving_hflx_in, ko_calving_state *s, kid_berg_soa *b, int64_t capacity, double *scalars);
/* forcing ingest (oracle/kid_oracle_ingest.c), IB:5236-5383; returns non-zero on inconsistent extents / staggers */
int ko_ingest_forcing(const ko_grid *g, const kid_forcing_in *in, double *const out[KID_NFORCING]);
void ko_default_params(kid_params *p);
int64_t ko_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
