/* rk_interactive_ref.c -- checker of the RK4 integrator with interacting bergs (TEST INFRASTRUCTURE; tests/rk_interactive.py loads it,
 * __graft_entry__.build() compiles it).
 *
 * evolve_icebergs (IB:7081-7200) with Runge_not_Verlet and interactive_icebergs_on: the first loop calls Runge_Kutta_stepping
 * (IB:7331-7683) per berg and writes back the berg's own lon, lat, ine, jne, xi, yj, uvel, vvel, axn .. byn (IB:7157-7167); the
 * second loop (IB:7182-7197) copies uvel, vvel, lon, lat to the *_old members the next step's pair forces read.
 *
 * The stage driver below is rk4_step of oracle/kid_oracle.c, stage by stage, with the oracle's accel_sts_ia in the place of
 * ko_accel.  accel_sts_ia, interactive_force and ctx_init are static in oracle/kid_oracle_mts.c: that file is compiled into this
 * one, so the pair force exists once.  Everything else comes from libkid_oracle. */
#include "../oracle/kid_oracle_mts.c"
#include <stdint.h>

enum { TKO_CELL_CHANGES = 0, TKO_BOUNCES, TKO_TANGENT_STEPS, TKO_BERG_STEPS, TKO_NCOUNT };
static int64_t g_counts[TKO_NCOUNT];
static int g_mode = 0;            /* traversal of the first sweep: 0 reference order, 1 reversed, 2 shuffled */
static uint64_t g_seed = 0;

void tko_set_traversal(int mode, int64_t seed) { g_mode = mode; g_seed = (uint64_t)seed; }
void tko_reset_counts(void) { memset(g_counts, 0, sizeof(g_counts)); }
void tko_get_counts(int64_t *out) { memcpy(out, g_counts, sizeof(g_counts)); }

static uint64_t next_u64(uint64_t *s) { /* splitmix64 */
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

/* IB:7331-7679 Runge_Kutta_stepping for row k.  Nothing of the row is written here. */
static void rk4_step_ia(mts_ctx *c, int64_t k, double *axn_o, double *ayn_o, double *bxn_o, double *byn_o, double *uveln, double *vveln,
                        double *lonn, double *latn, int *io, int *jo, double *xio, double *yjo, int *err) {
  const ko_grid *g = c->g; const kid_params *p = c->p;
  const double dt = p->dt, dt_2 = 0.5 * dt, dt_6 = dt / 6.;
  const double xi0 = BF(KID_B_XI, k), yj0 = BF(KID_B_YJ, k);
  int i = BI(KID_BI_INE, k), j = BI(KID_BI_JNE, k); double xi = xi0, yj = yj0;
  int bounced = 0, any_bounce = 0, moved = 0;
  const int on_tang = (BF(KID_B_LAT, k) > 89.) && g->d.grid_is_latlon;
  const int i1 = i, j1 = j;
  double axn = BF(KID_B_AXN, k), ayn = BF(KID_B_AYN, k), bxn = 0., byn = 0.;
  double axn1 = axn, axn2 = axn, axn3 = axn, axn4 = axn, ayn1 = ayn, ayn2 = ayn, ayn3 = ayn, ayn4 = ayn;
  double lon1 = BF(KID_B_LON, k), lat1 = BF(KID_B_LAT, k), x1 = 0, y1 = 0;
  if (on_tang) ko_rotpos_to_tang(p, lon1, lat1, &x1, &y1);
  double dxdl1, dydl; ko_meters_to_grid(g, p, lat1, &dxdl1, &dydl);
  double uvel1 = BF(KID_B_UVEL, k), vvel1 = BF(KID_B_VVEL, k), xdot1 = 0, ydot1 = 0;
  if (on_tang) ko_rotvec_to_tang(p, lon1, uvel1, vvel1, &xdot1, &ydot1);
  double u1 = uvel1 * dxdl1, v1 = vvel1 * dydl;
  double ax1, ay1, xddot1 = 0, yddot1 = 0, xddot1n = 0, yddot1n = 0;
  accel_sts_ia(c, k, i, j, xi, yj, lat1, uvel1, vvel1, uvel1, vvel1, dt_2, &ax1, &ay1, &axn1, &ayn1, &bxn, &byn);
  if (on_tang) { ko_rotvec_to_tang(p, lon1, ax1, ay1, &xddot1, &yddot1); ko_rotvec_to_tang(p, lon1, axn1, ayn1, &xddot1n, &yddot1n); }
  /* stage 2 */
  double lon2, lat2, uvel2, vvel2, x2, y2, xdot2 = 0, ydot2 = 0;
  if (on_tang) {
    x2 = x1 + dt_2 * xdot1; y2 = y1 + dt_2 * ydot1;
    xdot2 = xdot1 + dt_2 * xddot1; ydot2 = ydot1 + dt_2 * yddot1;
    ko_rotpos_from_tang(p, x2, y2, &lon2, &lat2); ko_rotvec_from_tang(p, lon2, xdot2, ydot2, &uvel2, &vvel2);
  } else { lon2 = lon1 + dt_2 * u1; lat2 = lat1 + dt_2 * v1; uvel2 = uvel1 + dt_2 * ax1; vvel2 = vvel1 + dt_2 * ay1; }
  i = i1; j = j1; xi = xi0; yj = yj0;
  ko_adjust_index_and_ground(g, p, &lon2, &lat2, &i, &j, &xi, &yj, &bounced, err);
  any_bounce |= bounced; moved |= (i != i1 || j != j1);
  double dxdl2; ko_meters_to_grid(g, p, lat2, &dxdl2, &dydl);
  double u2 = uvel2 * dxdl2, v2 = vvel2 * dydl;
  double ax2, ay2, xddot2 = 0, yddot2 = 0, xddot2n = 0, yddot2n = 0;
  accel_sts_ia(c, k, i, j, xi, yj, lat2, uvel2, vvel2, uvel1, vvel1, dt_2, &ax2, &ay2, &axn2, &ayn2, &bxn, &byn);
  if (on_tang) { ko_rotvec_to_tang(p, lon2, ax2, ay2, &xddot2, &yddot2); ko_rotvec_to_tang(p, lon2, axn2, ayn2, &xddot2n, &yddot2n); }
  /* stage 3 */
  double lon3, lat3, uvel3, vvel3, x3, y3, xdot3 = 0, ydot3 = 0;
  if (on_tang) {
    x3 = x1 + dt_2 * xdot2; y3 = y1 + dt_2 * ydot2;
    xdot3 = xdot1 + dt_2 * xddot2; ydot3 = ydot1 + dt_2 * yddot2;
    ko_rotpos_from_tang(p, x3, y3, &lon3, &lat3); ko_rotvec_from_tang(p, lon3, xdot3, ydot3, &uvel3, &vvel3);
  } else { lon3 = lon1 + dt_2 * u2; lat3 = lat1 + dt_2 * v2; uvel3 = uvel1 + dt_2 * ax2; vvel3 = vvel1 + dt_2 * ay2; }
  i = i1; j = j1; xi = xi0; yj = yj0;
  ko_adjust_index_and_ground(g, p, &lon3, &lat3, &i, &j, &xi, &yj, &bounced, err);
  any_bounce |= bounced; moved |= (i != i1 || j != j1);
  double dxdl3; ko_meters_to_grid(g, p, lat3, &dxdl3, &dydl);
  double u3 = uvel3 * dxdl3, v3 = vvel3 * dydl;
  double ax3, ay3, xddot3 = 0, yddot3 = 0, xddot3n = 0, yddot3n = 0;
  accel_sts_ia(c, k, i, j, xi, yj, lat3, uvel3, vvel3, uvel1, vvel1, dt, &ax3, &ay3, &axn3, &ayn3, &bxn, &byn);
  if (on_tang) { ko_rotvec_to_tang(p, lon3, ax3, ay3, &xddot3, &yddot3); ko_rotvec_to_tang(p, lon3, axn3, ayn3, &xddot3n, &yddot3n); }
  /* stage 4 */
  double lon4, lat4, uvel4, vvel4, x4, y4, xdot4 = 0, ydot4 = 0;
  if (on_tang) {
    x4 = x1 + dt * xdot3; y4 = y1 + dt * ydot3;
    xdot4 = xdot1 + dt * xddot3; ydot4 = ydot1 + dt * yddot3;
    ko_rotpos_from_tang(p, x4, y4, &lon4, &lat4); ko_rotvec_from_tang(p, lon4, xdot4, ydot4, &uvel4, &vvel4);
  } else { lon4 = lon1 + dt * u3; lat4 = lat1 + dt * v3; uvel4 = uvel1 + dt * ax3; vvel4 = vvel1 + dt * ay3; }
  i = i1; j = j1; xi = xi0; yj = yj0;
  ko_adjust_index_and_ground(g, p, &lon4, &lat4, &i, &j, &xi, &yj, &bounced, err);
  any_bounce |= bounced; moved |= (i != i1 || j != j1);
  double dxdl4; ko_meters_to_grid(g, p, lat4, &dxdl4, &dydl);
  double u4 = uvel4 * dxdl4, v4 = vvel4 * dydl;
  double ax4, ay4, xddot4 = 0, yddot4 = 0, xddot4n = 0, yddot4n = 0;
  accel_sts_ia(c, k, i, j, xi, yj, lat4, uvel4, vvel4, uvel1, vvel1, dt, &ax4, &ay4, &axn4, &ayn4, &bxn, &byn);
  if (on_tang) { ko_rotvec_to_tang(p, lon4, ax4, ay4, &xddot4, &yddot4); ko_rotvec_to_tang(p, lon4, axn4, ayn4, &xddot4n, &yddot4n); }
  /* combine IB:7597-7616 */
  if (on_tang) {
    double xn = x1 + dt_6 * ((xdot1 + xdot4) + 2. * (xdot2 + xdot3));
    double yn = y1 + dt_6 * ((ydot1 + ydot4) + 2. * (ydot2 + ydot3));
    double xdotn = xdot1 + dt_6 * ((xddot1 + xddot4) + 2. * (xddot2 + xddot3));
    double ydotn = ydot1 + dt_6 * ((yddot1 + yddot4) + 2. * (yddot2 + yddot3));
    double xddotn = ((xddot1n + xddot4n) + 2. * (xddot2n + xddot3n)) / 6.;
    double yddotn = ((yddot1n + yddot4n) + 2. * (yddot2n + yddot3n)) / 6.;
    ko_rotpos_from_tang(p, xn, yn, lonn, latn);
    ko_rotvec_from_tang(p, *lonn, xdotn, ydotn, uveln, vveln);
    ko_rotvec_from_tang(p, *lonn, xddotn, yddotn, &axn, &ayn);
    /* bxn, byn keep the values left by the 4th accel call */
  } else {
    *lonn = lon1 + dt_6 * ((u1 + u4) + 2. * (u2 + u3));
    *latn = lat1 + dt_6 * ((v1 + v4) + 2. * (v2 + v3));
    *uveln = uvel1 + dt_6 * ((ax1 + ax4) + 2. * (ax2 + ax3));
    *vveln = vvel1 + dt_6 * ((ay1 + ay4) + 2. * (ay2 + ay3));
    axn = ((axn1 + axn4) + 2. * (axn2 + axn3)) / 6.;
    ayn = ((ayn1 + ayn4) + 2. * (ayn2 + ayn3)) / 6.;
    bxn = (((ax1 + ax4) + 2. * (ax2 + ax3)) / 6) - (axn / 2);
    byn = (((ay1 + ay4) + 2. * (ay2 + ay3)) / 6) - (ayn / 2);
  }
  i = i1; j = j1; xi = xi0; yj = yj0;
  ko_adjust_index_and_ground(g, p, lonn, latn, &i, &j, &xi, &yj, &bounced, err);
  any_bounce |= bounced;
  *axn_o = axn; *ayn_o = ayn; *bxn_o = bxn; *byn_o = byn; *io = i; *jo = j; *xio = xi; *yjo = yj;
  g_counts[TKO_CELL_CHANGES] += moved; g_counts[TKO_BOUNCES] += any_bounce; g_counts[TKO_TANGENT_STEPS] += on_tang; g_counts[TKO_BERG_STEPS] += 1;
}

void tko_evolve_icebergs_interactive_rk(const ko_grid *g, const kid_params *p, kid_berg_soa *b, kid_bond_soa *bd, double *scalars) {
  mts_ctx ctx, *c = &ctx;
  ctx_init(c, g, p, b, bd, scalars);
  const int64_t np = c->nperm;
  int64_t *visit = (int64_t *)malloc(sizeof(int64_t) * (size_t)(np > 0 ? np : 1));
  for (int64_t q = 0; q < np; ++q) visit[q] = (g_mode == 1) ? c->perm[np - 1 - q] : c->perm[q];
  if (g_mode == 2) {
    uint64_t s = g_seed;
    for (int64_t q = np - 1; q > 0; --q) { const int64_t r = (int64_t)(next_u64(&s) % (uint64_t)(q + 1)); const int64_t t = visit[q]; visit[q] = visit[r]; visit[r] = t; }
  }
  for (int64_t q = 0; q < np; ++q) { /* first sweep IB:7106-7179 */
    const int64_t k = visit[q];
    if (!(BF(KID_B_STATIC_BERG, k) < 0.5)) continue;
    double axn, ayn, bxn, byn, uveln, vveln, lonn, latn, xi, yj; int i, j, err = 0;
    rk4_step_ia(c, k, &axn, &ayn, &bxn, &byn, &uveln, &vveln, &lonn, &latn, &i, &j, &xi, &yj, &err);
    if (err) scalars[KID_S_ERROR_COUNT] += 1.;
    if (p->override_iceberg_velocities) { uveln = p->u_override; vveln = p->v_override; }   /* IB:7151-7154 */
    BF(KID_B_AXN, k) = axn; BF(KID_B_AYN, k) = ayn; BF(KID_B_BXN, k) = bxn; BF(KID_B_BYN, k) = byn;
    BF(KID_B_UVEL, k) = uveln; BF(KID_B_VVEL, k) = vveln; BF(KID_B_LON, k) = lonn; BF(KID_B_LAT, k) = latn;
    BF(KID_B_XI, k) = xi; BF(KID_B_YJ, k) = yj; BI(KID_BI_INE, k) = i; BI(KID_BI_JNE, k) = j;
  }
  for (int64_t q = 0; q < np; ++q) { /* second sweep IB:7182-7197; a berg whose cell left the computational domain is sent away */
    const int64_t k = c->perm[q];
    if (!(BF(KID_B_STATIC_BERG, k) < 0.5)) continue;
    BF(KID_B_UVEL_OLD, k) = BF(KID_B_UVEL, k); BF(KID_B_VVEL_OLD, k) = BF(KID_B_VVEL, k);
    BF(KID_B_LON_OLD, k) = BF(KID_B_LON, k); BF(KID_B_LAT_OLD, k) = BF(KID_B_LAT, k);
    const int i = BI(KID_BI_INE, k), j = BI(KID_BI_JNE, k);
    if (i < g->d.isc || i > g->d.iec || j < g->d.jsc || j > g->d.jec) BI(KID_BI_ALIVE, k) = 0;
  }
  free(visit);
  ctx_free(c);
}
