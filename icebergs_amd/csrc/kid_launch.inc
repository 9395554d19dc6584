// kid_launch.inc -- the launch path of the per-berg kernel: which instance a handle gets (kid_launch_select.hpp), the three
// schedules (one stream, two halves, slow lane), and the entry points that go through them: the four phase entry points,
// kid_step_local, kid_step_gather, kid_run_step.  Included by kid_hip.hip once, after every host function a step calls.

// May the hot build be the plain one (berg_kernel<..., K = 1>, kid_device.hpp)?  Only when every switch of KID_SWITCHES
// has the value that build folds in, and none of the handle's flags is set.
static bool plain_namelist(const kid_handle *h) {
  const kid_params &p = h->params;
  bool same = true;
#define KID_X(name, plain, flp) same = same && (p.name == (decltype(p.name))(plain));
  KID_SWITCHES(KID_X)
#undef KID_X
  const Flags &f = h->flags;
  return same && h->gd.grid_is_latlon && !p.pass_fields_to_ocean_model && !f.has_static && !f.has_fl && !f.footprint && !f.no_diag &&
         !h->dbg.no_plain_build;
}
// ... and K = 2 with the footloose profile's (Cartesian grid, footloose state, no static bergs, no footprint planes)
static bool fl_profile_namelist(const kid_handle *h) {
  const kid_params &p = h->params;
  bool same = true;
#define KID_X(name, plain, flp) same = same && (p.name == (decltype(p.name))(flp));
  KID_SWITCHES(KID_X)
#undef KID_X
  const Flags &f = h->flags;
  return same && !h->gd.grid_is_latlon && !p.pass_fields_to_ocean_model && !f.has_static && f.has_fl && !f.footprint && !f.no_diag && !h->dbg.no_plain_build;
}
static bool lanes_eligible(const kid_handle *h) {
  const kid_params &p = h->params;
  return kid::lanes_eligible(h->side_mode, h->side_stream != nullptr, h->repro, p.static_icebergs != 0, p.mts != 0, p.interactive_icebergs_on != 0,
                             p.footloose != 0, p.grounding_fraction, p.find_melt_using_spread_mass != 0, (long long)h->n);
}

// -------------------------------------------------------------------------------------------------------
// one launch of one instance
// -------------------------------------------------------------------------------------------------------
// what every launch of one launch_berg / launch_berg_lanes call shares
struct BergLaunch { const DevGrid *gtab; bool plain, flprof; };
static BergLaunch berg_launch(const kid_handle *h) { return {h->fset[h->forc_parity].d_grid, plain_namelist(h), fl_profile_namelist(h)}; }

template <bool RK, bool OLD, unsigned PH, bool FAST, int K, bool STAGE>
static int launch_instance(kid_handle *h, const BergLaunch &c, hipStream_t s, unsigned nblocks, const Redo &redo) {
  static_assert(instance_exists(OLD, PH, STAGE), "no call site requests this instance (kid_launch_select.hpp)");
  hipLaunchKernelGGL((berg_kernel<RK, OLD, PH, FAST, K, STAGE>), dim3(nblocks), dim3(FAST ? KID_HOT_WG : 64), 0, s, c.gtab, h->d_params, h->d_bp, (long long)h->n, h->d_acc, h->ncell, h->flags, redo);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
// pass 1: every row of [redo.k0, redo.k0 + redo.klen) through the hot build hot_build_k names.  The plain builds live in a
// translation unit of their own (kid_hot_plain.inc); rebin: their re-binning instance (redo.rb, redo.perm).
template <bool RK, bool OLD, unsigned PH, bool STAGE>
static int launch_hot(kid_handle *h, const BergLaunch &c, hipStream_t s, const Redo &redo, bool rebin = false) {
  const unsigned nbp = (unsigned)((redo.klen + KID_HOT_WG - 1) / KID_HOT_WG);
  const int k = hot_build_k(RK, OLD, PH, c.plain, c.flprof, h->flags.store_env != 0, STAGE);
  h->hot_zero_mask = 0ull;   // (every build but the plain ones loads and stores every field)
  if constexpr (hot_build_k(RK, OLD, PH, true, false, false, STAGE) == 1) {   // (RK, OLD, PH) has plain builds
    if (k == 1 || k == 3) {
      // the fields this launch need not load or store: zeros in every row (known_zero_mask; the launch's own marks are set by now)
      Redo plain = redo;
      plain.zero = h->hot_zero_mask = known_zero_mask(h);
      kid::launch_hot_plain(k == 3, rebin, nbp, (void *)s, c.gtab, h->d_params, h->d_bp, (long long)h->n, h->d_acc, h->ncell, &h->flags, &plain);
      KID_HIP(h, hipGetLastError());
      return KID_OK;
    }
  }
  if constexpr (hot_build_k(RK, OLD, PH, false, true, false, STAGE) == 2) {   // ... has the footloose-profile build
    if (k == 2 && !rebin) return launch_instance<RK, OLD, PH, true, 2, STAGE>(h, c, s, nbp, redo);
  }
  if (rebin || k != 0) { h->err = "no such hot build of the per-berg kernel"; return KID_EINVAL; }
  return launch_instance<RK, OLD, PH, true, 0, STAGE>(h, c, s, nbp, redo);
}
// pass 2: the general build over the rows pass 1 queued (a few per cent: cell crossings, coast bounces, polar cells).  It is
// sized for the worst case of `rows` and its surplus workgroups exit on the device-side count.
template <bool RK, bool OLD, unsigned PH, bool STAGE>
static int launch_general(kid_handle *h, const BergLaunch &c, hipStream_t s, const Redo &redo, long long rows) {
  return launch_instance<RK, OLD, PH, false, 0, STAGE>(h, c, s, (unsigned)std::min<long long>((rows + 63) / 64, 2048), redo);
}
// The handle's (Runge_not_Verlet, old_interp_flds_order) and `stage` as template arguments of f.  An instance that does
// not exist is never instantiated; asking for it is an error.
template <unsigned PH, class F>
static int with_instance(kid_handle *h, bool stage, F &&f) {
  const bool rk = h->params.Runge_not_Verlet != 0, old = h->params.old_interp_flds_order != 0;
  auto go = [&](auto RK, auto OLD, auto STAGE) -> int {
    if constexpr (instance_exists(decltype(OLD)::value, PH, decltype(STAGE)::value)) return f(RK, OLD, STAGE);
    else { h->err = "no per-berg kernel for this phase mask, interpolation order and summation mode"; return KID_EINVAL; }
  };
  auto order = [&](auto RK, auto STAGE) { return old ? go(RK, std::true_type{}, STAGE) : go(RK, std::false_type{}, STAGE); };
  auto integrator = [&](auto STAGE) { return rk ? order(std::true_type{}, STAGE) : order(std::false_type{}, STAGE); };
  return stage ? integrator(std::true_type{}) : integrator(std::false_type{});
}

// -------------------------------------------------------------------------------------------------------
// launch_berg: the steps of its sequence
// -------------------------------------------------------------------------------------------------------
// Pipelined (a side stream is set): two halves; the general build of a half runs on the side stream while the main
// stream is already in the hot build of the other half (or of the next step): the ~85 us single-wave latency of the
// general build leaves the critical path.  Events order a half's hot build behind its own previous general build.
static int wait_general_builds(kid_handle *h, int part, int nparts) {
  if (h->evG_live[part]) KID_HIP(h, hipStreamWaitEvent(h->stream, h->evG[part], 0));
  if (nparts == 1 && h->evG_live[1]) KID_HIP(h, hipStreamWaitEvent(h->stream, h->evG[1], 0));
  return KID_OK;
}
static int zero_redo_counter(kid_handle *h, int *count) {   // (a prepass has done it for this step otherwise)
  if (!h->redo_prezeroed) KID_HIP(h, hipMemsetAsync(count, 0, sizeof(int), h->stream));
  return KID_OK;
}
// profiling: one (start, stop) pair around every hot-build launch (around hot and general build of a staging launch)
struct ProfilePair { hipEvent_t e0 = nullptr, e1 = nullptr; };
static int profile_start(kid_handle *h, ProfilePair &t) {
  if (!h->profile) return KID_OK;
  KID_HIP(h, hipEventCreate(&t.e0)); KID_HIP(h, hipEventCreate(&t.e1));
  KID_HIP(h, hipEventRecord(t.e0, h->stream));
  return KID_OK;
}
static int profile_stop(kid_handle *h, const ProfilePair &t) {
  if (!h->profile) return KID_OK;
  KID_HIP(h, hipEventRecord(t.e1, h->stream));
  h->pending.emplace_back(t.e0, t.e1); h->berg_launches++;
  return KID_OK;
}
// A pending re-binning: the whole-population plain hot build takes its rows through the permutation (the re-binning
// instance, kid_berg_kernel.hpp) and the general build that follows finds them in the new arrays; every other launch
// gets the rows copied first.
template <unsigned PH>
static int rebin_take_or_flush(kid_handle *h, bool whole, RebinTab &rtab, bool &fused) {
  fused = false;
  if (!h->rebin_pending) return KID_OK;
  // (Purely defensive: a field the plan left in place as zeros that this launch may write would have the launch store rows into
  // the array other lanes still read theirs from.  No sequence reaches it today -- whatever sets a mark flushes the pending
  // re-binning first or makes the step non-fusable -- the condition keeps that from depending on call sites elsewhere.)
  // (The same for a field the plan left in place as cold that a step of the handle now touches: cold_holds.)
  fused = PH == PH_STEP && rebin_fusable(h) && whole && h->rplan.n == h->n && (h->rplan.zero_skipped & ~known_zero_mask(h)) == 0ull && cold_holds(h) &&
          rebin_table(h, h->flags.store_env ? 3 : 1, rtab);
  return fused ? KID_OK : rebin_flush_rows(h);
}
// Cold fields stay deferred through the plain fused step alone -- the launch their rule was read from (kid_rows_plan.hpp); every
// other launch of the per-berg kernel finds every field in row order
template <unsigned PH>
static int cold_for_launch(kid_handle *h) {
  if (!h->cold.deferred || (PH == PH_STEP && rebin_fusable(h) && cold_holds(h))) return KID_OK;
  return cold_materialise(h);
}
static int rebin_bind(kid_handle *h, const RebinTab &rtab, Redo &redo) {
  hipLaunchKernelGGL(set_rebin_table_kernel, dim3(1), dim3(64), 0, h->stream, rtab, h->d_rb);
  KID_HIP(h, hipGetLastError());
  redo.rb = h->d_rb; redo.perm = h->rplan.perm;
  return KID_OK;
}
// after the hot build: the rows are in the second set of arrays now, the general build reads them there.  (On failure the
// table could not follow the rows: nothing more is launched on them.)
static int rebin_hand_over(kid_handle *h, Redo &redo) {
  h->rebin_pending = false; redo.rb = nullptr; redo.perm = nullptr; h->rebin_fused_count++;
  return rebin_swap(h);
}
// the general build of a part: on the main stream, or (two halves) on the side stream behind the part's hot build
template <bool RK, bool OLD, unsigned PH>
static int launch_general_part(kid_handle *h, const BergLaunch &c, const Redo &redo, int part, int nparts) {
  hipStream_t gs = (nparts == 2) ? h->side_stream : h->stream;
  if (nparts == 2) { KID_HIP(h, hipEventRecord(h->evF[part], h->stream)); KID_HIP(h, hipStreamWaitEvent(gs, h->evF[part], 0)); }
  const int rc = launch_general<RK, OLD, PH, false>(h, c, gs, redo, redo.klen);
  if (rc) return rc;
  if (nparts == 2) KID_HIP(h, hipEventRecord(h->evG[part], gs));
  h->evG_live[part] = nparts == 2;
  return KID_OK;
}
template <unsigned PH>
static int launch_berg_part(kid_handle *h, const BergLaunch &c, bool stage, const RebinTab *rtab, Redo redo, int part, int nparts) {
  int rc = KID_OK;
  if (rtab) { rc = rebin_bind(h, *rtab, redo); if (rc) return rc; }
  rc = wait_general_builds(h, part, nparts);
  if (!rc) rc = zero_redo_counter(h, redo.count);
  ProfilePair t;
  if (!rc) rc = profile_start(h, t);
  if (rc) return rc;
  return with_instance<PH>(h, stage, [&](auto RK, auto OLD, auto STAGE) -> int {
    constexpr bool rk = decltype(RK)::value, old = decltype(OLD)::value;
    int r = launch_hot<rk, old, PH, decltype(STAGE)::value>(h, c, h->stream, redo, rtab != nullptr);
    if constexpr (decltype(STAGE)::value) {   // the staging instance (reproducible sums): K = 0, both builds on the main stream
      if (!r) r = launch_general<rk, old, PH, true>(h, c, h->stream, redo, redo.klen);
      if (!r) r = profile_stop(h, t);
      h->evG_live[part] = false;
      return r;
    } else {
      if (!r) r = profile_stop(h, t);   // the timed kernel is the hot build (pass 1)
      if (!r && rtab) r = rebin_hand_over(h, redo);
      return r ? r : launch_general_part<rk, old, PH>(h, c, redo, part, nparts);
    }
  });
}
// One phase mask over the rows [range_k0, range_k0 + range_len) (default: all)
template <unsigned PH>
static int launch_phase(kid_handle *h, long long range_k0 = 0, long long range_len = -1) {
  if (need_forcing(h)) return KID_EINVAL;
  if (h->n == 0 || range_len == 0) return KID_OK;
  const bool old = h->params.old_interp_flds_order != 0, whole = range_k0 == 0 && range_len < 0;
  if (!old && !(PH & PH_INTERP) && (PH & (PH_EVOLVE | PH_THERMO)) && !h->flags.store_env) {
    h->err = "this entry point reads the bergs' stored environment, which kid_set_store_environment has switched off (use kid_run_step, or switch it on)";
    return KID_EINVAL;
  }
  h->zs.launched_berg((PH & PH_EVOLVE) != 0, (PH & PH_THERMO) != 0, h->params.Runge_not_Verlet != 0, h->params.bergy_bit_erosion_fraction == 0.,
                      h->flags.has_fl != 0, (PH & PH_FL) != 0);
  int rc = repro_refuse(h);
  if (!rc) rc = lanes_drain(h);
  RebinTab rtab;
  bool rebin_fused = false;
  if (!rc) rc = rebin_take_or_flush<PH>(h, whole, rtab, rebin_fused);
  if (!rc) rc = cold_for_launch<PH>(h);
  if (!rc) rc = refresh_tables(h);
  if (rc) return rc;
  const BergLaunch c = berg_launch(h);
  rows_killed(h);
  if (h->flags.store_env || !old) h->env_ever_stored = true;
  const bool stage = (PH & PH_SCATTER) != 0 && h->repro;   // the staging instance (kid_repro.inc); one part, no pipelining
  const int nparts = launch_parts(h->pipelined, stage, h->params.mts != 0, h->params.footloose != 0, (long long)h->n, range_len < 0);
  const long long half = ((h->n / 2 + 255) / 256) * 256;
  for (int part = 0; part < nparts && !rc; ++part) {
    const long long k0 = (nparts == 1) ? range_k0 : (part == 0 ? 0 : half);
    const long long klen = (nparts == 1) ? (range_len < 0 ? h->n : range_len) : (part == 0 ? half : h->n - half);
    const Redo redo{part == 0 ? h->d_redo_list : h->d_redo_list2, h->d_redo_cnt[part][h->redo_parity], k0, klen, nullptr, 0,
                    h->d_fl_cursor, h->d_iceberg_counter, (long long)h->capacity, h->gd.iec - h->gd.isc + 1, h->fl_step,
                    StageTab{h->rp.stage, h->rp.key, h->rp.mask, (long long)h->capacity}};
    rc = launch_berg_part<PH>(h, c, stage, rebin_fused ? &rtab : nullptr, redo, part, nparts);
  }
  if (nparts == 1) h->evG_live[1] = false;
  h->redo_prezeroed = false;
  if (rc) return rc;
  if (stage) return repro_fold(h, (PH & PH_THERMO) != 0, (PH & (PH_SPREAD | PH_TSPREAD)) != 0, range_k0, range_len < 0 ? h->n : range_len);
  return KID_OK;
}
// a mask whose sequence runs under both interpolation orders
template <unsigned PH>
static int launch_berg(kid_handle *h, long long range_k0 = 0, long long range_len = -1) {
  static_assert(instance_exists(true, PH, false) && instance_exists(false, PH, false), "this mask is bound to one order: launch_ordered");
  return launch_phase<PH>(h, range_k0, range_len);
}
// X under old_interp_flds_order, PH_INTERP | X under the new order (the interpolation sits inside the launch there)
template <unsigned X>
static int launch_ordered(kid_handle *h, long long range_k0 = 0, long long range_len = -1) {
  static_assert(!(X & PH_INTERP) && instance_exists(true, X, false) && instance_exists(false, PH_INTERP | X, false), "not an (old, new) pair of masks");
  return h->params.old_interp_flds_order ? launch_phase<X>(h, range_k0, range_len) : launch_phase<PH_INTERP | X>(h, range_k0, range_len);
}

// The "slow lane" schedule of the fused step (kid_set_side_stream mode 2).  The general build is a single-wave latency
// (~65 us for the few per cent of bergs that cross a cell edge or bounce) during which the chip idles.  Here it never
// sits between two hot builds: a berg the hot build of step s hands over is stepped by general-build launches on the
// side stream for steps s and s + 1 and returns to the hot build at s + 2:
//   main: prepass(s) | hot(s) ..................................... | prepass(s+1) | hot(s+1) ...
//   side:            | carry(s): step s of the bergs handed over at s-1 | new(s): step s of those handed over at s | gather(s)
// carry(s) starts with hot(s) and is long finished when hot(s+1) starts (event evC, normally already signalled);
// new(s) runs under hot(s+1), which skips its bergs (lane[k] >= s+1).  Per-step sums go to the accumulator block bound
// at launch; the caller alternates two blocks and launches the gather on the side stream (PipelinedStepper).
template <bool OLDV>
static int launch_berg_lanes(kid_handle *h) {
  constexpr unsigned PH = OLDV ? PH_STEP : (PH_INTERP | PH_STEP);
  static_assert(instance_exists(OLDV, PH, false), "the fused step of this order");
  if (need_forcing(h)) return KID_EINVAL;
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }   // (this schedule re-bins inside the step, with the copy)
  { int rc_t = refresh_tables(h); if (rc_t) return rc_t; }
  const BergLaunch c = berg_launch(h);
  h->zs.launched_berg(true, true, h->params.Runge_not_Verlet != 0, h->params.bergy_bit_erosion_fraction == 0., h->flags.has_fl != 0, false);
  hipStream_t M = h->stream, S = h->side_stream;
  const int s = h->lane_step, par = s & 1;
  rows_killed(h);
  if (h->flags.store_env || !OLDV) h->env_ever_stored = true;
  h->lanes_active = true;
  for (int q = 0; q < 2; ++q) if (h->evG_live[q] && h->pipelined) { KID_HIP(h, hipStreamWaitEvent(M, h->evG[q], 0)); h->evG_live[q] = false; }
  if (!h->redo_prezeroed) {  // no prepass: zero this step's counter here (it was last read by the previous carry-over launch)
    if (h->evC_live) KID_HIP(h, hipStreamWaitEvent(M, h->evC, 0));
    KID_HIP(h, hipMemsetAsync(h->d_redo_cnt[0][par], 0, sizeof(int), M));
  }
  int *list_new = par ? h->d_redo_list2 : h->d_redo_list, *list_old = par ? h->d_redo_list : h->d_redo_list2;
  const Redo hot{list_new, h->d_redo_cnt[0][par], 0, h->n, h->d_lane, s};
  const Redo carry{list_old, h->d_redo_cnt[0][par ^ 1], 0, h->n, nullptr, 0};
  // Every record / wait is a barrier packet of ~5 us on the stream it goes to: the main stream gets one wait (in the
  // prepass) and two records per step; with profiling on, the (start, stop) pair of the hot build doubles as the two.
  ProfilePair t;
  if (h->profile) { KID_HIP(h, hipEventCreate(&t.e0)); KID_HIP(h, hipEventCreate(&t.e1)); }
  hipEvent_t evP = h->profile ? t.e0 : h->evP, evF = h->profile ? t.e1 : h->evF[0];
  KID_HIP(h, hipEventRecord(evP, M));  // forcing records and accumulator block of this step are ready
  KID_HIP(h, hipStreamWaitEvent(S, evP, 0));
  const bool rebin_now = h->resort_interval > 0 && ++h->steps_since_sort >= h->resort_interval && !h->have_bonds && !h->dbg.stable_resort;
  int rebin_rc = KID_OK;
  auto lanes = [&](auto RK) -> int {
    constexpr bool rk = decltype(RK)::value;
    if (h->carry_valid) { const int r = launch_general<rk, OLDV, PH, false>(h, c, S, carry, h->n); if (r) return r; }
    // recorded even without a carry-over launch: everything enqueued on the side stream so far (the gather of the step
    // before last included) is complete once the next prepass has waited for it
    KID_HIP(h, hipEventRecord(h->evC, S)); h->evC_live = true;
    { const int r = launch_hot<rk, OLDV, PH, false>(h, c, M, hot); if (r) return r; }
    KID_HIP(h, hipEventRecord(evF, M));
    if (h->profile) { h->pending.emplace_back(t.e0, t.e1); h->berg_launches++; }
    if (rebin_now) {
      // re-binning inside the step: between the hot build and the general build of the bergs it handed over, whose list
      // and lanes move with the rows; nothing is drained and no latency is exposed (the carry-over launch of this step
      // is long finished, the main stream only has to say so before it moves rows)
      KID_HIP(h, hipStreamWaitEvent(M, h->evC, 0));
      rebin_rc = rebin_core(h, true, list_new, h->d_redo_cnt[0][par]);
      if (!h->evR) KID_HIP(h, hipEventCreateWithFlags(&h->evR, hipEventDisableTiming));
      KID_HIP(h, hipEventRecord(h->evR, M)); KID_HIP(h, hipStreamWaitEvent(S, h->evR, 0));
    } else KID_HIP(h, hipStreamWaitEvent(S, evF, 0));
    { const int r = launch_general<rk, OLDV, PH, false>(h, c, S, hot, h->n); if (r) return r; }
    KID_HIP(h, hipEventRecord(h->evG[0], S)); h->evG_live[0] = true;
    return KID_OK;
  };
  const int rc = h->params.Runge_not_Verlet ? lanes(std::true_type{}) : lanes(std::false_type{});
  if (rc || rebin_rc) return rc ? rc : rebin_rc;
  if (rebin_now) h->steps_since_sort = 0;
  h->carry_valid = true;
  h->lane_step = s + 1;
  h->redo_prezeroed = false;
  return KID_OK;
}

// the fused step of the handle's order, on the slow-lane schedule where it applies
static int launch_fused_step(kid_handle *h) {
  if (!lanes_eligible(h)) return launch_ordered<PH_STEP>(h);
  return h->params.old_interp_flds_order ? launch_berg_lanes<true>(h) : launch_berg_lanes<false>(h);
}

// -------------------------------------------------------------------------------------------------------
// the families of a step (IB:5409-5512), one function each
// -------------------------------------------------------------------------------------------------------
static int step_mts(kid_handle *h) {   // mts=T
  int rc = h->visited ? KID_OK : mts_first_visit(h);
  if (!rc && !h->params.static_icebergs) rc = kid_evolve_icebergs_mts(h);
  if (!rc) rc = kid_interp_gridded_fields_to_bergs(h);   // IB:5458
  if (!rc) rc = kid_set_conglom_ids(h);                  // transfer_mts_bergs, IB:5459
  if (!rc) rc = bond_orientations(h);
  return rc ? rc : launch_berg<PH_THERMO | PH_SPREAD>(h);
}
static int step_interactive(kid_handle *h) {   // single-time-step scheme with interactions
  const kid_params &p = h->params;
  const bool contact = (p.contact_distance > 0.) || (p.contact_spring_coef != p.spring_coef);
  int rc = h->visited ? KID_OK : sts_ia_first_visit(h);
  if (!rc && !p.old_interp_flds_order) rc = launch_berg<PH_INTERP>(h);
  if (!rc && !p.static_icebergs) rc = kid_evolve_icebergs_interactive(h);
  // footloose: the children are rows before the conglomerates are labelled and owe this step's thermodynamics and spreading
  // like everybody else (IB:5453); KID_ECAPACITY ends the step here, as it ends config 3's
  if (!rc && p.footloose) rc = kid_footloose_calving(h);
  if (!rc && contact) rc = kid_set_conglom_ids(h);   // IB:5470-5471
  if (!rc) rc = bond_orientations(h);
  // IB:5486 (the interpolation of IB:5473 in front of it is inside the launch below; the pass reads positions and sizes only)
  if (!rc && p.footloose) rc = kid_adjust_fl_berg_interactivity(h, nullptr);
  return rc ? rc : launch_ordered<PH_THERMO | PH_SPREAD>(h);
}
// Footloose calving sits between evolve and thermodynamics (IB:5453): fused into the per-berg launch (PH_FL), one pass over
// the SoA instead of three (SURVEY 8d: 320 B per berg-step instead of 530).  The children it appends are new rows; they
// owe this step's thermodynamics and spreading, which a second, short launch over those rows delivers.
static int step_footloose_fused(kid_handle *h) {
  { const int rc_a = auto_reserve(h, h->n + h->auto_min_free, "kid_step_local"); if (rc_a) return rc_a; }   // (one host compare while the mode is off or room is left)
  h->flags.has_fl = 1;
  KID_HIP(h, hipMemsetAsync(h->d_fl_cursor, 0, sizeof(int), h->stream));
  const long long n_old = h->n;
  int rc = launch_ordered<PH_STEP_FL>(h);
  const unsigned fl_step_now = h->fl_step;
  h->fl_step += 1u;   // one footloose pass (hot and general build of this launch share the step word)
  if (rc) return rc;
  int appended = 0;  // the population grew: the host needs the new size before the next launch
  KID_HIP(h, hipMemcpyAsync(&appended, h->d_fl_cursor, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if (appended <= h->capacity - n_old) {
    rc = fl_place_children(h, n_old, appended, fl_step_now);
    if (!rc) rc = fl_assign_ids(h, n_old, appended);
    if (rc) return rc;
  }
  rc = rows_appended(h, appended, nullptr, fl_full);
  return rc ? rc : launch_ordered<PH_THERMO | PH_SPREAD>(h, n_old, appended);
}
// phase by phase (KID_FL_UNFUSED, static bergs): three launches.  static_icebergs: evolve_icebergs is not called
// (IB:5428-5436); the calving that follows still is (IB:5453)
static int step_footloose_phases(kid_handle *h) {
  int rc = h->params.static_icebergs ? launch_berg<PH_INTERP>(h) : launch_berg<PH_INTERP | PH_EVOLVE>(h);
  if (!rc) rc = kid_footloose_calving(h);
  return rc ? rc : launch_berg<PH_INTERP | PH_THERMO | PH_SPREAD>(h);
}
// find_melt_using_spread_mass, IB:5490-5503: the gridded mass BEFORE the thermodynamics (calculate_mass_on_ocean without
// diagnostics, the 'mass' gather into grd%spread_mass_old, planes reset), then thermodynamics + create_gridded_icebergs_fields
// as usual; the gather replaces floating_melt by (spread_mass_old - spread_mass)/dt (IB:3436-3445)
static int step_spread_mass(kid_handle *h) {
  const kid_params &p = h->params;
  if (!h->d_spread_mass_old) {
    KID_HIP(h, h->mem.dev(h->d_spread_mass_old_own, 2 * h->ncell, 0));   // + spread_mass_tmp
    h->d_spread_mass_old = h->d_spread_mass_old_own;
  }
  int rc = KID_OK;
  if (!p.static_icebergs) { rc = p.old_interp_flds_order ? launch_berg<PH_EVOLVE>(h) : launch_berg<PH_INTERP | PH_EVOLVE>(h); if (rc) return rc; }
  rc = zero_planes(h, ON_OCEAN_ALL);
  if (rc) return rc;
  const Flags keep = h->flags;
  h->flags.no_diag = 1; h->flags.footprint = 0;
  rc = launch_berg<PH_SPREAD>(h);
  h->flags = keep;
  if (!rc) rc = gather_mass_and_reset(h, h->d_spread_mass_old);
  if (rc) return rc;
  if (!p.Iceberg_melt_without_decay) return launch_ordered<PH_THERMO | PH_SPREAD>(h);
  // the bergs do not decay, so the gridded mass AFTER the melt is what thermodynamics itself spreads (IB:3219-3238);
  // it is gathered into spread_mass_tmp (IB:3411-3413) before create_gridded_icebergs_fields spreads the unchanged bergs
  rc = launch_ordered<PH_THERMO | PH_TSPREAD>(h);
  if (!rc) rc = gather_mass_and_reset(h, h->d_spread_mass_old + h->ncell);
  return rc ? rc : launch_berg<PH_SPREAD>(h);
}
static int step_default(kid_handle *h) {
  const kid_params &p = h->params;
  // New order, IB:5423: interpolate, evolve; IB:5473: interpolate again at the new position, then thermodynamics.  Per berg
  // that is one chain, so one launch (the second interpolation sits between the phases inside berg_kernel), unless
  // KID_NEW_ORDER_UNFUSED asks for the two halves (which gives way to the slow-lane schedule)
  const bool old = p.old_interp_flds_order != 0;
  if (!p.static_icebergs && (old || !h->dbg.new_order_unfused || lanes_eligible(h))) return launch_fused_step(h);
  if (old) return launch_berg<PH_THERMO | PH_SPREAD>(h);   // static_icebergs: evolve_icebergs is not called (IB:5428)
  const int rc = p.static_icebergs ? launch_berg<PH_INTERP>(h) : launch_berg<PH_INTERP | PH_EVOLVE>(h);
  return rc ? rc : launch_berg<PH_INTERP | PH_THERMO | PH_SPREAD>(h);
}

extern "C" {

int kid_interp_gridded_fields_to_bergs(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_interp_gridded_fields_to_bergs"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  int rc = launch_berg<PH_INTERP>(h);
  if (rc || !h->params.mts) return rc;
  return mts_depth(h);
}
int kid_evolve_icebergs(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  if (h->params.static_icebergs) return KID_OK;  // IB:5428
  { const int rc_r = repro_refuse(h); if (rc_r) return rc_r; }
  if (h->params.mts) return kid_evolve_icebergs_mts(h);  // IB:5431
  if (h->params.interactive_icebergs_on) return kid_evolve_icebergs_interactive(h);
  return launch_berg<PH_EVOLVE>(h);
}
int kid_thermodynamics(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_thermodynamics"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  // find_melt_using_spread_mass: the gridded mass before the melt (grd%spread_mass_old, IB:5490-5503) is gathered inside
  // kid_step_local only; without it the gather would hand back the bergs' own melt as if the switch were off
  if (h->params.find_melt_using_spread_mass && (!h->d_spread_mass_old || h->d_spread_mass_old == h->d_spread_mass_old_own)) {
    h->err = "find_melt_using_spread_mass: the phase entry points do not gather spread_mass_old (IB:5490-5503); use kid_run_step / kid_step_local";
    return KID_EUNSUPPORTED;
  }
  const int rc = zero_planes(h, ON_OCEAN_VEL);   // IB:2872-2873
  return rc ? rc : launch_berg<PH_THERMO>(h);
}
int kid_create_gridded_icebergs_fields(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_create_gridded_icebergs_fields"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  int rc = zero_planes(h, ON_OCEAN_ALL);   // IB:4984-4987
  if (!rc) rc = launch_berg<PH_SPREAD>(h);
  return rc ? rc : launch_gather(h);
}

int kid_step_local(kid_handle *h) {   // IB:5409-5512
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_step_local"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  int rc = h->acc_prezeroed ? KID_OK : kid_zero_accumulators(h);  // kid_step_prepare has done it for this step
  h->acc_prezeroed = false;
  if (!rc) rc = repro_refuse(h);
  // a pending re-binning waits for the one launch that can take it (the plain fused step); every other kind of step copies first
  if (!rc && h->rebin_pending && !rebin_fusable(h)) rc = rebin_flush(h);
  if (!rc && !rebin_fusable(h)) rc = cold_materialise(h);   // (the other families launch kernels that read any field by row)
  if (rc) return rc;
  const kid_params &p = h->params;
  if (p.mts) return step_mts(h);
  if (p.interactive_icebergs_on) return step_interactive(h);
  if (p.footloose) return (!p.static_icebergs && !h->dbg.fl_unfused) ? step_footloose_fused(h) : step_footloose_phases(h);
  if (p.find_melt_using_spread_mass) return step_spread_mass(h);
  return step_default(h);
}
int kid_step_gather(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_step_gather"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  return launch_gather(h);
}
int kid_run_step(kid_handle *h, int nsteps) {
  if (!h || nsteps < 0) return KID_EINVAL;
  for (int s = 0; s < nsteps; ++s) {
    int rc = kid_step_local(h);
    if (rc) return rc;
    rc = kid_step_gather(h);
    if (rc) return rc;
    if (!h->lanes_active && !h->params.mts && !h->params.interactive_icebergs_on && h->resort_interval > 0 && ++h->steps_since_sort >= h->resort_interval) {  // IB:5437, amortised; bonded bergs keep their rows
      rc = kid_move_berg_between_cells(h);
      if (rc) return rc;
    }
  }
  return KID_OK;
}

}  // extern "C"
