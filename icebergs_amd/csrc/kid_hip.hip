// kid_hip.hip -- the translation unit of libkid_hip.so (gfx950 / MI355X).  See include/kid.h.  This file keeps the handle's life
// cycle (kid_create, kid_destroy, streams), the parameters and the device tables (refresh_tables), upload and download of the
// bergs, footloose calving, and the list of .inc files that hold everything else.
//
// Data layout in HBM
//   bergs   : structure of arrays, one contiguous fp64/int32 array of `capacity` elements per field of the
//             reference's `type iceberg` (FW:290-359), in reference traversal order (cell-major).
//   grid    : the 11 static + 11 forcing planes as the host passes them, plus the packed per-cell records (kid_cells.inc).
//   accum   : KID_NACC planes of ni*nj fp64 + KID_NSCALAR scalars in ONE block (one RCCL all-reduce per step),
//             followed by KID_NOUT derived planes (kid_planes.hpp, kid_cells.inc).
// Kernels: berg_kernel<RK,OLD,PH> (kid_berg_kernel.hpp), one lane per berg, PH selects interp / evolve / thermodynamics /
// spreading, so the reference's phase-by-phase call sites and the fused per-step launch share one body; per cell, kid_cells.inc.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "../../include/kid.h"
#include "kid_device.hpp"
#include "kid_thermo.hpp"
#include "kid_footloose.hpp"
#include "kid_berg_kernel.hpp"
#include "kid_rows_plan.hpp"
#include "kid_fl_contact.hpp"
#include "kid_reserve_plan.hpp"
#include "kid_check_plan.hpp"

using namespace kid;

// the plain hot build of the fused RK4 step: its own translation unit in the product build (kid_hot_plain.hip, another machine
// scheduler), included here in a one-file build
#ifdef KID_HOT_PLAIN_SEPARATE
namespace kid { void launch_hot_plain(bool store_env, bool rebin, unsigned nblocks, void *stream, const DevGrid *gtab, const kid_params *pp, const void *bp, long long n,
                                      double *acc, size_t ncell, const void *flags, const void *redo); }
#else
#include "kid_hot_plain.inc"
#endif

namespace {

// footloose_calving (IB:2503-2734): streaming pass, one lane per berg that existed when the pass started
__global__ void __launch_bounds__(256) footloose_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                        const FlChildCtx cx, double *__restrict__ acc, const size_t ncell) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= cx.n) return;
  const BergPtrs &b = *bt;
  if (b.i[KID_BI_ALIVE][q] == 0) return;
  footloose_one(g, *pp, b, cx, q, acc, ncell, acc - KID_NSCALAR);
}

// the device-side tables are rewritten by stream-ordered one-lane kernels (the new contents travel as kernel arguments):
// no host synchronisation, unlike a copy from pageable memory
__global__ void set_berg_table_kernel(const BergPtrs src, BergPtrs *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_rebin_table_kernel(const RebinTab src, RebinTab *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_params_kernel(const kid_params src, kid_params *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_time_kernel(int32_t year, double yearday, kid_params *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) { dst->current_year = year; dst->current_yearday = yearday; } }

#include "kid_mts.inc"
#include "kid_fl_interact.inc"

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
#include "kid_handle.hpp"

// Halo rows (kid_halo_bergs.inc) are force sources for one kid_evolve_icebergs and nothing else: between the unpack that
// brought them and the evolve that retires them, whatever would melt, spread, count, move or write them out is refused.
static int halo_rows_refuse(kid_handle *h, const char *what) {
  if (!h->halo_rows_live) return KID_OK;
  h->err = std::string(what) + ": halo rows are resident (copies of the neighbours' bergs, kid_unpack_immigrants); the next kid_evolve_icebergs retires them";
  return KID_EINVAL;
}
#include "kid_cells.inc"

static int check_params(kid_handle *h, const kid_params *p) {
  if (p->dem && !p->mts) { h->err = "dem needs mts=T (the DEM forces live on the MTS sub-steps)"; return KID_EINVAL; }
  if (p->mts) {
    if (p->Runge_not_Verlet) { h->err = "Runge_not_Verlet must be false to use MTS or DEM (FW:1485-1490)"; return KID_EINVAL; }
    if (p->old_interp_flds_order) { h->err = "old_interp_flds_order is false whenever mts/dem is on (FW:1483)"; return KID_EINVAL; }
    if (p->mts_sub_steps < 1) { h->err = "mts_sub_steps must be >= 1 (pass the value ice_bergs_framework_init derives, FW:1296-1301)"; return KID_EINVAL; }
    if (p->dem && !p->explicit_inner_mts) { h->err = "dem forces explicit_inner_mts=T (FW:1433)"; return KID_EINVAL; }
    if (p->dem && !p->iceberg_bonds_on) { h->err = "dem needs iceberg_bonds_on"; return KID_EINVAL; }
    if (p->max_bonds < 1 || p->max_bonds > KID_MAX_BONDS) { h->err = "max_bonds out of range"; return KID_EINVAL; }
    if (p->use_broken_bonds_for_substep_contact && !(p->break_bonds_on_sub_steps && p->dem && p->iceberg_bonds_on)) {
      h->err = "use_broken_bonds_for_substep_contact requires break_bonds_on_sub_steps, dem and iceberg_bonds_on (FW:1438-1447)"; return KID_EINVAL; }
    if (p->footloose) { h->err = "footloose together with mts is not implemented"; return KID_EUNSUPPORTED; }
  } else if (p->interactive_icebergs_on || p->iceberg_bonds_on) {
    // footloose children among interacting bergs: kid_fl_interact.inc.  With bonds a bonded edge element that would calve is the
    // reference's own FATAL (IB:2566-2569, 2585)
    if (p->footloose && p->iceberg_bonds_on) { h->err = "footloose together with iceberg_bonds_on: bonded footloose calving (edge elements that calve, IB:2566-2585) is not implemented"; return KID_EUNSUPPORTED; }
    if (p->iceberg_bonds_on && !p->interactive_icebergs_on) { h->err = "iceberg_bonds_on without interactive_icebergs_on is not implemented"; return KID_EUNSUPPORTED; }
    if (p->max_bonds < 1 || p->max_bonds > KID_MAX_BONDS) { h->err = "max_bonds out of range"; return KID_EINVAL; }
  }
  if (p->tidal_drift > 0.) { h->err = "tidal_drift needs FMS's random stream: not supported"; return KID_EUNSUPPORTED; }
  // time_average_weight=T is accepted: the spreading it moves into the integrator stages (IB:7264, 7395, 7433, 7490, 7620)
  // fills mass/area/Uvel/Vvel_on_ocean, but calculate_mass_on_ocean zeroes those planes again (IB:4984-4987) without
  // refilling them (IB:4997), and nothing reads them in between: the reference's spread_mass is identically zero in
  // this mode.  So the stage spreading is not launched and the spreading phase skips the berg (berg_kernel, PH_SPREAD).
  if (p->find_melt_using_spread_mass && (p->mts || p->interactive_icebergs_on || p->footloose)) {
    h->err = "find_melt_using_spread_mass is implemented for the plain evolve loop only (no bonds, interactions or footloose)";
    return KID_EUNSUPPORTED;
  }
  if (p->Runge_not_Verlet && p->footloose) { h->err = "Runge_not_Verlet must be false to use footloose (FW:1485-1490)"; return KID_EINVAL; }
  if (p->footloose && !p->use_operator_splitting) { h->err = "use_operator_splitting must be true to use footloose (FW:1476)"; return KID_EINVAL; }
  return KID_OK;
}

extern "C" {

// The build's arithmetic and measurement switches are part of its identity: a library built with -DKID_EXPERIMENTS (KID_EXP_*
// measurement macros, possibly wrong answers) or -DKID_EXACT_MATH (IEEE division/sqrt/pow everywhere) says so.
#ifndef KID_BUILD_ID
#define KID_BUILD_ID "unknown"
#endif
// "src <id>": the first 12 hex digits of the SHA-1 of the library's sources (csrc/Makefile): profiles name the build they measured
const char *kid_version(void) {
  return "kid_hip 0.3 (gfx950) src " KID_BUILD_ID
#ifdef KID_EXACT_MATH
         " exact-math"
#endif
#ifdef KID_EXPERIMENTS
         " EXPERIMENTS"
#endif
      ;
}
int64_t kid_sizeof(int which) {
  switch (which) { case 0: return (int64_t)sizeof(kid_params); case 1: return (int64_t)sizeof(kid_grid_desc);
                   case 2: return (int64_t)sizeof(kid_berg_soa); case 3: return (int64_t)sizeof(kid_bond_soa);
                   case 4: return (int64_t)sizeof(kid_forcing_in);
                   case 5: return (int64_t)sizeof(kid_calving_params); case 6: return (int64_t)sizeof(kid_calving_in); default: return -1; }
}
#ifdef KID_EXP_TIMING
// measurement build only: the segment clock of the per-berg kernels (kid_device.hpp, KID_TICK); out[0] = waves, out[1+n] = cycles of segment n
int kid_exp_timing(unsigned long long *out, int reset) {
  if (out) {
    std::vector<unsigned long long> all((size_t)KID_TPROF_WAVES * 16);
    if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(kid_tprof), all.size() * sizeof(unsigned long long)) != hipSuccess) return KID_EHIP;
    for (int q = 0; q < 16; ++q) out[q] = 0ull;
    for (size_t r = 0; r < (size_t)KID_TPROF_WAVES; ++r) for (int q = 0; q < 16; ++q) out[q] += all[r * 16 + q];
  }
  if (reset) {
    void *sym = nullptr;
    if (hipGetSymbolAddress(&sym, HIP_SYMBOL(kid_tprof)) != hipSuccess || hipMemset(sym, 0, (size_t)KID_TPROF_WAVES * 16 * sizeof(unsigned long long)) != hipSuccess) return KID_EHIP;
  }
  return KID_OK;
}
#endif
// kid_destroy reports a failed free through kid_last_error(NULL), to the thread that called it: the handle is gone by then
static thread_local std::string destroy_err;
const char *kid_last_error(const kid_handle *h) { return h ? h->err.c_str() : destroy_err.empty() ? "null handle" : destroy_err.c_str(); }

int kid_create(const kid_grid_desc *grid, const kid_params *params, int64_t capacity, int device, kid_handle **out) {
  if (!grid || !params || !out || capacity <= 0) return KID_EINVAL;
  if (capacity > (int64_t(1) << 29)) return KID_EINVAL;   // the per-berg kernel addresses a row by a 32-bit byte offset (2^29 rows of 8 bytes; 240 GB of berg state)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KID_ENODEV;
  if (device < 0 || device >= ndev) return KID_ENODEV;
  kid_handle *h = new kid_handle();
  *out = h;  // returned even on failure so that kid_last_error() can be read; caller still destroys it
  h->device = device;
  KID_HIP(h, hipSetDevice(device));
  h->gd = *grid;
  h->ni = grid->ied - grid->isd + 1; h->nj = grid->jed - grid->jsd + 1;
  if (h->ni < 5 || h->nj < 5 || grid->isc - grid->isd < 2 || grid->ied - grid->iec < 2 || grid->jsc - grid->jsd < 2 || grid->jed - grid->jec < 2) {
    h->err = "grid needs a halo of at least 2 cells"; return KID_EINVAL;
  }
  h->ncell = (size_t)h->ni * (size_t)h->nj;
  int rc = check_params(h, params);
  if (rc) return rc;
  h->params = *params;
  h->flags.footprint = footprint_needed(h->params) ? 1 : 0;
  h->capacity = capacity;
  if (getenv("KID_MTS_NO_GRAPH")) h->use_graph = false;  // A/B switch for measurements
  h->dbg.stable_resort = getenv("KID_STABLE_RESORT") != nullptr; h->dbg.no_plain_build = getenv("KID_NO_PLAIN_BUILD") != nullptr;
  h->dbg.fl_unfused = getenv("KID_FL_UNFUSED") != nullptr; h->dbg.new_order_unfused = getenv("KID_NEW_ORDER_UNFUSED") != nullptr;
  h->dbg.rebin_eager = getenv("KID_REBIN_EAGER") != nullptr; h->dbg.chksum_timing = getenv("KID_CHKSUM_TIMING") != nullptr;
  h->dbg.no_zero_skip = getenv("KID_NO_ZERO_SKIP") != nullptr; h->dbg.cold_eager = getenv("KID_COLD_EAGER") != nullptr;
  h->dbg.mts_always_label = getenv("KID_MTS_ALWAYS_LABEL") != nullptr; h->dbg.mts_no_fused = getenv("KID_MTS_NO_FUSED") != nullptr;
  if (const char *e = getenv("KID_MTS_FUSED_BLOCKS_CAP")) h->dbg.mts_fused_blocks_cap = atoi(e);
  if (const char *e = getenv("KID_MTS_POLL_LIMIT")) h->dbg.mts_poll_limit = atoi(e);
  KID_HIP(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  const size_t cap = (size_t)capacity;
  for (auto &plane : h->d_static) KID_HIP(h, h->mem.dev(plane, h->ncell, 0));
  for (auto &plane : h->d_forcing) KID_HIP(h, h->mem.dev(plane, h->ncell, 0));
  for (ForcingSet &fs : h->fset) {
    KID_HIP(h, h->mem.dev(fs.vel, h->ncell)); KID_HIP(h, h->mem.dev(fs.trc, h->ncell)); KID_HIP(h, h->mem.dev(fs.d_grid, 1));
    KID_HIP(h, h->mem.dev(fs.pkt, h->ncell * PK_GSTRIDE, 0));
  }
  KID_HIP(h, h->mem.dev(h->d_geo, h->ncell));
  KID_HIP(h, h->mem.dev(h->d_hotok, h->ncell, 0));
  if (grid->grid_is_latlon) KID_HIP(h, h->mem.dev(h->d_latref, 2 * h->ncell));   // DevGrid::latref
  KID_HIP(h, h->mem.dev(h->d_acc_own, (size_t)KID_NACC * h->ncell + KID_NSCALAR, 0));
  h->d_acc = h->d_acc_own + KID_NSCALAR;
  KID_HIP(h, h->mem.dev(h->d_out, (size_t)KID_NOUT * h->ncell, 0));
  KID_HIP(h, h->mem.dev(h->d_totals, KID_NSCALAR, 0));
  for (auto &field : h->bp.f) KID_HIP(h, h->mem.dev(field, cap, 0));
  for (auto &field : h->bp.i) KID_HIP(h, h->mem.dev(field, cap, 0));
  KID_HIP(h, h->mem.dev(h->bp.id, cap, 0));
  KID_HIP(h, h->mem.dev(h->d_bp, 1));
  KID_HIP(h, h->mem.dev(h->d_rb, 1));
  KID_HIP(h, h->mem.dev(h->d_params, 1));
  KID_HIP(h, h->mem.dev(h->d_lane, cap, 0));
  KID_HIP(h, h->mem.dev(h->d_count, 4));
  KID_HIP(h, h->mem.dev(h->d_iceberg_counter, h->ncell, 0));
  KID_HIP(h, h->mem.dev(h->d_fl_cursor, 1));
  for (int **q : {&h->d_redo_list, &h->d_redo_list2}) KID_HIP(h, h->mem.dev(*q, cap));
  KID_HIP(h, h->mem.dev(h->d_redo_count2, 4, 0));
  for (int part = 0; part < 2; ++part) for (int par = 0; par < 2; ++par) h->d_redo_cnt[part][par] = h->d_redo_count2 + (2 * part + par);
  for (hipEvent_t *e : {&h->evC, &h->evP, &h->evF[0], &h->evF[1], &h->evG[0], &h->evG[1]}) KID_HIP(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (hipEvent_t *e : {&h->ev0, &h->ev1, &h->ev2, &h->ev3}) KID_HIP(h, hipEventCreate(e));
  // The zero-fills above are on the handle's own stream.  kid_set_stream may name another one before the first upload,
  // and that stream does not order itself behind this one: wait here, or a fill could land after the upload (seen once,
  // with null-stream fills, as a zeroed `ine` array of a 1-berg population).
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_destroy(kid_handle *h) {
  if (!h) return KID_EINVAL;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  if (h->sub_graph_exec) (void)hipGraphExecDestroy(h->sub_graph_exec);
  for (hipEvent_t e : {h->evR, h->evC, h->evP, h->evF[0], h->evF[1], h->evG[0], h->evG[1], h->ev0, h->ev1, h->ev2, h->ev3}) if (e) (void)hipEventDestroy(e);
  for (auto &pe : h->pending) { (void)hipEventDestroy(pe.first); (void)hipEventDestroy(pe.second); }
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  const int e_rp = h->rp_mem.free_all(), e_mem = h->mem.free_all();
  const hipError_t e = (hipError_t)(e_rp ? e_rp : e_mem);
  delete h;
  if (e == hipSuccess) return KID_OK;
  destroy_err = std::string("kid_destroy: freeing the handle's memory: ") + hipGetErrorString(e);
  return KID_EHIP;
}

int kid_memory_in_use(int64_t *device_bytes, int64_t *pinned_bytes) {
  if (device_bytes) *device_bytes = kid::mem_in_use(kid::MEM_DEVICE).load();
  if (pinned_bytes) *pinned_bytes = kid::mem_in_use(kid::MEM_PINNED).load();
  return KID_OK;
}

int kid_set_params(kid_handle *h, const kid_params *params) {
  if (!h || !params) return KID_EINVAL;
  int rc = check_params(h, params);
  if (rc) return rc;
  if (!h->tables_dirty && h->d_params) {
    // A model clock that advances (bergs%current_year / current_yearday, every step of a real run) is not a reason to
    // rebuild the device tables -- which waits for the side stream, i.e. puts the slow lane's general build back between
    // two hot builds.  The two words are written in place by a stream-ordered one-lane kernel; the launches that may
    // still be in flight on the side stream (fused step without footloose) never read them.
    kid_params a = h->params, b = *params;
    a.current_year = b.current_year = 0; a.current_yearday = b.current_yearday = 0.;
    if (std::memcmp(&a, &b, sizeof(kid_params)) == 0) {
      h->params = *params;
      KID_HIP(h, hipSetDevice(h->device));
      hipLaunchKernelGGL(set_time_kernel, dim3(1), dim3(64), 0, h->stream, params->current_year, params->current_yearday, h->d_params);
      KID_HIP(h, hipGetLastError());
      return KID_OK;
    }
  }
  h->params = *params;
  h->tables_dirty = true;
  h->labels_stale = true;   // (the conglomerate labelling reads dem / max_bonds / use_broken_bonds_for_substep_contact)
  h->flags.footprint = footprint_needed(h->params) ? 1 : 0;
  if (!h->params.old_interp_flds_order && !h->env_off_requested) h->flags.store_env = 1;  // the stored environment is an input again
  return cold_settle(h);   // the new namelist may read a field that is deferred as cold
}
// order the main stream behind general-build launches that are still in flight on the side stream
static int join_side(kid_handle *h) {
  for (int q = 0; q < 2; ++q)
    if (h->evG_live[q]) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evG[q], 0)); }
  if (h->evC_live) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evC, 0)); }
  return KID_OK;
}
// Leave the slow-lane schedule: both lanes are complete through the last step once the side stream is joined, so every
// berg can go back to the hot build and nothing is carried over.  Needed before anything that moves rows (the lists
// hold row numbers) or that launches outside launch_berg_lanes (kid_launch.inc).
static int lanes_drain(kid_handle *h) {
  const int rc = join_side(h);
  if (rc || !h->lanes_active) return rc;
  KID_HIP(h, hipMemsetAsync(h->d_lane, 0, (size_t)h->capacity * sizeof(int), h->stream));
  // the other buffer of the in-step re-binning too: its rows beyond the population would come back with stamps of a
  // step count that starts over below
  if (h->d_lane_alt) KID_HIP(h, hipMemsetAsync(h->d_lane_alt, 0, (size_t)h->capacity * sizeof(int), h->stream));
  h->lanes_active = false; h->carry_valid = false; h->lane_step = 1;
  return KID_OK;
}
int kid_set_side_stream(kid_handle *h, void *s, int enable) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  int rc = join_side(h);
  if (rc) return rc;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  { const int rc_d = lanes_drain(h); if (rc_d) return rc_d; }
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->evG_live[0] = h->evG_live[1] = false; h->evC_live = false;
  h->side_stream = (hipStream_t)s;
  h->pipelined = enable == 1;
  h->side_mode = (s && enable == 2) ? 2 : 0;
  return KID_OK;
}
int kid_set_stream(kid_handle *h, void *s) {
  if (!h) return KID_EINVAL;
  // NULL is the device's default (null) stream -- e.g. torch's default current stream -- not "no stream": work the
  // caller orders with its own events or collectives must really be on the stream it names
  h->stream = (hipStream_t)s;
  return KID_OK;
}
// the cell hash of a berg id (ij_component_of_id FW:4227-4240) on this grid: i + iNg * (j - 1) + ij0 with local i, j
static inline int id_iNg(const kid_grid_desc &d) { return d.gni > 0 ? d.gni : d.iec - d.isc + 1; }
static inline int id_ij0(const kid_grid_desc &d) { return d.gni > 0 ? d.gi0 + d.gni * d.gj0 : 0; }
int kid_sync(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return mts_check_timeout(h);
}

#include "kid_ingest.inc"
}  // extern "C"
#include "kid_rows.inc"
extern "C" {

int kid_upload_bergs(kid_handle *h, const kid_berg_soa *host) {
  if (!h || !host || host->n < 0) return KID_EINVAL;
  if (host->n > h->capacity) { const int rc = auto_reserve(h, host->n, "kid_upload_bergs"); if (rc) return rc; }
  if (host->n > h->capacity) { h->err = "more bergs than capacity"; return KID_ECAPACITY; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  const size_t n = (size_t)host->n;
  for (int f = 0; f < KID_NB_F64; ++f) {
    if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(h->bp.f[f], host->f64[f], n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else KID_HIP(h, hipMemsetAsync(h->bp.f[f], 0, n * sizeof(double), h->stream));
  }
  for (int f = 0; f < KID_NB_I32; ++f) {
    if (host->i32[f]) KID_HIP(h, hipMemcpyAsync(h->bp.i[f], host->i32[f], n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    else if (f == KID_BI_ALIVE) { if (n) hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->bp.i[f], 1, (long long)n); }
    else KID_HIP(h, hipMemsetAsync(h->bp.i[f], 0, n * sizeof(int32_t), h->stream));
  }
  if (host->id) KID_HIP(h, hipMemcpyAsync(h->bp.id, host->id, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  else KID_HIP(h, hipMemsetAsync(h->bp.id, 0, n * sizeof(int64_t), h->stream));
  // cell indices are trusted by the kernels: reject anything outside the computational domain + first halo row
  if (host->i32[KID_BI_INE] && host->i32[KID_BI_JNE]) {
    for (size_t k = 0; k < n; ++k) {
      const int i = host->i32[KID_BI_INE][k], j = host->i32[KID_BI_JNE][k];
      if (i < h->gd.isc - 1 || i > h->gd.iec + 1 || j < h->gd.jsc - 1 || j > h->gd.jec + 1) {
        h->err = "berg cell index (ine,jne) outside the computational domain"; return KID_EINVAL;
      }
    }
  } else if (n > 0) { h->err = "ine/jne are required"; return KID_EINVAL; }
  if (h->bp.orient) { h->bp.orient = nullptr; h->tables_dirty = true; }
  rows_replaced(h, host);
  h->visited = false; h->have_bonds = false;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_download_bergs(kid_handle *h, kid_berg_soa *host) {
  if (!h || !host) return KID_EINVAL;
  if (host->n < h->n) { h->err = "host SoA too small"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  const size_t n = (size_t)h->n;
  for (int f = 0; f < KID_NB_F64; ++f)
    if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(host->f64[f], h->bp.f[f], n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  for (int f = 0; f < KID_NB_I32; ++f)
    if (host->i32[f]) KID_HIP(h, hipMemcpyAsync(host->i32[f], h->bp.i[f], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (host->id) KID_HIP(h, hipMemcpyAsync(host->id, h->bp.id, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  host->n = h->n;
  return KID_OK;
}

// With .not.old_interp_flds_order the stored environment (berg%uo ... od) is an input of evolve_icebergs and thermodynamics as
// the reference calls them, one after the other; the fused step (kid_run_step / kid_step_local) interpolates it for itself
// and only writes it -- 104 B per berg-step that nothing inside the library reads back.  Switching the store off is
// therefore allowed there too; the entry points that do read it then refuse to run (launch_phase, kid_launch.inc) instead of reading values
// of some earlier step.
int kid_set_store_environment(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  h->flags.store_env = on ? 1 : 0;
  h->env_off_requested = !on;
  return cold_settle(h);
}

static int refresh_tables(kid_handle *h) {
  if (h->tables_dirty) {
    const int rc = join_side(h);  // a general-build launch on the side stream may still be reading the tables
    if (rc) return rc;
    hipLaunchKernelGGL(set_berg_table_kernel, dim3(1), dim3(64), 0, h->stream, h->bp, h->d_bp);
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(64), 0, h->stream, h->params, h->d_params);
    for (int par = 0; par < 2; ++par) hipLaunchKernelGGL(set_grid_kernel, dim3(1), dim3(64), 0, h->stream, dev_grid(h, par), h->fset[par].d_grid);
    KID_HIP(h, hipGetLastError());
    h->tables_dirty = false;
  }
  return KID_OK;
}
// ids of the children a footloose pass appended to rows [n_old, n_old + m): the per-cell counter values in the order the
// reference's loop would have met the events (kid_footloose.hpp, fl_assign_ids_*)
// second half of calve_fl_icebergs for the children of one pass (kid_footloose.hpp): positions, copied members, constants
static int fl_place_children(kid_handle *h, long long n_old, int m, unsigned step) {
  if (!h->fl_place_warm) {   // the kernel's out-of-line helpers need stack scratch, which the runtime allocates at the FIRST launch
    // (1.6 s at 1e7 bergs' worth of device memory in use): an empty launch at the first footloose pass, not at the first event
    h->fl_place_warm = true;
    hipLaunchKernelGGL(fl_place_children_kernel<BergPtrs>, dim3(1), dim3(64), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, n_old, 0, step);
    KID_HIP(h, hipGetLastError());
  }
  if (m <= 0) return KID_OK;
  hipLaunchKernelGGL(fl_place_children_kernel<BergPtrs>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, n_old, m, step);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static int fl_assign_ids(kid_handle *h, long long n_old, int m) {
  if (m <= 0) return KID_OK;
  if (!h->d_fl_head) KID_HIP(h, h->mem.dev(h->d_fl_head, h->ncell, 0xff));   // -1: empty lists
  if (m > h->fl_ev_capacity) {
    KID_HIP(h, h->mem.drop(h->d_fl_next));
    KID_HIP(h, h->mem.drop(h->d_fl_newid));
    h->fl_ev_capacity = std::max<long long>(2ll * m, 4096);
    KID_HIP(h, h->mem.dev(h->d_fl_next, (size_t)h->fl_ev_capacity));
    KID_HIP(h, h->mem.dev(h->d_fl_newid, (size_t)h->fl_ev_capacity));
  }
  const FlIdCtx x{h->d_fl_head, h->d_fl_next, h->d_fl_newid, h->d_iceberg_counter, n_old, m, id_iNg(h->gd), id_ij0(h->gd)};
  const dim3 grid((unsigned)((m + 255) / 256)), block(256);
  const DevGrid g = dev_grid(h);
  hipLaunchKernelGGL(fl_assign_ids_push<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  hipLaunchKernelGGL(fl_assign_ids_rank<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  hipLaunchKernelGGL(fl_assign_ids_store<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static const char *const fl_full = "footloose calving ran out of capacity: create the handle with room for child bergs";
int kid_footloose_calving(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_footloose_calving"); if (rc_h) return rc_h; }
  if (!h->params.footloose || h->n == 0) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  int rc = repro_refuse(h);
  if (rc) return rc;
  rc = rebin_flush(h);
  if (rc) return rc;
  rc = refresh_tables(h);
  if (rc) return rc;
  h->flags.has_fl = 1;
  h->zs.launched_other();   // (parents lose their bits, children copy what their parents hold)
  // auto-reserve: min_free rows behind the parents before the launch (no retry afterwards: the parents' bits are spent by then)
  rc = auto_reserve(h, h->n + h->auto_min_free, "kid_footloose_calving");
  if (rc) return rc;
  KID_HIP(h, hipMemsetAsync(h->d_fl_cursor, 0, sizeof(int), h->stream));
  const unsigned fl_step_now = h->fl_step;
  FlChildCtx cx{h->d_fl_cursor, h->d_iceberg_counter, (long long)h->n, (long long)h->capacity, h->gd.iec - h->gd.isc + 1, h->fl_step++};
  hipLaunchKernelGGL(footloose_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->d_bp, cx, h->d_acc, h->ncell);
  KID_HIP(h, hipGetLastError());
  int appended = 0;  // the population grew: the host needs the new size before the next launch
  KID_HIP(h, hipMemcpyAsync(&appended, h->d_fl_cursor, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  // the children become rows only once they are placed and have their ids: after a failure of either helper the population is
  // what it was before the call
  if (appended <= h->capacity - h->n) {
    rc = fl_place_children(h, h->n, appended, fl_step_now);
    if (!rc) rc = fl_assign_ids(h, h->n, appended);
    if (rc) return rc;
  }
  return rows_appended(h, appended, nullptr, fl_full);
}
double kid_footloose_uniform(int32_t seed, int64_t berg_id, int64_t step, int32_t draw) {   // the number a child placement uses (host side of kid_rng.h)
  return kid_fl_uniform((uint32_t)seed, berg_id, (uint32_t)step, (uint32_t)draw);
}
int kid_set_footloose_step(kid_handle *h, int64_t step) {   // restart: continue the child-placement sequence (kid_rng.h)
  if (!h || step < 0) return KID_EINVAL;
  h->fl_step = (unsigned)step;
  return KID_OK;
}
int kid_get_footloose_step(kid_handle *h, int64_t *step) {
  if (!h || !step) return KID_EINVAL;
  *step = (int64_t)h->fl_step;
  return KID_OK;
}
int kid_set_iceberg_counter(kid_handle *h, const int32_t *counter) {  // grd%iceberg_counter_grd, (isd:ied,jsd:jed)
  if (!h || !counter) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipMemcpy(h->d_iceberg_counter, counter, h->ncell * sizeof(int32_t), hipMemcpyHostToDevice));
  return KID_OK;
}
int kid_get_iceberg_counter(kid_handle *h, int32_t *counter) {
  if (!h || !counter) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  KID_HIP(h, hipMemcpy(counter, h->d_iceberg_counter, h->ncell * sizeof(int32_t), hipMemcpyDeviceToHost));
  return KID_OK;
}

#include "kid_mts_host.inc"
#include "kid_calving.inc"
#include "kid_repro.inc"
}  // extern "C"
#include "kid_bond_init.inc"
#include "kid_budget.inc"
#include "kid_launch.inc"
#include "kid_reserve.inc"
extern "C" {

int kid_last_redo_count(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  int c[4] = {0, 0, 0, 0};
  KID_HIP(h, hipMemcpyAsync(c, h->d_redo_count2, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  *count = (int64_t)c[0 + h->redo_parity] + (h->pipelined ? (int64_t)c[2 + h->redo_parity] : 0);
  return KID_OK;
}
int kid_rebin_fused_count(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  *count = h->rebin_fused_count;
  return KID_OK;
}
int kid_hot_zero_mask(kid_handle *h, uint64_t *mask) {
  if (!h || !mask) return KID_EINVAL;
  *mask = (uint64_t)h->hot_zero_mask;
  return KID_OK;
}
int kid_profile_enable(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  h->profile = on != 0;
  h->berg_ms = 0.; h->all_ms = 0.; h->berg_launches = 0;
  return KID_OK;
}
int kid_profile_get(kid_handle *h, double *berg_ms, int64_t *launches, double *all_ms) {
  if (!h) return KID_EINVAL;
  // the events were only recorded while stepping (no host/device sync in the timed loop); resolve them now
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  for (auto &pe : h->pending) {
    float ms = 0.f;
    KID_HIP(h, hipEventElapsedTime(&ms, pe.first, pe.second));
    h->berg_ms += ms;
    (void)hipEventDestroy(pe.first); (void)hipEventDestroy(pe.second);
  }
  h->pending.clear();
  if (berg_ms) *berg_ms = h->berg_ms;
  if (launches) *launches = h->berg_launches;
  if (all_ms) *all_ms = h->all_ms;
  return KID_OK;
}

}  // extern "C"

#include "kid_locate.inc"
#include "kid_restart.inc"
#include "kid_traj.inc"
#include "kid_migrate.inc"
#include "kid_halo_bergs.inc"
#include "kid_halo.inc"
#include "kid_chksum.inc"
#include "kid_chksum_device.inc"
#include "kid_check.inc"
