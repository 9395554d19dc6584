/* kid.h -- C ABI of libkid_hip.so: the MI355X (gfx950) implementation of the NOAA-GFDL/icebergs evolve loop.
 *
 * Drop-in boundary.  Each entry point replaces one `subroutine f(bergs)` call site
 * inside icebergs_run() of /root/reference/src/icebergs.F90; the Fortran host keeps icebergs_init() /
 * icebergs_run() and its derived types, flattens the per-cell linked lists into the structure of arrays of
 * kid_types.h in reference traversal order, and calls these through the ISO_C_BINDING module
 * icebergs_amd/fortran/kid_hip_binding.F90 (see INTEGRATION.md for the glue a maintainer adds).
 *
 *   reference call site (icebergs.F90)                     entry point
 *   -----------------------------------------------------  --------------------------------------------
 *   ice_bergs_framework_init, grid copy   FW:1021-1094     kid_create + kid_set_static_grid
 *   forcing ingest result (grd%uo ... )   IB:5236-5383     kid_set_forcing
 *   the forcing ingest block itself       IB:5236-5383     kid_ingest_forcing (+ kid_get_forcing for send_data)
 *   calving block + accumulate_calving + calve_icebergs  IB:5203-5231, 5388, 5403   kid_calving
 *   write_restart_bergs / read_restart_bergs  IO2:124-631, 663-1049   kid_write_restart / kid_read_restart
 *   accumulator zeroing                   IB:5125-5156     kid_zero_accumulators
 *   interp_gridded_fields_to_bergs        IB:5423, 5473    kid_interp_gridded_fields_to_bergs
 *   evolve_icebergs                       IB:5433          kid_evolve_icebergs
 *   move_berg_between_cells               IB:5437          kid_move_berg_between_cells
 *   footloose_calving                     IB:5453          kid_footloose_calving
 *   adjust_fl_berg_interactivity          IB:5486          kid_adjust_fl_berg_interactivity
 *   thermodynamics                        IB:5505          kid_thermodynamics
 *   create_gridded_icebergs_fields        IB:5512          kid_create_gridded_icebergs_fields
 *   (all of the above, one coupling step)                  kid_run_step / kid_step_local + kid_step_gather
 *
 * Conventions: every function returns 0 on success and a negative KID_E* code on failure (the Fortran shim
 * turns non-zero into error_mesg(...,FATAL), the reference's abort-on-error convention, e.g. IB:3207).
 * Host arrays are caller-owned, column-major fp64 / int32 as Fortran owns them; the library owns device
 * memory only.  One handle <-> one HIP device and one stream; handles are not thread-safe (the reference is
 * single-threaded per rank and non-reentrant, IB:5110).  There is no CPU fallback: if no gfx950 device can be
 * used, kid_create fails.
 */
#ifndef KID_H
#define KID_H
#include "kid_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kid_handle kid_handle;

enum {
  KID_OK = 0,
  KID_EINVAL = -1,     /* bad argument / shape mismatch                         */
  KID_EHIP = -2,       /* a HIP runtime call failed (see kid_last_error)        */
  KID_ENODEV = -3,     /* no usable GPU                                         */
  KID_ECAPACITY = -4,  /* more bergs than the handle's capacity                 */
  KID_EUNSUPPORTED = -5 /* a switch combination this build does not implement   */
};

/* ---- lifetime ---- */
int kid_create(const kid_grid_desc *grid, const kid_params *params, int64_t capacity, int device,
               kid_handle **out);
/* Frees everything the handle allocated (buffers the caller bound with kid_bind_* stay the caller's).  If the runtime refuses a
 * free the rest is freed all the same, KID_EHIP is returned and kid_last_error(NULL), called by the same thread, names the
 * first failure. */
int kid_destroy(kid_handle *h);
/* Bytes of device and of pinned host memory that the live handles of this process hold at the moment, all devices together
 * (either pointer may be NULL).  A handle's share is back at what it was before kid_create once kid_destroy has returned. */
int kid_memory_in_use(int64_t *device_bytes, int64_t *pinned_bytes);
int kid_set_params(kid_handle *h, const kid_params *params);
/* Launch on an existing hipStream_t (e.g. PyTorch's current stream).  NULL names the device's default (null) stream;
 * a handle that is never given a stream uses a private non-blocking one. */
int kid_set_stream(kid_handle *h, void *hip_stream);
/* Pipelined launches: with `enable`, a fused per-berg launch goes through the hot build in two halves on the main stream
 * while the general build (cell hops, bounces; ~85 us of single-wave latency) of each half runs on `side_stream`, under
 * the hot build of the other half or of the next step.  Every entry point that reads berg state or accumulators on the
 * main stream first orders itself behind the side stream; a gather launched on the side stream itself is ordered by
 * that stream (icebergs_amd/distributed.py PipelinedStepper).  Results do not depend on the setting.
 * enable = 2, the "slow lane" schedule: the hot build stays one launch; a berg it hands over at step s is stepped by
 * general-build launches on `side_stream` for steps s and s+1 (under the hot builds of s+1 and s+2) and returns to the
 * hot build at s+2, so the general build's latency never sits between two hot builds.  The caller alternates two
 * accumulator blocks (kid_bind_accum_buffer) and launches the gather on the side stream; the per-cell forcing records
 * are double-buffered inside.  Applies to the fused RK4/Verlet step (either interpolation order) without footloose, bonds
 * or interactions and falls back to the plain schedule otherwise. */
int kid_set_side_stream(kid_handle *h, void *side_stream, int enable);
int kid_sync(kid_handle *h);
const char *kid_last_error(const kid_handle *h);
const char *kid_version(void);
int64_t kid_sizeof(int which); /* 0 kid_params, 1 kid_grid_desc, 2 kid_berg_soa, 3 kid_bond_soa, 4 kid_forcing_in, 5 kid_calving_params, 6 kid_calving_in: ABI layout check */

/* ---- grid and forcing (host pointers; KID_G_* / KID_F_* order) ---- */
int kid_set_static_grid(kid_handle *h, const double *const fields[KID_NGRID_STATIC]);
int kid_set_forcing(kid_handle *h, const double *const fields[KID_NFORCING]);
/* Same, but the planes already live in device memory (e.g. an ocean model on the same GPU): device-to-device
 * copy + the per-cell prepass, asynchronous on the handle's stream. */
int kid_set_forcing_device(kid_handle *h, const double *const dev_fields[KID_NFORCING]);

/* ---- berg population ---- */
int kid_upload_bergs(kid_handle *h, const kid_berg_soa *host);        /* sets the population (n <= capacity) */
int kid_download_bergs(kid_handle *h, kid_berg_soa *host);            /* host->n must be >= kid_num_bergs slots */
int kid_num_bergs(kid_handle *h, int64_t *n_slots, int64_t *n_alive); /* slots include dead bergs until compaction */
/* Drops melted / departed bergs and keeps the order of the rest.  One gather of every field into the second set of arrays that
 * the re-binning uses too: the first call of either allocates it (kid_memory_in_use then reports one more berg SoA for the
 * handle).  While bond tables exist (kid_upload_bonds, kid_initialize_bonds) rows keep their places: KID_EUNSUPPORTED, as from
 * kid_move_berg_between_cells, and nothing is changed -- unless kid_set_bonds_follow_rows has switched the tables to follow
 * their rows: then the lists of the kept rows move with them, and a list that named a dropped row keeps the slot, its other_id
 * and its count, with no partner row behind it. */
int kid_compact_bergs(kid_handle *h);
/* move_berg_between_cells (IB:5437): device counting sort of the SoA by cell (j-major), dead bergs dropped.  Results
 * never depend on it, speed does.  kid_run_step calls it every `steps` steps (default 16; 0 = never; never with bond tables,
 * mts or interacting bergs).  With bond tables: KID_EUNSUPPORTED and nothing changed, unless kid_set_bonds_follow_rows is on;
 * then the tables are carried through the same permutation, at once (the copy is never left to the next step). */
int kid_move_berg_between_cells(kid_handle *h);
int kid_set_resort_interval(kid_handle *h, int steps);
/* Bond tables follow their rows.  on = 0 (the default): kid_compact_bergs and kid_move_berg_between_cells refuse a handle with
 * bond tables, as above.  on = 1: both accept it and carry the tables through their permutation in one more launch
 * (csrc/kid_rows.inc, permute_bonds_kernel): every list moves with its row, in list order, with its other_id, broken marks and
 * bond fields bit for bit, and the rows of the partners are re-derived through the inverse permutation.  A partner that is dead
 * or dropped at that moment leaves the list's slot without a partner row, which is what kid_upload_bonds leaves for an id it
 * does not find among the live rows; dead rows lose their own lists.  The first such call allocates a second set of tables
 * (about 116 bytes per berg and slot; kid_memory_in_use reports it, kid_reserve frees it until the next permutation).  Any other
 * value of `on` is KID_EINVAL.  Accepted at any time between steps, with or without bonds.  kid_run_step's own schedule is the
 * same either way, and so is everything that refuses bonds for other reasons (kid_locate_bergs, tiles, halo rows,
 * reproducible sums, footloose). */
int kid_set_bonds_follow_rows(kid_handle *h, int on);
/* A hook for tests: the partner rows and partner slots the kernels follow, as [max_bonds * n] each, slot-major with stride n
 * (the layout of kid_bond_soa); -1 past a list's end and for a slot without a partner row.  n must be the handle's row count
 * (KID_EINVAL otherwise, and when no bonds were uploaded). */
int kid_bond_partner_rows(kid_handle *h, int32_t *row, int32_t *slot, int64_t n);

/* ---- growable capacity: the one convenience of the reference's linked lists, which grow on the heap ---- */
/* The handle's current row capacity: what kid_create was given, or what kid_reserve / auto-reserve have made of it since. */
int kid_capacity(kid_handle *h, int64_t *rows);
/* Makes the capacity at least `rows`.  rows <= the current capacity changes nothing and returns KID_OK (a handle never
 * shrinks); rows > 2^29, the limit of kid_create, is KID_EINVAL.  Rows keep their numbers, so the call is legal with bond
 * tables, with halo rows resident and in a decomposed run with bergs waiting to be packed; it joins the side stream, runs a
 * pending re-binning and leaves the slow-lane schedule.  Afterwards every result is what a handle created at the new
 * capacity and brought to the same state would give.  Every block that holds state is moved on its own (allocate, copy the
 * first n rows, swap, free), so the most held at any moment is the new total plus one old block; scratch is reallocated, or
 * freed and allocated again by whoever needs it next.  If the device runs out of memory the call returns KID_EHIP with the
 * runtime's message and the handle is valid at the old capacity.  Not a step-path call: it synchronises the stream once per
 * block. */
int kid_reserve(kid_handle *h, int64_t rows);
/* Auto-reserve, off by default: the entry points that append rows make room before they write.  growth = 0 switches it off;
 * otherwise growth >= 1 and min_free >= 0, and max_capacity = 0 means 2^29 (anything else: KID_EINVAL).  A call that is
 * about to hold `need` rows, more than the capacity, grows the handle to min(max_capacity, max(need, ceil(capacity * growth)));
 * need > max_capacity is KID_ECAPACITY before anything is written, and kid_last_error names both numbers.
 *   count known first: kid_upload_bergs (host->n), kid_unpack_immigrants[_pair] (what is left over after the compaction they
 *     already try) and kid_calving (between its count pass and its emit pass: one more stream synchronisation, in this mode
 *     only) cannot overflow any more;
 *   children made inside a per-berg launch (kid_footloose_calving, kid_step_local / kid_run_step with footloose, at every
 *     step): capacity - n >= min_free is ensured before the launch.  A launch that makes more children than that is still
 *     KID_ECAPACITY -- no retry, the parents' bits are spent -- and the message gives the number of rows it tried to append:
 *     choose min_free from the largest per-step append the run has seen.
 * With the mode off every call behaves and reports exactly as before. */
int kid_set_auto_reserve(kid_handle *h, int64_t min_free, double growth, int64_t max_capacity);

/* berg%uo..od (the last interpolated environment).  With old_interp_flds_order accel re-interpolates (IB:2035) and the
 * stored copy is read only by trajectory records (FW:5422) and bergs_chksum (FW:7040): a run with ignore_traj=T may
 * switch it off (on = 0) and save 13 stores per berg per step.  With .not.old_interp_flds_order the stored environment is
 * an input of evolve_icebergs and thermodynamics called one after the other, but not of the fused step, which interpolates
 * it for itself: switched off there, kid_run_step / kid_step_local still run, and the entry points that read it
 * (kid_evolve_icebergs, kid_thermodynamics) return KID_EINVAL.  Default on. */
int kid_set_store_environment(kid_handle *h, int on);

/* Reproducible per-cell sums: the device side of the namelist's `parallel_reprod`.  Off by default.  With it on, every
 * accumulator plane, the find_melt_using_spread_mass planes and net_heat_to_ocean are functions of the set of bergs only:
 * each berg's contributions are stored, then summed per cell in the reference's traversal order (inorder keys start_year,
 * start_day, start_mass, start_lon, start_lat, then the berg id) as a strict left fold onto what the plane holds; the
 * heat total is the per-cell sums reduced by a tree of fixed shape.  Results no longer depend on the row layout, the
 * re-binning interval, compaction, wave scheduling or fused versus phase-by-phase launches; per-berg arithmetic is that
 * of the default path.  Turning it on allocates about 0.4 KB per berg of capacity (KID_EHIP if that fails); turning it off
 * frees it.  Not implemented together with mts, interactive_icebergs_on or footloose: KID_EUNSUPPORTED, here and at
 * every step while both are on (kid_last_error names the switch).  The sum across GPUs of a sharded run stays the
 * all-reduce's. */
int kid_set_reproducible_sums(kid_handle *h, int on);

/* Forcing ingest on the device: the block of icebergs_run that builds grd%uo .. grd%hi from the
 * coupler's arguments, IB:5236-5383 + invert_tau_for_du IB:8272-8296: B/C-grid velocities, B/C/A-grid wind stress,
 * stress -> velocity difference, the Kelvin test on sst, sss = -1 when absent, land / NaN scrub.  One rank owns the
 * whole domain, so mpp_update_domains reduces to the zonal wrap of the halo columns (in->cyclic_x) or to nothing.
 * Replaces the host-side ingest + kid_set_forcing.  Host arrays are staged and the call returns when they may be
 * reused; with in->on_device nothing is copied and the call is asynchronous on the handle's stream.
 * add_iceberg_thickness_to_SSH (IB:5330-5337) stays with the host. */
int kid_ingest_forcing(kid_handle *h, const kid_forcing_in *in);
/* grd%uo .. grd%hi as the handle holds them (KID_F_* order, data-domain planes, NULL entries skipped): what the
 * reference hands to send_data for id_uo, id_vo, ... (IB:5529-5548).  Needs kid_set_forcing or kid_ingest_forcing. */
int kid_get_forcing(kid_handle *h, double *const fields[KID_NFORCING]);

/* ---- calving source ----
 * kid_calving is, in this order, the calving block of icebergs_run (IB:5203-5231: mask, running mean IB:5999-6038, kg/s),
 * accumulate_calving (IB:6153-6222) and calve_icebergs (IB:6225-6402): the buckets grd%stored_ice(:,:,1:10) /
 * grd%stored_heat live on the device, and bergs calved from overflowing buckets are appended to the resident SoA
 * (ids from the per-cell counter, kid_set_iceberg_counter).  bergs%current_year / current_yearday come from kid_params.
 * scalars[KID_NCALV_SCALARS]: what the call adds to the budget scalars of type icebergs (KID_CS_* order; may be NULL).
 * Returns KID_ECAPACITY when the SoA cannot hold the new bergs.  Replaces IB:5203-5231, 5388, 5397, 5403. */
int kid_set_calving_params(kid_handle *h, const kid_calving_params *cp);
/* read_restart_calving: stored_ice (10 data-domain planes), stored_heat, the two running means; NULL keeps the handle's */
int kid_set_calving_state(kid_handle *h, const double *stored_ice, const double *stored_heat, const double *rmean_calving,
                          const double *rmean_calving_hflx);
/* ... and for write_restart_calving / send_data (id_stored_ice, id_real_calving IB:5593-5600); NULL entries are skipped */
int kid_get_calving_state(kid_handle *h, double *stored_ice, double *stored_heat, double *rmean_calving,
                          double *rmean_calving_hflx, double *real_calving);
int kid_calving(kid_handle *h, const kid_calving_in *in, double *scalars);
/* grd%calving (kg/s, the unused remainder: id_unused IB:5396, returned to the coupler at IB:5656) and grd%calving_hflx
 * after kid_calving; data-domain planes, NULL skipped.  The melt the step adds to grd%calving_hflx (IB:3129) is the
 * accumulator KID_A_CALVING_HFLX. */
int kid_get_calving(kid_handle *h, double *calving, double *calving_hflx);

/* ---- restart files straight from the structure of arrays ----
 * icebergs.res.nc as write_restart_bergs writes it (icebergs_fms2io.F90:124-420: one unlimited dimension "i", the same
 * variable names, order, types and long_name / units attributes, ids split into id_cnt / id_ij), bonds_iceberg.res.nc
 * for bonded populations (IO2:466-583) and calving.res.nc
 * (IO2:583-631: stored_ice, stored_heat, iceberg_counter_grd, the running means).  netCDF classic (CDF-2) written and
 * read directly: neither FMS nor libnetcdf is needed.
 * The first three work on host arrays and need no device: */
int kid_restart_write_bergs(const char *path, const kid_params *p, const kid_berg_soa *host);
int kid_restart_count_bergs(const char *path, int64_t *n);
/* fills the arrays of `host` (room for `capacity` rows): the file's fields, zeros elsewhere, *_old = current values and
 * halo_berg = 0 as read_restart_bergs sets them (IO2:895-925); xi / yj need the grid and are left to kid_read_restart,
 * and so are the ids of a file with the old 32-bit iceberg_num (they come back 0 here; generate_id needs the counters) */
int kid_restart_read_bergs(const char *path, kid_berg_soa *host, int64_t capacity);
/* bonds_iceberg.res.nc (IO2:466-583, read_restart_bonds IO2:1190-1481): one record per bond side; `bergs` gives the ids
 * and cells of both ends.  Reading puts every bond at the head of its berg's list, as form_a_bond does. */
int kid_restart_write_bonds(const char *path, const kid_params *p, const kid_berg_soa *bergs, const kid_bond_soa *bonds);
int kid_restart_read_bonds(const char *path, const kid_berg_soa *bergs, kid_bond_soa *bonds);
/* the resident state to <dir>/icebergs.res.nc (+ bonds_iceberg.res.nc with bonds, + calving.res.nc when the calving
 * source is on), and back:
 * bergs outside the computational domain or in cells of zero area are dropped (IO2:880-884, 948-955), xi / yj are
 * recomputed on the device from (lon, lat, ine, jne) (IO2:945) */
int kid_write_restart(kid_handle *h, const char *dir);
int kid_read_restart(kid_handle *h, const char *dir);
/* ---- a berg's cell from its position: ignore_ij_restart / use_slow_find (IO2:876-891) ----
 * mode 1 is find_cell_by_search (FW:5710-5842: the walk over the cell centres from the nearest inset corner, find_better_min and
 * find_cell_loc on stagnation, find_cell when the moves run out), mode 2 is find_cell (FW:6011-6041: the structured-grid guess,
 * then the scan of the computational domain, j outer, i inner, first hit).  One lane per berg; the scan is shared by the wave
 * (csrc/kid_locate.inc).  A berg the reference's path does not find is not found here either.  The grid needs lonc / latc and a
 * halo of one cell (the walk reads the centres one cell beyond the computational domain): KID_EINVAL otherwise.
 *
 * kid_locate_bergs: on the live resident rows, from their lon, lat: writes ine, jne and xi, yj (pos_within_cell, IO2:947).  A row
 * that no cell of the computational domain holds, or whose cell has area 0 (grounded, IO2:950-957), becomes dead -- its cell
 * set to (isc, jsc), so that a decomposed handle does not take it for a berg waiting to be packed -- and leaves with the next
 * kid_num_bergs tail drop, compaction or re-binning.  counts (may be NULL) = {found, not on this grid, grounded}.  No other
 * field changes.  Refused with nothing written: mode outside {1, 2} and no static grid (KID_EINVAL), halo rows resident
 * (KID_EINVAL), bond tables on the handle (KID_EUNSUPPORTED: bonds keep their rows; locate first, then kid_upload_bonds). */
int kid_locate_bergs(kid_handle *h, int mode, int64_t counts[3]);
/* kid_read_restart with ignore_ij_restart: mode 0 (the default) trusts the file's ine, jne; with 1 or 2 they are ignored and
 * every berg of the file is searched by that mode in temporary device blocks sized by the file (freed before the call
 * returns), after which the read goes on as before: a berg that was not found fails the domain test, ids of a legacy file
 * are handed out in file order before the grounded filter.  A handle that reads one global file keeps the bergs of its own
 * computational domain.  Another mode: KID_EINVAL. */
int kid_set_restart_locate(kid_handle *h, int mode);
/* bergs_chksum (FW:6889-6987: the "write_restart berg chksum=.. chksum2=.. chksum3=.. chksum4=.. chksum5=.. #=.." line of
 * icebergs_save_restart, IB:8145, which the reference's regression tests record) on the resident population:
 * out[0..4] = chksum, chksum2, chksum3, chksum4, chksum5 as the default integers the reference prints, out[5] = #, the number
 * of bergs on the computational domain.  FMS's mpp_chksum is restated (wrap-around sum of bit patterns); see
 * csrc/kid_chksum.inc for the quirks that are reproduced on purpose. */
int kid_bergs_chksum(kid_handle *h, int64_t out[6]);
/* The same six integers, always identical to kid_bergs_chksum's on the same state, without the download: the traversal order
 * is built on the device by stable radix passes (csrc/kid_chksum_device.inc), chksum, chksum2 and chksum5 are integer
 * reductions there, and for chksum3 = chksum4 the device hands the host 16 bytes per berg of the computational domain (mass
 * and time_hash * pos_hash, in traversal order) plus the per-cell counts: the logarithm is the host's std::log, so that the
 * integers do not depend on which of the two routines computed them.  Same contract as kid_bergs_chksum: halo rows resident
 * are refused, dead rows and live rows outside the computational domain do not count, n = 0 gives six zeros, bond tables may be
 * resident.  per_cell (may be NULL) receives the record of the reference's '# of bergs/cell' line (FW:6978-6979): grd_chksum2
 * of the plane of per-cell counts.  Temporary device blocks sized by the number of rows and by the grid, freed before return. */
int kid_bergs_chksum_device(kid_handle *h, int64_t out[6], kid_grd_chksum *per_cell);
/* checksum_gridded (FW:6685-6758): one record per field, out[KID_CHK_UO .. KID_CHK_DEPTH] in the reference's order, n_out >=
 * KID_NCHK (else KID_EINVAL).  A plane is what kid_get_forcing, kid_get_calving, kid_get_calving_state and kid_get_accumulators
 * would return at that moment, or the static grid; an accumulator plane that the step neither zeroes nor fills (footprint
 * planes nobody reads, diagnostics that are off) reads as zeros; a field the handle does not hold (calving never configured,
 * a forcing plane never given, lonc / latc not set) has present = 0 and zeros.  grd_chksum2 / grd_chksum3 (FW:6761-6886)
 * over the computational domain; 3-d fields are the nine-slot *_on_ocean planes, stored_ice and melt_by_class.  Nothing is
 * downloaded: two device sweeps over all fields, each a tree of fixed shape (no atomics), so two calls on the same state
 * return the same bits; the mean, rms and sd differ from the reference's serial sums by rounding. */
int kid_checksum_gridded(kid_handle *h, kid_grd_chksum *out, int32_t n_out);
/* ---- the invariants the reference asserts under debug = .true. (csrc/kid_check.inc), on the resident rows, nothing downloaded
 * but the report.  `what` is a non-empty combination of
 *   KID_CHECK_POSITION    check_position (FW:6576-6603) on every live row: n_rows, n_xiyj, n_land, max_dxi, max_dyj.  The
 *                         recomputation is pos_within_cell as kid_locate_bergs, kid_read_restart and the immigrants' unpack
 *                         store it, so a state they wrote has no mismatch.  A cell outside the data domain gives -999, -999:
 *                         a mismatch, as in the reference; its mask is not read.
 *   KID_CHECK_ORDER       count_out_of_order (FW:4039-4089): n_in_halo, n_identical.  "# out of order" has no counterpart:
 *                         rows have no list order, and every traversal that depends on one sorts first.
 *   KID_CHECK_DUPLICATES  check_for_duplicates (FW:4118-4158): n_same_id, n_same_berg (with the four *_fast members under mts).
 *   KID_CHECK_IDS         check_for_duplicate_ids_in_list (FW:7405-7452) on this handle: n_dup_ids.
 * The last three look at the live rows whose cell is on the computational domain: halo copies and leavers drop out, as they do
 * from the reference's loops.  Equal means equal by value (Fortran's .ne.): a NaN equals nothing, -0.0 equals +0.0.  Members of
 * the report that a check not asked for would fill are 0 (first_id, first_row: -1).  Offenders are reported, never an error:
 * KID_OK when the checks ran.  KID_EINVAL: a NULL argument, `what` 0 or outside KID_CHECK_ALL, KID_CHECK_POSITION without a
 * static grid.  Nothing is written to a row or added to KID_S_ERROR_COUNT; halo rows may be resident; deferred cold fields are
 * gathered first, as for every reader.  Temporary device blocks sized by the number of rows, freed before return.  Cost: radix
 * passes over the rows that count, plus m(m-1)/2 compares per group of m rows with equal start keys (none in a healthy state). */
int kid_check_bergs(kid_handle *h, uint32_t what, kid_check_report *rep);
/* the ids of the rows KID_CHECK_IDS counts, ascending, duplicates kept; *n = how many.  ids == NULL: the count only.  More than
 * `capacity`: KID_ECAPACITY with *n set and nothing written.  What a decomposed run exchanges to find an id that two tiles own
 * (check_for_duplicates_in_parallel, FW:7344-7403). */
int kid_sorted_ids(kid_handle *h, int64_t *ids, int64_t capacity, int64_t *n);

/* ---- trajectories: record_posn (FW:5328-5498) as a device pass that appends one record per selected berg
 * to buffers in HBM, and iceberg_trajectories.nc (icebergs_fms2io.F90:1631-2103) written from them: dimension "i", lon,
 * lat, year, day, id_cnt, id_ij, then the save_fl_traj group, then the long group unless save_short_traj (same names,
 * types and attributes).  kid_write_trajectories appends to an existing file, like the reference, and empties the buffers.
 * With kid_traj_params.save_bond_traj every bond of a sampled berg is sampled too, from each of its two bergs (FW:5456-5490),
 * and kid_write_bond_trajectories writes / extends bond_trajectories.nc (write_bond_trajectory, icebergs_fms2io.F90:2106-2331:
 * lon, lat, year, day, length, n1, n2, id_cnt1, id_ij1, id_cnt2, id_ij2 and, with dem, tangd1, tangd2, nstress, sstress,
 * rel_rotation, broken); with no bond records pending it leaves the file system alone, as the reference does. */
int kid_set_traj_params(kid_handle *h, const kid_traj_params *tp);
int kid_record_posn(kid_handle *h);
int kid_num_traj_records(kid_handle *h, int64_t *n);
int kid_write_trajectories(kid_handle *h, const char *path);
int kid_num_bond_traj_records(kid_handle *h, int64_t *n);
int kid_write_bond_trajectories(kid_handle *h, const char *path);

/* ---- berg migration between the handles of a domain-decomposed model (first slice; send_bergs_to_other_pes
 * FW:2997-3247).  The handle packs and unpacks the reference's wire format (pack_berg_into_buffer2 FW:3250-3301,
 * unpack_berg_from_buffer2 FW:3455-3680: buffer_width reals per berg, integers as reals); the caller moves the buffers
 * (mpp_send / mpp_recv), so a GPU rank can exchange bergs with ranks running the reference.  Call order per step, as FW:3022-3230:
 * pack E, pack W, send/recv, unpack both, then pack N, pack S, send/recv, unpack both -- after kid_evolve_icebergs /
 * kid_step_local (a berg that left the computational domain is dead on the device with its post-evolve state kept; packing
 * consumes it).  kid_pack_emigrants: *n = bergs selected for `dir` (KID_DIR_*); if *n > capacity nothing is packed and
 * KID_ECAPACITY is returned.  kid_unpack_immigrants appends, resets the *_old fields (FW:3573-3577), finds each berg's cell on
 * this grid (check_and_find_cell FW:5973-6008) and its xi / yj (FW:3634); a berg no cell of the data domain takes is dropped
 * and KID_EINVAL returned (the reference's FATAL, FW:3660).  Bonds, mts and dem: KID_EUNSUPPORTED. */
/* A decomposed host calls kid_buffer_width once at initialisation (ice_bergs_framework_init sizes its buffers there,
 * FW:1263-1292).  From the first migration call on the handle is in "decomposed" mode: a berg that left the tile is a dead row
 * whose cell lies outside the computational domain until a pack call has collected it, and such rows survive whatever the host
 * does between kid_evolve_icebergs and the exchange -- kid_move_berg_between_cells (the reference's own order, IB:5437-5447),
 * the dead-tail drop of kid_num_bergs, kid_compact_bergs; the rows of bergs already packed are reclaimed by those calls, and
 * by kid_unpack_immigrants itself before it reports KID_ECAPACITY.  A handle that never makes a migration call deletes leavers
 * at once, as a PE without neighbours does (FW:3024-3041). */
int kid_buffer_width(kid_handle *h, int32_t *width);
int kid_pack_emigrants(kid_handle *h, int32_t dir, double *buf, int64_t capacity, int64_t *n);
int kid_unpack_immigrants(kid_handle *h, const double *buf, int64_t n);
/* the two directions of one exchange pass in one launch and one host read each way: axis 0 = east (a) and west (b), axis 1 =
 * north (a) and south (b); the pair unpack appends the rows of buf_a, then those of buf_b (the order of the reference's two
 * unpack loops, FW:3064-3097).  Same results as the single calls. */
int kid_pack_emigrants_pair(kid_handle *h, int32_t axis, double *buf_a, int64_t capacity_a, int64_t *n_a, double *buf_b, int64_t capacity_b, int64_t *n_b);
int kid_unpack_immigrants_pair(kid_handle *h, const double *buf_a, int64_t n_a, const double *buf_b, int64_t n_b);
/* Halo bergs (update_halo_icebergs FW:1800-2131): interactive_force (IB:480-607) walks the lists of the neighbouring cells, which on
 * a tile's edge belong to another rank; the reference fills them with copies of the neighbour's bergs.  kid_pack_halo_bergs_pair
 * packs the copies both ways along an axis in one launch, in the record of the migration calls with halo_berg (real 30) = 1; the
 * source rows stay as they are.  w = width (0: the grid's halo), 2 <= w <= min(halo, nic, njc), else KID_EINVAL.
 *   axis 0, live rows in cells jsc..jec:  buf_hi (for the east neighbour) = columns iec-w+2 .. iec (w-1 of them),
 *                                         buf_lo (for the west neighbour) = columns isc .. isc+w-1      (FW:1896, 1911);
 *   axis 1, live rows in columns isd..ied (the halo rows axis 0 has just brought included: a diagonal neighbour's bergs arrive
 *           in two hops):                 buf_hi (north) = rows jec-w+2 .. jec, buf_lo (south) = rows jsc .. jsc+w-1 (FW:1981, 1995).
 * A NULL buffer: no neighbour on that side, nothing is selected for it.  *n = rows selected; if *n > capacity nothing is packed
 * and KID_ECAPACITY is returned.  The neighbour hands the records to kid_unpack_immigrants(_pair), which finds their cells
 * anywhere in its data domain.  Call order per step: axis 0 pack, send/recv, unpack, axis 1 pack, send/recv, unpack, then
 * kid_evolve_icebergs.
 * A halo row is a force source for that one kid_evolve_icebergs: its velocity sweep skips the row, its position sweep retires it
 * (dead, its cell put back inside; the next compaction or re-binning drops it).  From the unpack to that evolve
 * kid_interp_gridded_fields_to_bergs, kid_thermodynamics, the spreading and gather calls, kid_step_local, kid_run_step,
 * kid_budget, kid_stock, kid_incr_mass, kid_pack_emigrants*, kid_move_berg_between_cells, kid_footloose_calving,
 * kid_adjust_fl_berg_interactivity, kid_calving, kid_write_restart, kid_bergs_chksum, kid_record_posn and kid_write_trajectories return KID_EINVAL.  The reference takes the copies before thermodynamics (IB:5462)
 * and uses them in the next step's evolve; these calls do not fix the moment.
 * Covered: interactive_icebergs_on under the single-time-step Verlet scheme without bonds.  iceberg_bonds_on, mts, dem,
 * footloose, find_melt_using_spread_mass, static_icebergs, periodic_reentry, a namelist without interactive_icebergs_on and Runge_not_Verlet:
 * KID_EUNSUPPORTED from the pack call, and from an unpack call that meets a record with halo_berg = 1. */
int kid_pack_halo_bergs_pair(kid_handle *h, int32_t axis, int32_t width, double *buf_hi, int64_t capacity_hi, int64_t *n_hi, double *buf_lo, int64_t capacity_lo, int64_t *n_lo);
int kid_halo_berg_count(kid_handle *h, int64_t *n);   /* resident halo rows (alive, halo_berg = 1) */

/* ---- halo update of the on-ocean planes of a domain-decomposed model: mpp_update_domains(var_on_ocean, grd%domain) of
 * sum_up_spread_fields (IB:6106-6107), split where the reference calls the message layer.  A berg writes the nine slots of its
 * own cell only, so the 9-point sum (IB:6126-6131) of a cell on a tile's edge reads slots that belong to the neighbouring tile.
 * The handle packs the edge strips of the live planes and unpacks the neighbours' strips into its halo; the caller moves the
 * buffers, as with the berg migration above.  Per step of a tile, in the reference's order: kid_zero_accumulators,
 * [kid_interp_gridded_fields_to_bergs], kid_evolve_icebergs, the berg exchange, [interp again], kid_thermodynamics,
 * kid_calculate_mass_on_ocean, then per axis (0, then 1) kid_pack_halo_pair, send/recv, kid_unpack_halo_pair, then kid_step_gather.
 *
 * Buffer layout.  np = kid_halo_plane_count planes, in accumulator order from KID_A_MASS_ON_OCEAN; w = width,
 * 1 <= w <= min(halo, nic, njc), anything else KID_EINVAL (and so is an axis other than 0 or 1).
 *   axis 0 (east/west), rows jsc .. jec:          buf_hi (for the east neighbour) = columns iec-w+1 .. iec,
 *                                                 buf_lo (for the west neighbour) = columns isc .. isc+w-1;
 *       element order plane, j, i (i fastest), np * njc * w doubles each;
 *       unpack writes from_lo into columns isc-w .. isc-1 and from_hi into iec+1 .. iec+w.
 *   axis 1 (north/south), columns isc-w .. iec+w  (the corner columns axis 0 has just filled: a diagonal neighbour's corner arrives
 *                                                 in two hops, as with mpp_update_domains):
 *                                                 buf_hi = rows jec-w+1 .. jec, buf_lo = rows jsc .. jsc+w-1;
 *       the same element order, np * w * (nic + 2w) doubles each;
 *       unpack writes from_lo into rows jsc-w .. jsc-1 and from_hi into jec+1 .. jec+w.
 * A NULL pointer: no neighbour on that side (NULL_PE).  Nothing is packed for it, and on unpack that halo keeps what it holds: the
 * zero of the spreading's memset, which is what the halo of an undivided grid holds.
 * One launch packs (unpacks) both directions of an axis for all live planes, on the handle's stream, behind the side stream.
 * on_device: the buffers are device addresses (a torch tensor handed to RCCL, a GPU-aware MPI); the call only enqueues and the
 * caller orders its own work behind the handle's stream.  Otherwise the strips go through a pinned staging buffer: the pack call
 * returns when the data are in buf_hi / buf_lo, the unpack call when from_lo / from_hi may be reused.
 * Not covered: find_melt_using_spread_mass on tiles (its two extra gathers inside kid_step_local would need the same update),
 * the forcing planes (the host owns them).
 *
 * The tripolar north fold.  A tile of the top row has no north neighbour; its rows jec+1 .. jec+w lie beyond the fold and hold
 * what its mirror partner's rows jec .. jec-w+1 hold, turned by 180 degrees (FMS: halo(i, nj+k) = field(ni+1-i, nj+1-k) for a
 * centred scalar), with the nine slots of every group mirrored through the centre (IB:6110-6122: 1<->9, 2<->8, 3<->7, 4<->6).
 * The sending side is kid_pack_halo_pair(h, 1, w, buf_hi, NULL, ...) as it stands; the caller moves buf_hi to the partner.
 *   kid_unpack_halo_fold: element (plane 9 q + s, strip row r, strip column c) of the partner's strip goes to row jec + w - r,
 *       column (isc-w) + (nic+2w-1-c) and, with swap_slots != 0, to plane 9 q + (8 - s); swap_slots == 0 keeps the plane
 *       (old_bug_rotated_weights = T).  Call it after the east/west pass, next to the kid_unpack_halo_pair of the south strip.
 *   kid_fold_halo_self: the same for a handle that owns the whole zonal width and so is its own partner: planes to planes, no buffer.
 * The widths kid_unpack_halo_pair refuses and a NULL from_fold: KID_EINVAL; so is either call while halo rows are resident.
 * The caller says whether to swap: the library does not read old_bug_rotated_weights here. */
/* calculate_mass_on_ocean (IB:4984-...), the spreading half of kid_create_gridded_icebergs_fields: zero the 36 on-ocean planes,
 * the spreading launch (with reproducible sums: its fold too), NO gather.  kid_step_gather is the other half. */
int kid_calculate_mass_on_ocean(kid_handle *h);
int kid_halo_plane_count(kid_handle *h, int32_t *nplanes);   /* 9 (mass_on_ocean only) or 36: the rule of kid_accum_live_count */
int kid_halo_buffer_count(kid_handle *h, int32_t axis, int32_t width, int64_t *count);   /* doubles per direction */
int kid_pack_halo_pair(kid_handle *h, int32_t axis, int32_t width, double *buf_hi, double *buf_lo, int32_t on_device);
int kid_unpack_halo_pair(kid_handle *h, int32_t axis, int32_t width, const double *from_lo, const double *from_hi, int32_t on_device);
int kid_unpack_halo_fold(kid_handle *h, int32_t width, const double *from_fold, int32_t swap_slots, int32_t on_device);
int kid_fold_halo_self(kid_handle *h, int32_t width, int32_t swap_slots);

/* kid_set_forcing_device + kid_zero_accumulators for the step about to start, as one per-cell launch (fields == NULL
 * keeps the current forcing and only zeroes); the following kid_step_local does not zero again. */
int kid_step_prepare(kid_handle *h, const double *const device_fields[KID_NFORCING]);

/* ---- the hot path, phase by phase (same order as icebergs_run, IB:5423-5512) ---- */
int kid_zero_accumulators(kid_handle *h);
int kid_interp_gridded_fields_to_bergs(kid_handle *h);
int kid_evolve_icebergs(kid_handle *h);
int kid_footloose_calving(kid_handle *h);
/* kid_footloose_calving and the fused footloose step add the children to the population only once they are placed and have
 * their ids.  After KID_EHIP from either the row count (kid_num_bergs) is what it was before the call and no child is part of
 * the population; the parents have already shed the mass and the footloose step has advanced, so the handle is good for
 * reading out, not for stepping on.  After KID_ECAPACITY the handle is full (n_slots = capacity) and the children beyond it
 * were not written. */
/* Footloose children are placed on their parent's perimeter (displace_fl_bergs, IB:2631, 2664, 6432-6498) with the
 * counter-based generator of include/kid_rng.h: rn = f(kid_params.fl_rng_seed, parent id, footloose step, draw).  The step
 * counts the footloose passes of this handle (0 at kid_create, +1 per kid_footloose_calving or fused footloose step);
 * a restarted run sets it to continue the sequence.  (The reference seeds FMS's stream from the PE and the time, IB:2548.) */
double kid_footloose_uniform(int32_t seed, int64_t berg_id, int64_t step, int32_t draw);   /* the generator, for hosts that want to check a placement */
int kid_set_footloose_step(kid_handle *h, int64_t step);
int kid_get_footloose_step(kid_handle *h, int64_t *step);
/* adjust_fl_berg_interactivity (IB:2765-2841, called at IB:5486), for footloose together with interactive_icebergs_on under the
 * single-time-step Verlet scheme (no bonds, no mts).  A footloose child is born with fl_k = -1 and neither feels nor exerts a
 * contact force; this pass sets fl_k = -2, from which on the child collides like any other berg, for every live child that has
 * no other berg -- its parent and its siblings count, whatever their fl_k -- within contact range: closer than
 * max(R1 + R2, contact_distance) with contact_cells_lon = contact_cells_lat = 1, than contact_distance otherwise, looked for in
 * the cells i-contact_cells_lon .. i+contact_cells_lon by j-contact_cells_lat .. j+contact_cells_lat around the child's own,
 * cut at isd+1 .. ied, jsd+1 .. jed.  Only fl_k of promoted rows changes.  Its place in a step driven phase by phase:
 *   kid_zero_accumulators, [kid_interp_gridded_fields_to_bergs], kid_evolve_icebergs, kid_footloose_calving,
 *   [kid_set_conglom_ids with contact_distance > 0 or contact_spring_coef /= spring_coef], [kid_interp_gridded_fields_to_bergs],
 *   kid_adjust_fl_berg_interactivity, kid_thermodynamics, kid_create_gridded_icebergs_fields;
 * kid_step_local and kid_run_step run this sequence themselves.  The cell tables of the contact searches are brought up to date
 * first, so that rows appended since they were built (the children of this step) are candidates and partners.
 * promoted: the number of children the call promoted (one 4-byte read and a stream synchronisation); NULL: nothing is read
 * back and the call only enqueues.  Nothing happens (and *promoted = 0) unless footloose and interactive_icebergs_on are both on.
 * KID_EINVAL while halo rows are resident (kid_pack_halo_bergs_pair above). */
int kid_adjust_fl_berg_interactivity(kid_handle *h, int64_t *promoted);
int kid_thermodynamics(kid_handle *h);
int kid_create_gridded_icebergs_fields(kid_handle *h);

/* ---- bonded bergs, multiple time stepping, DEM (mts=T) ----
 * Bond lists travel as kid_bond_soa (include/kid_types.h), uploaded after the bergs they belong to; rows of bond
 * partners are re-derived from other_id (connect_all_bonds, FW:4963-5125).  While bonds exist the SoA is never
 * re-binned, so rows are stable between upload and download.
 *   kid_evolve_icebergs_mts   evolve_icebergs_mts IB:5431 / IB:6576-7078 (kid_evolve_icebergs dispatches to it when mts=T)
 *   kid_set_conglom_ids       transfer_mts_bergs IB:5459 -> set_conglom_ids FW:2601-2646 with whole conglomerates resident
 * kid_step_local / kid_run_step run the mts=T sequence of icebergs_run, including the once-after-upload `Visited`
 * block (IB:5409-5420: interpolate, label conglomerates, orig_bond_length). */
int kid_upload_bonds(kid_handle *h, const kid_bond_soa *host);
int kid_download_bonds(kid_handle *h, kid_bond_soa *host);
int kid_evolve_icebergs_mts(kid_handle *h);
int kid_set_conglom_ids(kid_handle *h);
/* The bonded tail of icebergs_init (IB:153-171) with manually_initialize_bonds: initialize_iceberg_bonds IB:356-441 +
 * connect_all_bonds + assign_n_bonds, on the resident population.  Needs iceberg_bonds_on (KID_EINVAL otherwise).
 * from_radii != 0: manually_initialize_bonds_from_radii (r_dist < 1.25 (radius1 + radius2), radius = sqrt(length width rdenom),
 * rdenom = 1/(2 sqrt 3) with hexagonal_icebergs, 1/4 otherwise); else r_dist < length (length_for_manually_initialize_bonds;
 * a non-positive length forms nothing).  r_dist is the reference's: fp64, the metric of convert_from_grid_to_meters at the mean
 * latitude, no periodic wrap of the longitude difference, correctly rounded square roots.  Every live row takes part, static
 * bergs and halo rows included; dead rows neither bond nor are bonded.
 * Order: a berg's new partners fill its slots in reverse traversal order (form_a_bond inserts at the head: slot 0 is the
 * partner the traversal -- cell, then the `inorder` keys, then row -- visits last).  Bonds already on the handle stay, in their
 * order, behind the new ones; a pair that is bonded already is skipped, so a second call changes nothing (icebergs_init calls
 * the routine twice).  New bonds: broken = 0, every KID_NBOND_F64 member 0.  n_bonds of every live berg is set to its count.
 * Partner rows and slots are written on the device; the host reads two counters.  Afterwards the handle is as after
 * kid_upload_bonds: the next step runs the `Visited` block (conglomerate labels, orig_bond_length).
 * The search is one lane per berg over a window of cells whose half-width follows from the largest threshold of the call and
 * the smallest cell extent of the static grid (kid_bond_init.inc), never all pairs unless the window is the whole domain.
 * If some berg would hold more than max_bonds bonds nothing is written and KID_ECAPACITY is returned (kid_last_error gives the
 * count and the berg's id); the handle stays usable.
 * *nformed (may be NULL): bond records added, both ends counted. */
int kid_initialize_bonds(kid_handle *h, int32_t from_radii, double length, int64_t *nformed);
/* count_bonds FW:5172-5285 with check_bond_quality: *nbonds = bond records of the bergs on the computational domain (the
 * reference's count, each bond from both its ends), *unmatched = those whose partner is not resident or holds no bond back to
 * this berg (what the reference's quality check flags).  A device reduction and one 16-byte read; either pointer may be NULL. */
int kid_count_bonds(kid_handle *h, int64_t *nbonds, int64_t *unmatched);
/* evolve_icebergs (IB:7081-7200) with interactive_icebergs_on under the single-time-step scheme, two sweeps with the
 * spring/damping terms of interactive_force inside accel.  Verlet: the velocity sweep, then the position sweep.
 * Runge_not_Verlet: the four stages of Runge_Kutta_stepping with position and velocity, then the *_old copies
 * (kid_evolve_icebergs dispatches to it when interactive_icebergs_on and mts=F) */
int kid_evolve_icebergs_interactive(kid_handle *h);

/* ---- budgets: what a coupled host asks outside the step.  Device reductions over the resident state (csrc/kid_budget.inc)
 * and one read of 96 bytes; nothing is downloaded.  Like kid_bergs_chksum they first order themselves behind the side stream
 * and run the copy of a pending re-binning; they change neither the population nor the planes, and a step after one of them
 * gives the bits of a step without.  Every sum is taken over the live rows whose cell lies on the computational domain (the
 * loops of sum_mass, FW:6617-6619): halo rows, dead rows and, in a handle that has migrated, dead rows waiting to be packed
 * do not count.
 * The sums are trees of fixed shape, without floating-point atomics: lanes of a wave by a butterfly, the four waves of a
 * block through LDS, the block sums by one finishing block in a fixed order.  The shape depends on the number of rows
 * only, so two calls on the same resident state return the same bits.  With kid_set_reproducible_sums on (and none of mts,
 * interactive_icebergs_on, footloose, where that mode refuses to step and these calls sum as by default) the rows are first
 * put in the mode's static order with the rows that do not count behind the others, and the same tree runs over that order:
 * the result no longer depends on the row layout, the re-binning interval or compaction.  That is invariance to the order,
 * not the reference's serial sum; the two differ by rounding.
 * The host sums the structs of several handles (ranks) itself, as the reference does with mpp_sum (IB:5728-5766). */
/* The budget block of icebergs_run (IB:5702-5727), the members of kid_budget_out (include/kid_types.h). */
int kid_budget(kid_handle *h, kid_budget_out *out);
/* icebergs_stock_pe (IB:8102-8133).  berg_mass = sum_mass(bergs) (IB:8119, 8124): bergs, bergy bits, footloose bits and
 * footloose bergy bits, all of them always, weighted by mass_scaling (FW:6627); stored_mass = the stored ice of the
 * computational domain, all classes (IB:8120, 8125; 0 for a handle without calving state).
 *   KID_STOCK_WATER: *value = stored_mass + berg_mass            (IB:8121)
 *   KID_STOCK_HEAT:  *value = -(stored_mass + berg_mass) * HLF   (IB:8126, kid_params.HLF): the latent heat of that ice; neither
 *                    heat_density nor grd%stored_heat enters the reference's stock (they are kid_budget's floating_heat, stored_heat)
 * No switch of the namelist makes the reference's routine return zero.  Any other index: *value = 0 as the reference's
 * `case default` leaves it (IB:8128-8129), and KID_EINVAL. */
int kid_stock(kid_handle *h, int32_t index, double *value);
/* icebergs_incr_mass (IB:6046-6074): mass(i,j) = mass(i,j) + grd%spread_mass(i,j) over the computational domain (IB:6066-6068),
 * with the spread mass of the last gather (KID_O_SPREAD_MASS), which is in kg m-2 already (the area division is
 * sum_up_spread_fields', IB:6077-6150): there is none here.  Without add_weight_to_ocean the call returns at once and the plane
 * is unchanged (IB:6057).  bergs%passive_mode (IB:6067) is not a member of kid_params: the caller skips the call, as
 * kid_icebergs_incr_mass of the Fortran glue does.  `mass` is the caller's plane (isc:iec, jsc:jec), ni x nj with the first index
 * fastest; another shape: KID_EINVAL.  on_device: `mass` is a device address, the add is one per-cell kernel on the handle's
 * stream and the call does not wait for it; otherwise the plane is staged through the device and the call returns when it is back. */
int kid_incr_mass(kid_handle *h, double *mass, int32_t on_device, int32_t ni, int32_t nj);

/* grd%iceberg_counter_grd (FW:1017), the per-cell counter generate_id draws berg ids from; (isd:ied,jsd:jed) int32 */
int kid_set_iceberg_counter(kid_handle *h, const int32_t *counter);
int kid_get_iceberg_counter(kid_handle *h, int32_t *counter);

/* ---- the hot path, fused: one launch does evolve + thermodynamics + mass spreading per berg ---- */
int kid_step_local(kid_handle *h);   /* zero accumulators, per-berg kernel(s); accumulators hold LOCAL sums */
int kid_step_gather(kid_handle *h);  /* 9-point gather + derived fields (after the cross-GPU all-reduce) */
int kid_run_step(kid_handle *h, int nsteps); /* nsteps x (kid_step_local; kid_step_gather) */

/* ---- results ---- */
/* acc: KID_NACC fields, out: KID_NOUT fields, each (ied-isd+1)*(jed-jsd+1); scalars: KID_NSCALAR running totals
 * since kid_create (the reference keeps them on `bergs`). NULL skips. */
int kid_get_accumulators(kid_handle *h, double *acc, double *out, double *scalars);
/* Device view of the accumulator block for RCCL: KID_NSCALAR + KID_NACC*ncell contiguous doubles -- the step's scalar
 * increments first, then the planes, so that the scalars and the planes a step fills (a prefix of the planes: distributed.py
 * accumulator_views) are one contiguous range, one all-reduce. */
int kid_accum_device_ptr(kid_handle *h, void **dev_ptr, int64_t *count);
/* How many doubles from the start of that block one step fills under the current parameters (the scalar increments + the
 * planes that are zeroed, scattered into and read by the gather): what a sharded run sums across GPUs between
 * kid_step_local and kid_step_gather.  MPI hosts: MPI_Allreduce(MPI_IN_PLACE, dev_ptr, live_count, MPI_DOUBLE, MPI_SUM). */
int kid_accum_live_count(kid_handle *h, int64_t *count);
/* Use caller-owned device memory (e.g. a torch tensor) for the accumulator block instead. */
int kid_bind_accum_buffer(kid_handle *h, void *dev_ptr, int64_t count);
/* find_melt_using_spread_mass (IB:5490-5503): grd%spread_mass_old -- the gridded mass before the thermodynamics -- and, with
 * Iceberg_melt_without_decay, spread_mass_tmp (IB:3411-3413) live in two planes that kid_step_local fills and kid_step_gather
 * reads.  Both are 9-point gathers of per-cell sums, i.e. linear in what each GPU's bergs contribute: a sharded run binds a
 * buffer of its own here (2 planes of ni*nj fp64) and all-reduces it between kid_step_local and kid_step_gather together with
 * the accumulator planes.  NULL returns to the handle's own planes.  The phase entry points do not fill them: with the switch on
 * and no buffer bound here, kid_thermodynamics returns KID_EUNSUPPORTED instead of a melt flux computed as if it were off. */
int kid_bind_spread_mass_old(kid_handle *h, void *dev_ptr, int64_t count);

/* ---- measurement: HIP-event timing of the per-berg kernel on the launch stream ---- */
int kid_profile_enable(kid_handle *h, int on);
/* telemetry: bergs that the hot build handed to the general build in the most recent per-berg launch */
int kid_last_redo_count(kid_handle *h, int64_t *count);
/* Re-binnings (kid_move_berg_between_cells) since kid_create whose copy of the rows was taken over by the plain hot build of
 * the step that followed, instead of a launch of its own.  Diagnostic: results never depend on it; KID_REBIN_EAGER=1 in the
 * environment at kid_create keeps it at zero. */
int kid_rebin_fused_count(kid_handle *h, int64_t *count);
/* The per-berg fields the most recent hot-build launch treated as zeros -- neither loaded nor stored -- one bit per KID_B_*
 * member: axn, ayn (an RK run since the upload), mass_of_bits (bergy_bit_erosion_fraction = 0, no footloose), heat_density
 * (calving off), each only while the upload held zeros there and no launch since could have written anything else.  0 for every
 * build but the plain hot builds.  Diagnostic: results never depend on it; KID_NO_ZERO_SKIP=1 in the environment at
 * kid_create keeps it at zero. */
int kid_hot_zero_mask(kid_handle *h, uint64_t *mask);
int kid_profile_get(kid_handle *h, double *berg_kernel_ms_total, int64_t *berg_kernel_launches,
                    double *all_ms_total);

#ifdef __cplusplus
}
#endif
#endif /* KID_H */
