// kid_handle.hpp -- the handle behind the C ABI, the owner of its device and pinned memory, and the forward declarations
// of the host-side functions that the .inc files and kid_hip.hip share.  Included by kid_hip.hip once, after the kernels
// (the handle holds their argument tables); the only file of the library that calls the HIP allocator.
#pragma once
#include "kid_mem.hpp"

// kid::MemOwner on the HIP allocator.  Fills are hipMemsetAsync on the handle's stream, whichever it is at the time of
// the call, so they are ordered before whatever the handle launches next.
struct HipAllocator {
  static constexpr int unknown_error = (int)hipErrorInvalidValue;   // asked to release a pointer the owner never handed out
  const hipStream_t *stream;
  int alloc(void **p, size_t bytes, kid::MemKind k) const { return (int)(k == kid::MEM_PINNED ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes)); }
  int release(void *p, kid::MemKind k) const { return (int)(k == kid::MEM_PINNED ? hipHostFree(p) : hipFree(p)); }
  int fill(void *p, int byte, size_t bytes) const { return (int)hipMemsetAsync(p, byte, bytes, *stream); }
  int copy(void *dst, const void *src, size_t bytes) const { return (int)hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice); }
};
// temporary storage of a rocprim call: ask rocprim for the size (null pointer), reserve() it, pass p and bytes
struct Scratch { void *p = nullptr; size_t bytes = 0; };
struct HipMem : kid::MemOwner<HipAllocator> {
  explicit HipMem(const hipStream_t *stream) : kid::MemOwner<HipAllocator>(HipAllocator{stream}) {}
  // `count` elements of T, typed faces of alloc / release / grow
  template <class T> hipError_t dev(T *&p, size_t count, int fill = kid::MEM_NOFILL, kid::MemKind k = kid::MEM_DEVICE) { void *q = nullptr; const int e = alloc(&q, count * sizeof(T), k, fill); p = (T *)q; return (hipError_t)e; }
  template <class T> hipError_t pinned(T *&p, size_t count) { return dev(p, count, kid::MEM_NOFILL, kid::MEM_PINNED); }
  template <class T> hipError_t drop(T *&p) { void *q = p; const int e = release(&q); p = (T *)q; return (hipError_t)e; }
  template <class T> hipError_t regrow(T *&p, size_t keep_count, size_t count) { void *q = p; const int e = grow(&q, keep_count * sizeof(T), count * sizeof(T)); p = (T *)q; return (hipError_t)e; }
  hipError_t reserve(Scratch &t, size_t bytes) {
    if (t.p && t.bytes >= bytes) return hipSuccess;
    int e = release(&t.p);
    if (!e) e = alloc(&t.p, bytes, kid::MEM_DEVICE);
    t.bytes = e ? 0 : bytes;
    return (hipError_t)e;
  }
};

// argument table of permute_all_kernel (kid_rows.inc): entries [0, n8) are 8-byte fields, [n8, n8 + n4) 4-byte
namespace {
enum { KID_PERM_MAX = KID_NB_F64 + KID_NB_I32 + 2 };   // every field, the ids, the lane array of the slow-lane schedule
struct PermTable { const void *src[KID_PERM_MAX]; void *dst[KID_PERM_MAX]; int n8, n4; };
// one set of the slot-major bond tables (the members of MtsDev that are indexed by MB_S): argument of permute_bonds_kernel
struct BondTables { int32_t *bcount = nullptr; int64_t *bother_id = nullptr; int32_t *bbroken = nullptr, *bother_row = nullptr, *bother_slot = nullptr; double *bf[KID_NBOND_F64] = {}; };
}  // namespace

// one set of what pack_forcing builds (kid_cells.inc): the per-cell records, the gathered cell packets of the hot build, and
// the device copy of the grid descriptor that points at them (berg_kernel reads it as a table)
struct ForcingSet { VelRec *vel = nullptr; TrcRec *trc = nullptr; double *pkt = nullptr; DevGrid *d_grid = nullptr; };
// what the handle has been given of the grid and the forcing
struct ForcingState {
  bool have_static = false, have_forcing = false;
  bool have_centres = false;   // kid_set_static_grid was given lonc and latc (optional there; the cell search walks on them)
  bool have_planes = false;    // d_forcing holds all eleven planes
  bool held[KID_NFORCING] = {};   // d_forcing[k] holds a plane that was given (kid_set_forcing, kid_ingest_forcing; ssh also from kid_set_forcing_device, kid_step_prepare)
};

struct kid_handle {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  // Every device or pinned block the handle allocates comes from `mem` (those of reproducible sums, which go when the mode
  // is switched off, from `rp_mem`) and goes back with it in kid_destroy; the members below only point into them.
  HipMem mem{&stream}, rp_mem{&stream};
  kid_grid_desc gd{};
  kid_params params{};
  int ni = 0, nj = 0;
  size_t ncell = 0;
  int64_t capacity = 0, n = 0;
  // kid_set_auto_reserve (kid_reserve.inc): auto_growth = 0 is off; the entry points that append rows grow the handle by this rule
  double auto_growth = 0.; int64_t auto_min_free = 0, auto_max_capacity = 0;
  // device memory
  double *d_static[KID_NGRID_STATIC] = {}, *d_forcing[KID_NFORCING] = {};
  GeoRec *d_geo = nullptr; double *d_hotok = nullptr; double *d_latref = nullptr;
  // the accumulator block: KID_NSCALAR step scalars, then KID_NACC planes of ncell (scalars first, so that they and the planes a
  // step really fills -- a prefix -- are ONE contiguous range for the all-reduce); d_acc points at plane 0
  double *d_acc_own = nullptr, *d_acc = nullptr;
  double *d_out = nullptr;                        // KID_NOUT*ncell
  double *d_totals = nullptr;                     // KID_NSCALAR running totals (the block's scalars are per-step)
  BergPtrs bp{};
  BergPtrs *d_bp = nullptr;      // device copy of the field-pointer table
  kid_params *d_params = nullptr; // device copy of the parameter block
  bool tables_dirty = true;
  Scratch scan_tmp;             // the scan of the row flags (kid_compact_bergs)
  unsigned long long *d_count = nullptr;
  int *d_redo_list = nullptr;  // bergs the FAST build hands to the general build
  // pipelined launches (kid_set_side_stream): the population goes through the hot build in two halves on the main
  // stream while the general build of each half runs on the side stream, under the hot build of the other half
  hipStream_t side_stream = nullptr; bool pipelined = false;
  int *d_redo_list2 = nullptr, *d_redo_count2 = nullptr;
  int *d_redo_cnt[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [part][parity]: a step's counters are zeroed by its prepass
  int redo_parity = 0; bool redo_prezeroed = false, acc_prezeroed = false;
  kid::ZeroState zs;                       // per field: held anything but zeros at the last upload; a launch since may have written it non-zero (kid_rows_plan.hpp)
  unsigned long long hot_zero_mask = 0ull; // fields the last hot-build launch treated as zeros, one bit per KID_B_* (kid_hot_zero_mask: tests, A/B runs)
  bool tail_valid = false;                 // the dead rows are exactly the tail (true between a re-binning and the next launch)
  bool mig_mode = false;                   // the host exchanges bergs with other handles (kid_migrate.inc): dead rows waiting to be packed are kept
  int32_t *d_keep = nullptr;               // layout flags of such a run (keep_flags_kernel)
  long long mig_last[2] = {0, 0};          // records of the last pack call per slot: sizes the pinned staging buffer
  long long halo_last[2] = {0, 0};         // the same for kid_pack_halo_bergs_pair
  bool halo_rows_live = false;             // copies of the neighbours' bergs are resident (kid_halo_bergs.inc): set by an unpack call, cleared by the evolve that retires them
  bool env_ever_stored = false;            // some launch since the last upload wrote berg%uo..od
  bool env_off_requested = false;          // kid_set_store_environment(h, 0)
  double *d_orient = nullptr;              // bond-derived hexagon orientation per berg (mts / interacting bergs)
  hipEvent_t evF[2] = {nullptr, nullptr}, evG[2] = {nullptr, nullptr}; bool evG_live[2] = {false, false};
  // "slow lane" schedule (kid_set_side_stream mode 2, launch_berg_lanes in kid_launch.inc)
  int side_mode = 0; int *d_lane = nullptr, *d_lane_alt = nullptr; hipEvent_t evR = nullptr; int lane_step = 1; bool lanes_active = false, carry_valid = false, evC_live = false;
  hipEvent_t evC = nullptr, evP = nullptr;
  // The forcing records, twice: while a side stream is in use, general-build launches of the previous step may still read
  // theirs, so pack_forcing (kid_cells.inc) alternates between the two sets and nothing else changes forc_parity.
  ForcingSet fset[2]; int forc_parity = 0;
  // A/B switches for measurements and tests, read from the environment ONCE, when the handle is created (nothing on the
  // stepping path calls getenv): KID_MTS_NO_GRAPH, KID_STABLE_RESORT, KID_NO_PLAIN_BUILD, KID_FL_UNFUSED, KID_NEW_ORDER_UNFUSED,
  // KID_MTS_ALWAYS_LABEL, KID_MTS_NO_FUSED, KID_REBIN_EAGER (every re-binning copies the rows at once), KID_NO_ZERO_SKIP (the plain hot builds load and store every field, the row permutation moves the fields known to be zero), KID_COLD_EAGER (no field is cold: a row permutation moves every member it did before cold fields), KID_CHKSUM_TIMING (kid_bergs_chksum_device prints the times of its parts), KID_MTS_FUSED_BLOCKS_CAP (workgroups the fused sub-step kernel may use: tests of its
  // fall-back), KID_MTS_POLL_LIMIT (spins before a lane of that kernel gives up: tests of the time-out)
  struct DebugOpts { bool stable_resort = false, no_plain_build = false, fl_unfused = false, new_order_unfused = false, mts_always_label = false, mts_no_fused = false, rebin_eager = false, chksum_timing = false, no_zero_skip = false, cold_eager = false;
                     int mts_fused_blocks_cap = 0, mts_poll_limit = 0; } dbg;
  int32_t *d_iceberg_counter = nullptr;  // grd%iceberg_counter_grd (FW:1017)
  bool fl_place_warm = false;
  unsigned fl_step = 0;                  // footloose passes so far: third counter word of the child-placement generator (kid_rng.h)
  int *d_fl_cursor = nullptr;
  int *d_fl_promoted = nullptr;          // kid_adjust_fl_berg_interactivity: children promoted by one pass, when the caller asks
  int32_t *d_fl_head = nullptr, *d_fl_next = nullptr; int64_t *d_fl_newid = nullptr; long long fl_ev_capacity = 0;   // fl_assign_ids_*
  unsigned *d_key[2] = {nullptr, nullptr}, *d_idx[2] = {nullptr, nullptr};  // radix-sort ping-pong buffers
  Scratch sort_tmp;
  BergPtrs bp_alt{};            // second set of field arrays: a re-binning or compaction writes all fields there in one launch, then swaps (perm_storage)
  // A re-binning whose permutation is known (rebin_plan) but whose copy has not run (rebin_apply): the next whole-population
  // plain hot build takes its rows through the permutation itself (launch_phase, kid_launch.inc); anything else that looks at rows, row
  // numbers or the pointer tables runs the copy first (rebin_flush).  Nothing of this state is visible from outside.
  bool rebin_pending = false;
  int64_t rebin_fused_count = 0;   // re-binnings taken by that launch so far (kid_rebin_fused_count: tests, A/B runs)
  struct RebinPlan { PermTable t{}; int moved_f[KID_NB_F64] = {}; int nmf = 0; unsigned long long moved = 0ull, zero_skipped = 0ull; const unsigned *perm = nullptr; long long n = 0;
                     unsigned moved_i32 = 0u; bool moved_id = false, origin_moves = false; } rplan;   // the int32 fields and the id move unless cold; `origin` moves in their place
  // Cold fields (kid_rows_plan.hpp): while `deferred`, the members of `set` sit where they were when the first permutation left them
  // out, and field f of row k is bp.f[f][origin[k]].  Everything that reads them by row or changes which rows exist materialises
  // first (cold_materialise, kid_rows.inc).  materialised: gathers so far
  struct ColdState { kid::ColdSet set; bool deferred = false; int64_t materialised = 0; int32_t *origin = nullptr, *origin_alt = nullptr; } cold;
  RebinTab *d_rb = nullptr;     // device table of the re-binning instance of the plain hot builds
  unsigned *d_cell_hist = nullptr; Scratch cscan_tmp; bool stable_resort = false;
  int resort_interval = 16, steps_since_sort = 0;
  // multiple time stepping / DEM
  MtsDev mts{}; MtsDev *d_mts = nullptr;
  int mb = 0; bool mts_ready = false, mts_dirty = true, have_bonds = false, visited = false;
  // kid_set_bonds_follow_rows: compaction and re-binning accept a handle with bond tables and carry them along (bonds_move,
  // kid_rows.inc).  bond_alt: the second set of tables, made at the first such permutation and dropped by kid_reserve; the two
  // sets change places after every permutation.  bond_alt_rows: rows of it that may hold something else than what the tables are born with
  bool bonds_follow = false; BondTables bond_alt{}; long long bond_alt_rows = 0;
  unsigned long long *d_key64[2] = {nullptr, nullptr}; int *d_rows[2] = {nullptr, nullptr};
  int *d_static_rows = nullptr; long long static_rows_n = -1, static_rows_cap = 0;   // rows ordered by the five static `inorder` keys (mts_build_order)
  unsigned long long *d_last_key = nullptr; int *d_order_flag = nullptr; long long order_n = -1;   // cell key of every row at the last sort: an unchanged population keeps its order
  unsigned long long *d_bond_sig = nullptr; bool labels_stale = true;   // per-berg signature of what the conglomerate labelling reads (set_conglom_ids skips itself while nothing changes)
  MtsDev mts_shadow{}; bool mts_shadow_valid = false;   // what d_mts holds (the table is re-uploaded only when it differs)
  int conglom_batch = 8;                                // label-propagation sweeps launched before the first convergence check (set_conglom_ids)
  Scratch mts_tmp;
  unsigned long long *d_bond_words = nullptr;           // counters of kid_initialize_bonds / kid_count_bonds (kid_bond_init.inc)
  double bond_ext[2] = {0., 0.}; bool bond_ext_valid = false;   // smallest cell extents in metres of the static grid (bond_extents)
  hipGraphExec_t sub_graph_exec = nullptr;  // the captured sub-step loop of evolve_icebergs_mts
  long long sub_graph_n = -1; int sub_graph_steps = 0; bool sub_graph_pair = false; double sub_graph_dt = 0.; hipStream_t sub_graph_stream = nullptr;
  bool use_graph = true;
  int fused_blocks[2] = {0, 0};             // co-resident workgroups of mts_substeps_kernel<4> / <8> (0: not asked yet)
  bool fused_ran = false;                   // a fused sub-step launch since the last look at its time-out counter
  int64_t fused_launches = 0;               // fused sub-step launches since kid_create (kid_mts_fused_launches: tests)
  Flags flags{0, 0, 1, 0, 0};
  // trajectories (kid_traj.inc): one buffer per sampled field, grown on demand
  bool traj_on = false; kid_traj_params traj_params{}; double *d_traj_f[64] = {}; double *d_traj_day = nullptr; int64_t *d_traj_id = nullptr;
  int32_t *d_traj_year = nullptr, *d_traj_nbonds = nullptr; unsigned long long *d_traj_cursor = nullptr; long long traj_capacity = 0, traj_count_bound = 0; int traj_nf = 0;
  double *d_mig_buf = nullptr; long long mig_capacity = 0; unsigned long long *mig_word = nullptr;   // pinned staging of kid_pack_emigrants / kid_unpack_immigrants
  double *halo_buf = nullptr; long long halo_capacity = 0;   // pinned staging of kid_pack_halo_pair / kid_unpack_halo_pair (kid_halo.inc)
  double *d_btraj_f[16] = {}; int64_t *d_btraj_id[2] = {}; int32_t *d_btraj_i[2] = {}; long long btraj_capacity = 0, btraj_count_bound = 0;   // bond samples
  double *d_spread_mass_old = nullptr;   // grd%spread_mass_old (find_melt_using_spread_mass, IB:5495-5497) + spread_mass_tmp; the handle's own or the caller's (kid_bind_spread_mass_old)
  double *d_spread_mass_old_own = nullptr;
  ForcingState forc;           // written by kid_set_static_grid and forcing_given (kid_cells.inc)
  int restart_locate = 0;      // kid_set_restart_locate: 0 kid_read_restart trusts the file's ine, jne; 1, 2 it searches (kid_locate.inc)
  double *d_calv_state = nullptr, *d_calv_scal = nullptr, *d_calv_part = nullptr; unsigned char *d_calv_flag = nullptr; int2 *d_calv_list = nullptr; double *calv_host = nullptr; kid_calving_params calv_params{};  // kid_calving (kid_calving.inc)
  bool calving_on = false, calving_first_call = true, rmean_init = false, rmean_hflx_init = false;
  double *d_ingest_stage = nullptr; size_t ingest_stage_count = 0; unsigned long long *d_ingest_key = nullptr;  // kid_ingest_forcing
  bool profile = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double berg_ms = 0., all_ms = 0.; int64_t berg_launches = 0;
  // reproducible sums (kid_set_reproducible_sums, kid_repro.inc): staging table, row keys / masks, the static canonical order
  // (valid while srows_n == n; reset wherever rows move), sort buffers, cell starts, per-cell heat and its block sums
  bool repro = false;
  struct Repro { double *stage = nullptr; int32_t *key = nullptr; unsigned long long *mask = nullptr; int *srows = nullptr; long long srows_n = -1;
                 unsigned long long *k64[2] = {nullptr, nullptr}; int *rows[2] = {nullptr, nullptr}; unsigned *k32[2] = {nullptr, nullptr};
                 int *cs = nullptr; double *cell_heat = nullptr, *part = nullptr; Scratch tmp; } rp;
  double *d_budget = nullptr, *d_budget_plane = nullptr;   // kid_budget.inc: block partials + results of the sweep; staging plane of kid_incr_mass
  std::string err;
};

#define KID_HIP(h, call)                                                                      \
  do {                                                                                        \
    hipError_t e__ = (call);                                                                  \
    if (e__ != hipSuccess) {                                                                  \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                          \
      return KID_EHIP;                                                                        \
    }                                                                                         \
  } while (0)

// host-side functions used before the file that defines them (the .inc files are included where their kernels belong)
extern "C" {
static int refresh_tables(kid_handle *h), join_side(kid_handle *h);
static int rebin_flush(kid_handle *h);   // run the copy of a pending re-binning (no-op without one) and put the cold fields in row order (cold_materialise)
static int rebin_flush_rows(kid_handle *h);   // ... the copy alone: for the step and for the callers that never look at a cold field
static int cold_materialise(kid_handle *h), cold_settle(kid_handle *h);   // kid_rows.inc
static int rebin_plan(kid_handle *h, bool dead_last);
static int rebin_core(kid_handle *h, bool with_lane, int *list, const int *list_count), rebin_apply(kid_handle *h, bool with_lane, int *list, const int *list_count);
static bool plain_namelist(const kid_handle *h), lanes_eligible(const kid_handle *h);   // kid_launch.inc
static int repro_refuse(kid_handle *h);                                                  // kid_repro.inc
static int mts_check_timeout(kid_handle *h), mts_fold_scalars(kid_handle *h), mts_refresh(kid_handle *h);   // kid_mts_host.inc
static int halo_bergs_supported(kid_handle *h, const char *what);                                                                           // kid_halo_bergs.inc
static int auto_reserve(kid_handle *h, int64_t need, const char *what);                  // kid_reserve.inc
}
