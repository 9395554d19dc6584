// kid_traj.inc -- trajectory sampling straight from the structure of arrays (SURVEY.md 8f N2):
//   record_posn      /root/reference/src/icebergs_framework.F90:5328-5498  -> record_posn_kernel: one lane per berg, the
//                    selected bergs append one record each to field buffers in HBM (a workgroup reserves its records
//                    with one atomic)
//   write_trajectory /root/reference/src/icebergs_fms2io.F90:1631-2103     -> kid_write_trajectories: iceberg_trajectories.nc
//                    (netCDF classic, see kid_restart.inc) with the reference's variables, types and attributes; an
//                    existing file is extended, as the reference does on every traj_write_hrs
//   bond samples     FW:5456-5490 (inside record_posn, save_bond_traj) -> record_bond_posn_kernel, one lane per bond slot
//   write_bond_trajectory IO2:2106-2331                                    -> kid_write_bond_trajectories: bond_trajectories.nc
// The reference keeps the samples in per-berg linked lists and gathers them to the I/O rank; here a sample is a row.
namespace {
struct TrajVar { const char *name; int field; int group; const char *longname, *units; };  // group: 1 save_fl_traj, 2 + footloose, 3 long, 4 + mts, 5 + dem
// order of the def_var calls, IO2:1829-1892; field < 0: -1 year (int), -2 day, -3 id_cnt (int), -4 id_ij (int), -5 n_bonds (int)
static const TrajVar kTrajVars[] = {
  {"lon", KID_B_LON, 0, "longitude", "degrees_E"}, {"lat", KID_B_LAT, 0, "latitude", "degrees_N"},
  {"year", -1, 0, "year", "years"}, {"day", -2, 0, "year day", "days"},
  {"id_cnt", -3, 0, "counter component of iceberg id", "dimensionless"}, {"id_ij", -4, 0, "position component of iceberg id", "dimensionless"},
  {"mass", KID_B_MASS, 1, "mass", "kg"}, {"start_mass", KID_B_START_MASS, 1, "start_mass", "kg"}, {"thickness", KID_B_THICKNESS, 1, "thickness", "m"},
  {"mass_of_bits", KID_B_MASS_OF_BITS, 1, "mass_of_bits", "kg"}, {"uvel", KID_B_UVEL, 1, "zonal spped", "m/s"}, {"vvel", KID_B_VVEL, 1, "meridional spped", "m/s"},
  {"mass_scaling", KID_B_MASS_SCALING, 2, "mass_scaling", "dimensionless"}, {"mass_of_fl_bits", KID_B_MASS_OF_FL_BITS, 2, "mass_of_fl_bits", "kg"},
  {"mass_of_fl_bergy_bits", KID_B_MASS_OF_FL_BERGY_BITS, 2, "mass_of_fl_bergy_bits", "kg"}, {"fl_k", KID_B_FL_K, 2, "footloose calving k", "none"},
  {"uvel_prev", KID_B_UVEL_PREV, 3, nullptr, nullptr}, {"vvel_prev", KID_B_VVEL_PREV, 3, nullptr, nullptr},
  {"uo", KID_B_UO, 3, "ocean zonal spped", "m/s"}, {"vo", KID_B_VO, 3, "ocean meridional spped", "m/s"},
  {"ui", KID_B_UI, 3, "ice zonal spped", "m/s"}, {"vi", KID_B_VI, 3, "ice meridional spped", "m/s"},
  {"ua", KID_B_UA, 3, "atmos zonal spped", "m/s"}, {"va", KID_B_VA, 3, "atmos meridional spped", "m/s"},
  {"heat_density", KID_B_HEAT_DENSITY, 3, "heat_density", "J/kg"}, {"width", KID_B_WIDTH, 3, "width", "m"}, {"length", KID_B_LENGTH, 3, "length", "m"},
  {"ssh_x", KID_B_SSH_X, 3, "sea surface height gradient_x", "non-dim"}, {"ssh_y", KID_B_SSH_Y, 3, "sea surface height gradient_y", "non-dim"},
  {"sst", KID_B_SST, 3, "sea surface temperature", "degrees_C"}, {"sss", KID_B_SSS, 3, "sea surface salinity", "psu"},
  {"cn", KID_B_CN, 3, "sea ice concentration", "none"}, {"hi", KID_B_HI, 3, "sea ice thickness", "m"},
  {"axn", KID_B_AXN, 3, "explicit zonal acceleration", "m"}, {"ayn", KID_B_AYN, 3, "explicit meridional acceleration", "m"},
  {"bxn", KID_B_BXN, 3, "implicit zonal acceleration", "m"}, {"byn", KID_B_BYN, 3, "implicit meridional acceleration", "m"},
  {"halo_berg", KID_B_HALO_BERG, 3, "halo status", "non-dim"}, {"od", KID_B_OD, 3, "ocean_depth", "m"},
  {"axn_fast", KID_B_AXN_FAST, 4, "explicit fast step zonal acceleration", "m"}, {"ayn_fast", KID_B_AYN_FAST, 4, "explicit fast step meridional acceleration", "m"},
  {"bxn_fast", KID_B_BXN_FAST, 4, "implicit fast step zonal acceleration", "m"}, {"byn_fast", KID_B_BYN_FAST, 4, "implicit fast step meridional acceleration", "m"},
  {"n_bonds", -5, 6, "number of bonds", "dimensionless"},
  {"ang_vel", KID_B_ANG_VEL, 5, "angular velocity", "rad/s"}, {"ang_accel", KID_B_ANG_ACCEL, 5, "angular acceleration", "rad/s^2"}, {"rot", KID_B_ROT, 5, "accumulated rotation", "rad"},
};
enum { KID_NTRAJ_VARS = sizeof(kTrajVars) / sizeof(kTrajVars[0]) };
static bool traj_wanted(const kid_params &p, const kid_traj_params &tp, int group) {
  switch (group) {
    case 0: return true;
    case 1: return tp.save_fl_traj != 0;
    case 2: return tp.save_fl_traj != 0 && p.footloose != 0;
    case 3: return tp.save_short_traj == 0;
    case 4: return tp.save_short_traj == 0 && p.mts != 0;
    case 5: return tp.save_short_traj == 0 && p.dem != 0;
    default: return tp.save_short_traj == 0 && p.iceberg_bonds_on != 0;
  }
}
struct TrajDev { const double *src[KID_NTRAJ_VARS]; double *dst[KID_NTRAJ_VARS]; int nf; };   // the fp64 fields to sample and where they go
}  // namespace

__global__ void __launch_bounds__(256) record_posn_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, const kid_traj_params tp, const TrajDev td,
                                                          int64_t *rec_id, int32_t *rec_nbonds, double *rec_day, int32_t *rec_year, const int32_t *bcount, unsigned long long *cursor,
                                                          long long capacity, long long n, int *overflow) {
  __shared__ int wave_tot[4];
  __shared__ unsigned long long block_base;
  const kid_params &p = *pp;
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  bool take = false;
  if (k < n && b.i[KID_BI_ALIVE][k] != 0) {
    const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
    if (i >= g.isc && i <= g.iec && j >= g.jsc && j <= g.jec) {  // FW:5346
      const double mass = b.f[KID_B_MASS][k], thick = b.f[KID_B_THICKNESS][k], fl_k = b.f[KID_B_FL_K][k];
      const double berg_area = mass / (p.rho_bergs * thick);                                                 // FW:5370
      bool by_class = false;
      if (tp.save_nonfl_traj_by_class && fl_k >= 0. && berg_area > tp.traj_area_thres_sntbc * 1.e6)         // FW:5371-5380
        by_class = b.f[KID_B_START_MASS][k] >= (b.f[KID_B_LAT][k] < 0. ? tp.save_traj_by_class_start_mass_thres_s : tp.save_traj_by_class_start_mass_thres_n);
      const bool save_fl_berg = fl_k < 0. && berg_area > tp.traj_area_thres_fl * 1.e6;                       // FW:5381-5385
      const bool bonded = bcount && bcount[k] > 0;                                                          // associated(current_bond)
      take = (double)p.current_year > tp.save_all_traj_year || by_class || berg_area >= tp.traj_area_thres * 1.e6 || bonded || save_fl_berg;  // FW:5387-5388
    }
  }
  const unsigned long long m = __ballot(take);
  const int lane = (int)__lane_id(), before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) { const int tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]; block_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull; }
  __syncthreads();
  if (!take) return;
  long long r = (long long)block_base + before;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) r += wave_tot[w];
  if (r >= capacity) { *overflow = 1; return; }
  for (int f = 0; f < td.nf; ++f) td.dst[f][r] = td.src[f][k];
  rec_id[r] = b.id[k];
  rec_day[r] = p.current_yearday; rec_year[r] = p.current_year;   // posn%day, posn%year, FW:5391-5392
  rec_nbonds[r] = bcount ? bcount[k] : b.i[KID_BI_N_BONDS][k];
}

namespace {
enum { BT_LON = 0, BT_LAT, BT_DAY, BT_LENGTH, BT_N1, BT_N2, BT_TANGD1, BT_TANGD2, BT_NSTRESS, BT_SSTRESS, BT_REL_ROTATION, BT_NF64 };
struct BondTrajDev { double *f[BT_NF64]; int64_t *id1, *id2; int32_t *year, *broken; };
}  // namespace

// one lane per (berg, slot): a bond is sampled from each of its two bergs, as the reference's loop over bergs and their
// bond lists does (FW:5456-5490); a slot whose partner is not here (other_berg not associated) is skipped
__global__ void __launch_bounds__(256) record_bond_posn_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, const MtsDev m, const BondTrajDev bt,
                                                               unsigned long long *cursor, long long capacity, long long n, int *overflow) {
  __shared__ int wave_tot[4];
  __shared__ unsigned long long block_base;
  const kid_params &p = *pp;
  const long long t = (long long)blockIdx.x * 256ll + threadIdx.x;
  const long long k = t % (n > 0 ? n : 1); const int s = (int)(t / (n > 0 ? n : 1));   // slot-major, like the bond arrays
  bool take = false; int o = -1;
  if (s < m.mb && b.i[KID_BI_ALIVE][k] != 0 && s < m.bcount[k]) {
    const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
    o = m.bother_row[MB_S(s, k)];
    take = o >= 0 && i >= g.isc && i <= g.iec && j >= g.jsc && j <= g.jec;   // a bonded berg is always sampled, FW:5387
  }
  const unsigned long long mk = __ballot(take);
  const int lane = (int)__lane_id(), before = __popcll(mk & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[threadIdx.x >> 6] = __popcll(mk);
  __syncthreads();
  if (threadIdx.x == 0) { const int tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3]; block_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull; }
  __syncthreads();
  if (!take) return;
  long long r = (long long)block_base + before;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) r += wave_tot[w];
  if (r >= capacity) { *overflow = 1; return; }
  const double lon = b.f[KID_B_LON][k], lat = b.f[KID_B_LAT][k], lon_o = b.f[KID_B_LON][o], lat_o = b.f[KID_B_LAT][o];
  double dx_dlon, dy_dlat;
  grid_to_meters(g, p, 0.5 * (lat + lat_o), dx_dlon, dy_dlat);                       // FW:5461-5467
  const double dx = (lon - lon_o) * dx_dlon, dy = (lat - lat_o) * dy_dlat, len = b.f[KID_B_LENGTH][k];
  bt.f[BT_N1][r] = dx / len; bt.f[BT_N2][r] = dy / len;                              // FW:5470: over the berg's length
  bt.f[BT_LON][r] = 0.5 * (lon + lon_o); bt.f[BT_LAT][r] = 0.5 * (lat + lat_o);      // FW:5471-5472
  bt.f[BT_DAY][r] = p.current_yearday; bt.year[r] = p.current_year;
  bt.f[BT_LENGTH][r] = MBD(KID_BOND_LENGTH, s, k);
  bt.id1[r] = b.id[k]; bt.id2[r] = b.id[o];
  bt.f[BT_TANGD1][r] = MBD(KID_BOND_TANGD1, s, k); bt.f[BT_TANGD2][r] = MBD(KID_BOND_TANGD2, s, k);   // written only with dem, FW:5478-5485
  bt.f[BT_NSTRESS][r] = MBD(KID_BOND_NSTRESS, s, k); bt.f[BT_SSTRESS][r] = MBD(KID_BOND_SSTRESS, s, k);
  bt.f[BT_REL_ROTATION][r] = MBD(KID_BOND_REL_ROTATION, s, k); bt.broken[r] = m.bbroken[MB_S(s, k)];
}

extern "C" {

int kid_set_traj_params(kid_handle *h, const kid_traj_params *tp) {
  if (!h || !tp) return KID_EINVAL;
  if (h->traj_count_bound > 0 && (tp->save_short_traj != h->traj_params.save_short_traj || tp->save_fl_traj != h->traj_params.save_fl_traj)) {
    h->err = "write the pending trajectory records before changing what a record holds"; return KID_EINVAL;
  }
  h->traj_params = *tp; h->traj_on = true;
  return KID_OK;
}

// the fp64 berg fields a record holds under the current switches, in file order
static int traj_fields(const kid_handle *h, int out[KID_NTRAJ_VARS]) {
  int nf = 0;
  for (const TrajVar &v : kTrajVars) if (v.field >= 0 && traj_wanted(h->params, h->traj_params, v.group)) out[nf++] = v.field;
  return nf;
}
static int traj_reserve(kid_handle *h, long long want) {   // room for `want` records in every buffer
  if (want <= h->traj_capacity) return KID_OK;
  long long cap = std::max<long long>(want, std::max<long long>(2 * h->traj_capacity, 1024));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  const size_t keep = (size_t)h->traj_capacity;
  for (int f = 0; f < KID_NTRAJ_VARS; ++f) if (h->traj_nf > f || h->d_traj_f[f]) KID_HIP(h, h->mem.regrow(h->d_traj_f[f], keep, (size_t)cap));
  KID_HIP(h, h->mem.regrow(h->d_traj_day, keep, (size_t)cap));
  KID_HIP(h, h->mem.regrow(h->d_traj_id, keep, (size_t)cap));
  KID_HIP(h, h->mem.regrow(h->d_traj_year, keep, (size_t)cap));
  KID_HIP(h, h->mem.regrow(h->d_traj_nbonds, keep, (size_t)cap));
  h->traj_capacity = cap;
  return KID_OK;
}

static int btraj_reserve(kid_handle *h, long long want) {   // room for `want` bond records
  if (want <= h->btraj_capacity) return KID_OK;
  const long long cap = std::max<long long>(want, std::max<long long>(2 * h->btraj_capacity, 1024));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  const size_t keep = (size_t)h->btraj_capacity;
  for (int f = 0; f < BT_NF64; ++f) KID_HIP(h, h->mem.regrow(h->d_btraj_f[f], keep, (size_t)cap));
  for (int f = 0; f < 2; ++f) { KID_HIP(h, h->mem.regrow(h->d_btraj_id[f], keep, (size_t)cap)); KID_HIP(h, h->mem.regrow(h->d_btraj_i[f], keep, (size_t)cap)); }
  h->btraj_capacity = cap;
  return KID_OK;
}

int kid_record_posn(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_record_posn"); if (rc_h) return rc_h; }
  if (!h->traj_on) { h->err = "kid_set_traj_params must be called first"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  if (h->n == 0) return KID_OK;
  { const int rc = refresh_tables(h); if (rc) return rc; }
  int fields[KID_NTRAJ_VARS];
  h->traj_nf = traj_fields(h, fields);
  if (!h->d_traj_cursor) KID_HIP(h, h->mem.dev(h->d_traj_cursor, 4, 0));
  { const int rc = traj_reserve(h, h->traj_count_bound + h->n); if (rc) return rc; }
  TrajDev td{}; td.nf = h->traj_nf;
  for (int f = 0; f < td.nf; ++f) { td.src[f] = h->bp.f[fields[f]]; td.dst[f] = h->d_traj_f[f]; }
  const unsigned nb = (unsigned)((h->n + 255) / 256);
  hipLaunchKernelGGL(record_posn_kernel, dim3(nb), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->bp, h->traj_params, td, h->d_traj_id, h->d_traj_nbonds, h->d_traj_day, h->d_traj_year,
                     (const int32_t *)(h->have_bonds ? h->mts.bcount : nullptr), h->d_traj_cursor, h->traj_capacity, (long long)h->n,
                     reinterpret_cast<int *>(h->d_traj_cursor + 1));
  KID_HIP(h, hipGetLastError());
  h->traj_count_bound += h->n;
  if (h->traj_params.save_bond_traj && h->have_bonds && h->mts.mb > 0) {   // FW:5456
    const long long slots = (long long)h->n * h->mts.mb;
    { const int rc = btraj_reserve(h, h->btraj_count_bound + slots); if (rc) return rc; }
    BondTrajDev bt{};
    for (int f = 0; f < BT_NF64; ++f) bt.f[f] = h->d_btraj_f[f];
    bt.id1 = h->d_btraj_id[0]; bt.id2 = h->d_btraj_id[1]; bt.year = h->d_btraj_i[0]; bt.broken = h->d_btraj_i[1];
    hipLaunchKernelGGL(record_bond_posn_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->bp, h->mts, bt,
                       h->d_traj_cursor + 2, h->btraj_capacity, (long long)h->n, reinterpret_cast<int *>(h->d_traj_cursor + 3));
    KID_HIP(h, hipGetLastError());
    h->btraj_count_bound += slots;
  }
  return KID_OK;
}

int kid_num_traj_records(kid_handle *h, int64_t *n) {
  if (!h || !n) return KID_EINVAL;
  *n = 0;
  if (!h->d_traj_cursor) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  unsigned long long c[2] = {0, 0};
  KID_HIP(h, hipMemcpyAsync(c, h->d_traj_cursor, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if ((int)(c[1] & 0xffffffffull)) { h->err = "trajectory buffer overflow"; return KID_ECAPACITY; }
  *n = (int64_t)c[0];
  h->traj_count_bound = (long long)c[0];   // now exact
  return KID_OK;
}

int kid_write_trajectories(kid_handle *h, const char *path) {
  if (!h || !path) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_write_trajectories"); if (rc_h) return rc_h; }
  if (!h->traj_on) { h->err = "kid_set_traj_params must be called first"; return KID_EINVAL; }
  int64_t nrec = 0;
  int rc = kid_num_traj_records(h, &nrec);
  if (rc) return rc;
  const kid_params &p = h->params;
  int fields[KID_NTRAJ_VARS];
  const int nf = traj_fields(h, fields);
  const size_t n = (size_t)std::max<int64_t>(nrec, 1);
  std::vector<std::vector<double>> col((size_t)nf, std::vector<double>(n));
  std::vector<double> day(n); std::vector<int64_t> id(n); std::vector<int32_t> year(n), nbonds(n);
  if (nrec > 0) {
    for (int f = 0; f < nf; ++f) KID_HIP(h, hipMemcpyAsync(col[(size_t)f].data(), h->d_traj_f[f], (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(day.data(), h->d_traj_day, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(id.data(), h->d_traj_id, (size_t)nrec * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(year.data(), h->d_traj_year, (size_t)nrec * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(nbonds.data(), h->d_traj_nbonds, (size_t)nrec * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
  }
  // an existing file is extended (IO2:1747-1826 reopens it and appends after the last record)
  ncfile::File old; std::string err; long long nold = 0;
  { FILE *probe = std::fopen(path, "rb"); if (probe) { std::fclose(probe); if (ncfile::read(path, old, err)) { h->err = std::string("cannot extend ") + path + ": " + err; return KID_EINVAL; }
      const ncfile::Var *lon = ncfile::find(old, "lon"); if (!lon) { h->err = std::string(path) + " is not a trajectory file"; return KID_EINVAL; } nold = ncfile::count(old, *lon); } }
  ncfile::File f;
  const long long ntot = nold + nrec;
  f.dims.emplace_back("i", ntot); f.unlimited = 0; f.numrecs = ntot;
  f.gatts = {ncfile::att_int("file_format_major_version", 0), ncfile::att_int("file_format_minor_version", 1)};   // IO2:1895-1896
  int fcol = 0;
  for (const TrajVar &v : kTrajVars) {
    if (!traj_wanted(p, h->traj_params, v.group)) continue;
    ncfile::Var nv; nv.name = v.name; nv.dims = {0}; nv.record = true;
    const bool is_int = v.field == -1 || v.field == -3 || v.field == -4 || v.field == -5;
    nv.type = is_int ? ncfile::NC_INT : ncfile::NC_DOUBLE;
    const char *ln = v.longname, *un = v.units;
    if (v.field == KID_B_UVEL_PREV && p.mts) { ln = "zonal speed mts"; un = "m/s"; }         // IO2:1980-1983
    if (v.field == KID_B_VVEL_PREV && p.mts) { ln = "meridional speed mts"; un = "m/s"; }
    if (ln) nv.atts = {ncfile::att_text("long_name", ln), ncfile::att_text("units", un)};
    const ncfile::Var *ov = nold ? ncfile::find(old, v.name) : nullptr;
    if (nold && (!ov || ncfile::count(old, *ov) != nold)) { h->err = std::string(path) + " holds other variables than the current trajectory switches give"; return KID_EINVAL; }
    if (is_int) {
      std::vector<int32_t> x((size_t)std::max<long long>(ntot, 1));
      for (long long q = 0; q < nold; ++q) x[(size_t)q] = (int32_t)ncfile::value(*ov, q);
      for (long long q = 0; q < nrec; ++q)
        x[(size_t)(nold + q)] = v.field == -1 ? year[(size_t)q] : v.field == -3 ? (int32_t)(id[(size_t)q] >> 32) : v.field == -4 ? (int32_t)(id[(size_t)q] & 0xffffffffll) : nbonds[(size_t)q];
      ncfile::set_data(nv, x.data(), ntot);
    } else {
      std::vector<double> x((size_t)std::max<long long>(ntot, 1));
      for (long long q = 0; q < nold; ++q) x[(size_t)q] = ncfile::value(*ov, q);
      const double *src = v.field == -2 ? day.data() : col[(size_t)fcol].data();
      for (long long q = 0; q < nrec; ++q) x[(size_t)(nold + q)] = src[q];
      if (v.field >= 0) ++fcol;
      ncfile::set_data(nv, x.data(), ntot);
    }
    f.vars.push_back(nv);
  }
  if (ncfile::write(f, path)) { h->err = std::string("cannot write ") + path; return KID_EINVAL; }
  KID_HIP(h, hipMemsetAsync(h->d_traj_cursor, 0, 2 * sizeof(unsigned long long), h->stream));   // the samples are on disk: start over
  h->traj_count_bound = 0;
  return KID_OK;
}

int kid_num_bond_traj_records(kid_handle *h, int64_t *n) {
  if (!h || !n) return KID_EINVAL;
  *n = 0;
  if (!h->d_traj_cursor) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  unsigned long long c[2] = {0, 0};
  KID_HIP(h, hipMemcpyAsync(c, h->d_traj_cursor + 2, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if ((int)(c[1] & 0xffffffffull)) { h->err = "bond trajectory buffer overflow"; return KID_ECAPACITY; }
  *n = (int64_t)c[0];
  h->btraj_count_bound = (long long)c[0];
  return KID_OK;
}

int kid_write_bond_trajectories(kid_handle *h, const char *path) {
  if (!h || !path) return KID_EINVAL;
  if (!h->traj_on) { h->err = "kid_set_traj_params must be called first"; return KID_EINVAL; }
  int64_t nrec = 0;
  int rc = kid_num_bond_traj_records(h, &nrec);
  if (rc) return rc;
  if (nrec == 0) return KID_OK;                       // associated(traj4io) is false: no file is touched, IO2:2172
  const bool dem = h->params.dem != 0;
  const size_t n = (size_t)nrec;
  std::vector<std::vector<double>> col(BT_NF64, std::vector<double>(n));
  std::vector<int64_t> id1(n), id2(n); std::vector<int32_t> year(n), broken(n);
  for (int f = 0; f < BT_NF64; ++f) KID_HIP(h, hipMemcpyAsync(col[(size_t)f].data(), h->d_btraj_f[f], n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipMemcpyAsync(id1.data(), h->d_btraj_id[0], n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipMemcpyAsync(id2.data(), h->d_btraj_id[1], n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipMemcpyAsync(year.data(), h->d_btraj_i[0], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipMemcpyAsync(broken.data(), h->d_btraj_i[1], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  ncfile::File old; std::string err; long long nold = 0;   // an existing file is extended, IO2:2192-2218
  { FILE *probe = std::fopen(path, "rb"); if (probe) { std::fclose(probe); if (ncfile::read(path, old, err)) { h->err = std::string("cannot extend ") + path + ": " + err; return KID_EINVAL; }
      const ncfile::Var *lon = ncfile::find(old, "lon"); if (!lon || !ncfile::find(old, "id_cnt1")) { h->err = std::string(path) + " is not a bond trajectory file"; return KID_EINVAL; } nold = ncfile::count(old, *lon); } }
  // order of the def_var calls, IO2:2222-2240; field: >= 0 a BT_ column, -1 year, -3/-4 id1 halves, -5/-6 id2 halves, -7 broken
  struct BV { const char *name; int field; bool dem_only; const char *longname, *units; };
  static const BV vars[] = {
    {"lon", BT_LON, false, "longitude", "degrees_E"}, {"lat", BT_LAT, false, "latitude", "degrees_N"},
    {"year", -1, false, "year", "years"}, {"day", BT_DAY, false, "year day", "days"},
    {"length", BT_LENGTH, false, "length", "m"}, {"n1", BT_N1, false, "unit vector 1", "non-dim"}, {"n2", BT_N2, false, "unit vector 2", "non-dim"},
    {"id_cnt1", -3, false, "counter component of first connected iceberg id", "dimensionless"},
    {"id_ij1", -4, false, "position component of first connected iceberg id", "dimensionless"},
    {"id_cnt2", -5, false, "counter component of second connected iceberg id", "dimensionless"},
    {"id_ij2", -6, false, "position component of second connected iceberg id", "dimensionless"},
    {"tangd1", BT_TANGD1, true, "zonal tangential displacement", "m"}, {"tangd2", BT_TANGD2, true, "meridional tangential displacement", "m"},
    {"nstress", BT_NSTRESS, true, "normal stress", "Pa"}, {"sstress", BT_SSTRESS, true, "shear stress", "Pa"},
    {"rel_rotation", BT_REL_ROTATION, true, "relative rotation", "rad"}, {"broken", -7, true, "broken status", "none"},
  };
  ncfile::File f;
  const long long ntot = nold + nrec;
  f.dims.emplace_back("i", ntot); f.unlimited = 0; f.numrecs = ntot;
  f.gatts = {ncfile::att_int("file_format_major_version", 0), ncfile::att_int("file_format_minor_version", 1)};   // IO2:2242-2243
  for (const BV &v : vars) {
    if (v.dem_only && !dem) continue;
    ncfile::Var nv; nv.name = v.name; nv.dims = {0}; nv.record = true;
    const bool is_int = v.field < 0;
    nv.type = is_int ? ncfile::NC_INT : ncfile::NC_DOUBLE;
    nv.atts = {ncfile::att_text("long_name", v.longname), ncfile::att_text("units", v.units)};
    const ncfile::Var *ov = nold ? ncfile::find(old, v.name) : nullptr;
    if (nold && (!ov || ncfile::count(old, *ov) != nold)) { h->err = std::string(path) + " holds other variables than the current switches give"; return KID_EINVAL; }
    if (is_int) {
      std::vector<int32_t> x((size_t)ntot);
      for (long long q = 0; q < nold; ++q) x[(size_t)q] = (int32_t)ncfile::value(*ov, q);
      for (long long q = 0; q < nrec; ++q) {
        const size_t u = (size_t)q;
        x[(size_t)(nold + q)] = v.field == -1 ? year[u] : v.field == -3 ? (int32_t)(id1[u] >> 32) : v.field == -4 ? (int32_t)(id1[u] & 0xffffffffll)
                              : v.field == -5 ? (int32_t)(id2[u] >> 32) : v.field == -6 ? (int32_t)(id2[u] & 0xffffffffll) : broken[u];
      }
      ncfile::set_data(nv, x.data(), ntot);
    } else {
      std::vector<double> x((size_t)ntot);
      for (long long q = 0; q < nold; ++q) x[(size_t)q] = ncfile::value(*ov, q);
      for (long long q = 0; q < nrec; ++q) x[(size_t)(nold + q)] = col[(size_t)v.field][(size_t)q];
      ncfile::set_data(nv, x.data(), ntot);
    }
    f.vars.push_back(nv);
  }
  if (ncfile::write(f, path)) { h->err = std::string("cannot write ") + path; return KID_EINVAL; }
  KID_HIP(h, hipMemsetAsync(h->d_traj_cursor + 2, 0, 2 * sizeof(unsigned long long), h->stream));
  h->btraj_count_bound = 0;
  return KID_OK;
}

}  // extern "C"
