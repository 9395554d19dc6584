// kid_calving.inc -- the calving source on the device (SURVEY.md 8f N3):
//   the calving block of icebergs_run  /root/reference/src/icebergs.F90:5203-5231, 5397
//   get_running_mean_calving           IB:5999-6038
//   accumulate_calving                 IB:6153-6222
//   calve_icebergs                     IB:6225-6402  (generate_id FW:4165-4179)
// Everything up to the bucket overflow is pointwise in the cell, so it is ONE per-cell launch over the data domain
// (calving_accumulate_kernel); the budget sums it feeds are reduced per workgroup and added with one atomic each.
// calve_icebergs is one thread per cell of the computational domain: the class loop and the `do while` of a cell are
// sequential in the reference too (stored_heat and the id counter of the cell thread through them), cells are
// independent, and new bergs are appended to the SoA through an atomic cursor like footloose children.
struct CalvingDev {
  const double *calving_in, *hflx_in;   // (isc:iec, jsc:jec)
  double *calving, *hflx;               // grd%calving, grd%calving_hflx (data domain)
  double *stored_ice, *stored_heat, *real_calving, *rmean_calving, *rmean_hflx;
  const double *area, *msk, *lat;
  double *scal;                         // KID_NCALV_SCALARS
  double *part;                         // per-workgroup partial sums
  unsigned char *calved_flag;           // the cell calved in the previous call (its real_calving entries are not zero)
  int ni, nj, ic0, ic1, jc0, jc1;
  double dt, alpha, beta, rd_s, rd_n;
  int do_rmean, init_rmean, init_rmean_hflx, first_call;
  kid_calving_params cp;
};

// Budget sums: every workgroup leaves its partial in part[block * stride + q]; calving_finish_kernel adds the partials
// of one scalar in a fixed order (same-address fp64 atomics from thousands of workgroups serialise, and their order
// would make the sums irreproducible).
__device__ __forceinline__ void calving_block_put(double v, double *part, double *lds4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *part = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}
enum { CALV_PART_ACC = 8, CALV_PART_CALVE = 4 + 2 * KID_NCLASSES };
struct CalvFinish { const double *part; int nblocks, stride; double *scal; int dst[CALV_PART_CALVE]; const unsigned long long *entries; };  // entries: nblocks = ceil((*entries >> 32) / 256)
__global__ void __launch_bounds__(256) calving_finish_kernel(const CalvFinish f) {
  __shared__ double red[256];
  const int q = blockIdx.x;
  const int nblocks = f.entries ? ((int)(*f.entries >> 32) + 255) / 256 : f.nblocks;
  double v = 0.;
  for (int b = threadIdx.x; b < nblocks; b += 256) v += f.part[(size_t)b * f.stride + q];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0 && f.dst[q] >= 0) f.scal[f.dst[q]] = red[0];
}

__global__ void __launch_bounds__(256) calving_accumulate_kernel(const CalvingDev a) {
  __shared__ double lds4[4];
  const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const size_t ncell = (size_t)a.ni * a.nj;
  const bool live = c < (long long)ncell;
  const int i = live ? (int)(c % a.ni) : 0, j = live ? (int)(c / a.ni) : 0;
  const bool in_c = live && i >= a.ic0 && i <= a.ic1 && j >= a.jc0 && j <= a.jc1;
  double s_recv = 0., s_inc = 0., s_inch = 0., s_st = 0., s_sth = 0., s_used = 0., s_hused = 0., s_unused = 0.;
  if (live) {
    const double area = a.area[c], msk = a.msk[c];
    double calving = a.calving[c], hflx = a.hflx[c];
    if (in_c) {  // IB:5203-5212
      const size_t q = (size_t)(i - a.ic0) + (size_t)(j - a.jc0) * (a.ic1 - a.ic0 + 1);
      const double cin = a.calving_in[q];
      s_recv = cin * area;
      hflx = a.hflx_in[q] * msk;
      calving = cin * msk;
    }
    if (a.do_rmean) {  // IB:5215-5219, 5999-6038
      double rm = a.init_rmean ? calving : a.rmean_calving[c];
      double rh = a.init_rmean_hflx ? hflx : a.rmean_hflx[c];
      if (a.alpha != 0.) {
        rm = a.beta * calving + a.alpha * rm; rh = a.beta * hflx + a.alpha * rh;
        calving = rm; hflx = rh;
      }
      a.rmean_calving[c] = rm; a.rmean_hflx[c] = rh;
    }
    calving = calving * msk * area;   // IB:5221, kg/s
    hflx = hflx * msk;                // IB:5227
    if (in_c) { s_inc = calving; s_inch = hflx * area; }
    double stored_heat = a.stored_heat[c];
    if (a.first_call && in_c) {       // IB:6171-6190
      double sum_ice = 0.;
      for (int k = 0; k < KID_NCLASSES; ++k) sum_ice += a.stored_ice[k * ncell + c];
      s_st = sum_ice;
      if (calving != 0.) stored_heat = sum_ice * hflx * area / calving;
      s_sth = stored_heat;
    }
    const bool south = a.lat[c] < 0.;
    for (int k = 0; k < KID_NCLASSES; ++k)  // IB:6192-6198
      a.stored_ice[k * ncell + c] = a.stored_ice[k * ncell + c] + a.dt * calving * (south ? a.cp.distribution_s[k] : a.cp.distribution_n[k]);
    const double rd = south ? a.rd_s : a.rd_n;
    if (in_c) s_used = calving * (1. - rd);          // IB:6211
    calving = calving * rd;                          // IB:6214
    const double tmp = a.dt * hflx * area * (1. - rd);  // IB:6217
    if (in_c) s_hused = tmp;
    stored_heat = stored_heat + tmp;                 // IB:6219
    hflx = hflx * rd;                                // IB:6220
    if (in_c) s_unused = calving;                    // IB:5397
    a.calving[c] = calving; a.hflx[c] = hflx; a.stored_heat[c] = stored_heat;
  }
  double *part = a.part + (size_t)blockIdx.x * CALV_PART_ACC;
  calving_block_put(s_recv * a.dt, part + 0, lds4);
  calving_block_put(s_inc * a.dt, part + 1, lds4);
  calving_block_put(s_inch * a.dt, part + 2, lds4);
  calving_block_put(s_st, part + 3, lds4);
  calving_block_put(s_sth, part + 4, lds4);
  calving_block_put(s_used * a.dt, part + 5, lds4);
  calving_block_put(s_hused, part + 6, lds4);
  calving_block_put(s_unused, part + 7, lds4);
}

// calve_icebergs in two launches.  calve_count_kernel is the light, bandwidth-bound pass over every cell of the
// computational domain: the `do while` of IB:6273 without its side effects gives the number of bergs the cell calves;
// a workgroup reserves the rows of the SoA and the entries of the list of calving cells with one atomic each.
// calve_emit_kernel is the heavy pass (position in the cell, interpolation, ~70 stores per berg) over that list only:
// every lane has work, and the registers that pass needs do not throttle the streaming pass.
// reserve: ONE 64-bit word, rows appended in the low half and calving cells listed in the high half, so that a workgroup
// reserves both with a single atomic (same-line atomics from thousands of workgroups serialise at ~10 ns each)
struct CalveCtx { unsigned long long *reserve; int32_t *counter; long long n, capacity; int iNg, ij0; int2 *list; };

__global__ void __launch_bounds__(1024) calve_count_kernel(const DevGrid g, const kid_params *pp, const CalvingDev a, const CalveCtx cx) {
  __shared__ int wave_tot[16], wave_cells[16], block_base, block_list;
  const kid_params &p = *pp;
  const int nic = a.ic1 - a.ic0 + 1, njc = a.jc1 - a.jc0 + 1;
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const bool live = t < (long long)nic * njc;
  const int i = live ? g.isc + (int)(t % nic) : g.isc, j = live ? g.jsc + (int)(t / nic) : g.jsc;
  const int c = g.idx(i, j);
  const size_t ncell = (size_t)a.ni * a.nj;
  int mine = 0;
  if (live) {
    const bool south = a.lat[c] < 0.;
    double st[KID_NCLASSES];
#pragma unroll
    for (int k = 0; k < KID_NCLASSES; ++k) st[k] = a.stored_ice[k * ncell + c];  // ten loads in flight
#pragma unroll
    for (int k = 0; k < KID_NCLASSES; ++k) {
      const double bucket = (south ? p.initial_mass_s[k] : p.initial_mass_n[k]) * (south ? a.cp.mass_scaling_s[k] : a.cp.mass_scaling_n[k]);
      double stored = st[k];
      while (stored >= bucket) { stored = stored - bucket; ++mine; }
    }
    // grd%real_calving is zero wherever nothing calved (IB:6253): a cell rewrites its ten entries only if it calves now
    // (calve_emit_kernel) or did in the previous call (one flag byte per cell): a quiet cell costs the ten loads above
    if (mine == 0 && a.calved_flag[c] != 0) {
      for (int k = 0; k < KID_NCLASSES; ++k) a.real_calving[k * ncell + c] = 0.;
      a.calved_flag[c] = 0;
    }
  }
  int incl = mine;  // inclusive scan over the wave
  for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off); if ((int)__lane_id() >= off) incl += o; }
  const unsigned long long calving = __ballot(mine > 0);
  const int before = __popcll(calving & ((1ull << __lane_id()) - 1ull));
  if (__lane_id() == 63) { wave_tot[threadIdx.x >> 6] = incl; wave_cells[threadIdx.x >> 6] = __popcll(calving); }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0, cells = 0;
    for (int w = 0; w < 16; ++w) { tot += wave_tot[w]; cells += wave_cells[w]; }
    const unsigned long long old = cells ? atomicAdd(cx.reserve, ((unsigned long long)cells << 32) | (unsigned long long)tot) : 0ull;
    block_base = (int)(old & 0xffffffffull); block_list = (int)(old >> 32);
  }
  __syncthreads();
  if (mine > 0) {
    int slot = block_base + (incl - mine), pos = block_list + before;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) { slot += wave_tot[w]; pos += wave_cells[w]; }
    cx.list[pos] = make_int2((int)t, slot);
  }
}

// The field-pointer table comes BY VALUE (kernel argument): read through a pointer, every store to a berg field could
// alias the table and each of the ~70 stores of a new berg would wait for a fresh load of the next field pointer.
__global__ void __launch_bounds__(256) calve_emit_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, const CalvingDev a, const CalveCtx cx) {
  __shared__ double lds4[4];
  __shared__ int cls[2 * KID_NCLASSES];
  const kid_params &p = *pp;
  const int nic = a.ic1 - a.ic0 + 1;
  const int ncalving = (int)(*cx.reserve >> 32);
  if ((int)(blockIdx.x * blockDim.x) >= ncalving) return;  // the launch is sized for "every cell calves"
  const int entry = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = entry < ncalving;
  if (threadIdx.x < 2 * KID_NCLASSES) cls[threadIdx.x] = 0;
  __syncthreads();
  double to_bergs = 0., heat_to_bergs = 0., nerr = 0., ntot = 0.;
  if (live) {
    const int2 ent = cx.list[entry];
    const int i = g.isc + ent.x % nic, j = g.jsc + ent.x / nic;
    int slot = ent.y;
    const int c = g.idx(i, j);
    const size_t ncell = (size_t)a.ni * a.nj;
    const bool south = a.lat[c] < 0.;
    a.calved_flag[c] = 1;
    double stored_heat = a.stored_heat[c];
    int32_t cnt = cx.counter[c];  // grd%iceberg_counter_grd(i,j): this thread is its only writer in this launch
    // every berg of the cell is born at the same point: the mean of the four corners, IB:6274-6275
    const GlbCell cell{g, c};
    const Corners cq = cell.corners();
    const double blon = 0.25 * ((cq.lon11 + cq.lon00) + (cq.lon01 + cq.lon10));
    const double blat = 0.25 * ((cq.lat11 + cq.lat00) + (cq.lat01 + cq.lat10));
    double xi, yj;
    Env e{};
    {
      int err = 0; bool bail = false;
      // (once per calving cell: the reference's own operations, so that what a new berg starts with equals the reference's bit for bit)
      if (!pos_within_cell<false, 0, false, true>(g, p, cell, blon, blat, i, j, xi, yj, err, bail)) nerr += 1.;  // FATAL IB:6281
      if (!p.old_interp_flds_order) interp_flds<0, false, true>(p, cell, xi, yj, e);                             // IB:6353-6364
    }
    double st[KID_NCLASSES];
#pragma unroll
    for (int k = 0; k < KID_NCLASSES; ++k) st[k] = a.stored_ice[k * ncell + c];  // one memory latency, not ten in a chain
#pragma unroll
    for (int k = 0; k < KID_NCLASSES; ++k) {
      const double initial_mass = south ? p.initial_mass_s[k] : p.initial_mass_n[k];  // IB:6262-6270
      const double mass_scaling = south ? a.cp.mass_scaling_s[k] : a.cp.mass_scaling_n[k];
      const double bucket = initial_mass * mass_scaling;
      double stored = st[k], real_calving = 0., ddt = 0.;
      int ncalved = 0;
#pragma unroll 1
      while (stored >= bucket) {  // IB:6273
        const long long q = cx.n + slot++;
        const double heat_density = stored_heat / stored;  // IB:6329, J/kg
        if (q < cx.capacity) {
#pragma unroll
          for (int f = 0; f < KID_NB_F64; ++f) b.f[f][q] = 0.0;  // velocities, accelerations, bits, fl_k, halo/static, mts and dem fields
          b.f[KID_B_LON][q] = blon; b.f[KID_B_LAT][q] = blat; b.f[KID_B_XI][q] = xi; b.f[KID_B_YJ][q] = yj;
          b.i[KID_BI_INE][q] = i; b.i[KID_BI_JNE][q] = j;
          if (p.interactive_icebergs_on || p.footloose) { b.f[KID_B_LON_OLD][q] = blon; b.f[KID_B_LAT_OLD][q] = blat; }  // IB:6297-6305
          b.f[KID_B_MASS][q] = initial_mass;
          b.f[KID_B_THICKNESS][q] = south ? a.cp.initial_thickness_s[k] : a.cp.initial_thickness_n[k];
          b.f[KID_B_WIDTH][q] = south ? a.cp.initial_width_s[k] : a.cp.initial_width_n[k];
          b.f[KID_B_LENGTH][q] = south ? a.cp.initial_length_s[k] : a.cp.initial_length_n[k];
          b.f[KID_B_START_LON][q] = blon; b.f[KID_B_START_LAT][q] = blat;
          b.i[KID_BI_START_YEAR][q] = p.current_year;
          {  // generate_id FW:4165-4179
            cnt += 1;
            const int32_t ij = i + (cx.iNg * (j - 1)) + cx.ij0;
            b.id[q] = (int64_t)cnt * ((int64_t)1 << 32) + (int64_t)ij;
          }
          b.f[KID_B_START_DAY][q] = p.current_yearday + ddt / 86400.;
          b.f[KID_B_START_MASS][q] = initial_mass; b.f[KID_B_MASS_SCALING][q] = mass_scaling;
          b.f[KID_B_HEAT_DENSITY][q] = heat_density;
          b.i[KID_BI_N_BONDS][q] = 0; b.i[KID_BI_CONGLOM_ID][q] = 0; b.i[KID_BI_ALIVE][q] = 1;
          if (!p.old_interp_flds_order) {
            b.f[KID_B_UO][q] = e.uo; b.f[KID_B_VO][q] = e.vo; b.f[KID_B_UI][q] = e.ui; b.f[KID_B_VI][q] = e.vi;
            b.f[KID_B_UA][q] = e.ua; b.f[KID_B_VA][q] = e.va; b.f[KID_B_SSH_X][q] = e.ssh_x; b.f[KID_B_SSH_Y][q] = e.ssh_y;
            b.f[KID_B_SST][q] = e.sst; b.f[KID_B_SSS][q] = e.sss; b.f[KID_B_CN][q] = e.cn; b.f[KID_B_HI][q] = e.hi; b.f[KID_B_OD][q] = e.od;
          }
        } else { cnt += 1; nerr += 1.; }  // the SoA is full: the host reports KID_ECAPACITY; the buckets are still drained as in the reference
        const double heat_to_berg = bucket * heat_density;  // IB:6367-6383
        stored_heat = stored_heat - heat_to_berg;
        heat_to_bergs = heat_to_bergs + heat_to_berg;
        stored = stored - bucket;
        to_bergs = to_bergs + bucket;
        real_calving = real_calving + bucket / p.dt;
        ddt = ddt - p.dt * 2. / 17.;
        ++ncalved;
      }
      a.real_calving[k * ncell + c] = real_calving;
      if (ncalved) {
        a.stored_ice[k * ncell + c] = stored;
        atomicAdd(&cls[(south ? 0 : KID_NCLASSES) + k], ncalved);
        ntot += (double)ncalved;
      }
    }
    a.stored_heat[c] = stored_heat;
    cx.counter[c] = cnt;
  }
  double *part = a.part + (size_t)blockIdx.x * CALV_PART_CALVE;
  calving_block_put(to_bergs, part + 0, lds4);
  calving_block_put(heat_to_bergs, part + 1, lds4);
  calving_block_put(nerr, part + 2, lds4);
  calving_block_put(ntot, part + 3, lds4);  // the barriers inside these calls also complete the LDS class counters
  if (threadIdx.x < 2 * KID_NCLASSES) part[4 + threadIdx.x] = (double)cls[threadIdx.x];
}

static int calving_ensure(kid_handle *h) {
  if (h->d_calv_state) return KID_OK;
  const size_t planes = 2 + 2 * KID_NCLASSES + 1 + 2;  // calving, hflx, stored_ice, real_calving, stored_heat, two running means
  KID_HIP(h, h->mem.dev(h->d_calv_state, planes * h->ncell, 0));
  // one small block: the KID_NCALV_SCALARS sums, then the row cursor and the calving-cell count (one memset, one copy back)
  KID_HIP(h, h->mem.dev(h->d_calv_scal, KID_NCALV_SCALARS + 1));
  KID_HIP(h, h->mem.pinned(h->calv_host, KID_NCALV_SCALARS + 1));
  KID_HIP(h, h->mem.dev(h->d_calv_flag, h->ncell, 0));
  KID_HIP(h, h->mem.dev(h->d_calv_list, h->ncell));
  KID_HIP(h, h->mem.dev(h->d_calv_part, (h->ncell + 255) / 256 * (CALV_PART_ACC + CALV_PART_CALVE)));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}
static double *calv_plane(kid_handle *h, int which) { return h->d_calv_state + (size_t)which * h->ncell; }
enum { CALV_CALVING = 0, CALV_HFLX = 1, CALV_STORED_ICE = 2, CALV_REAL = 2 + KID_NCLASSES, CALV_STORED_HEAT = 2 + 2 * KID_NCLASSES, CALV_RMEAN = 3 + 2 * KID_NCLASSES, CALV_RMEAN_HFLX = 4 + 2 * KID_NCLASSES };

int kid_set_calving_params(kid_handle *h, const kid_calving_params *cp) {
  if (!h || !cp) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = calving_ensure(h); if (rc) return rc; }
  h->calv_params = *cp;
  h->calving_on = true;
  return KID_OK;
}

// read_restart_calving (stored_ice, stored_heat, the running means): data-domain planes; NULL keeps what the handle holds
int kid_set_calving_state(kid_handle *h, const double *stored_ice, const double *stored_heat, const double *rmean_calving, const double *rmean_calving_hflx) {
  if (!h) return KID_EINVAL;
  if (!h->calving_on) { h->err = "kid_set_calving_params must be called first"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  const size_t pb = h->ncell * sizeof(double);
  if (stored_ice) KID_HIP(h, hipMemcpyAsync(calv_plane(h, CALV_STORED_ICE), stored_ice, KID_NCLASSES * pb, hipMemcpyHostToDevice, h->stream));
  if (stored_heat) KID_HIP(h, hipMemcpyAsync(calv_plane(h, CALV_STORED_HEAT), stored_heat, pb, hipMemcpyHostToDevice, h->stream));
  if (rmean_calving) { KID_HIP(h, hipMemcpyAsync(calv_plane(h, CALV_RMEAN), rmean_calving, pb, hipMemcpyHostToDevice, h->stream)); h->rmean_init = true; }
  if (rmean_calving_hflx) { KID_HIP(h, hipMemcpyAsync(calv_plane(h, CALV_RMEAN_HFLX), rmean_calving_hflx, pb, hipMemcpyHostToDevice, h->stream)); h->rmean_hflx_init = true; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_get_calving_state(kid_handle *h, double *stored_ice, double *stored_heat, double *rmean_calving, double *rmean_calving_hflx, double *real_calving) {
  if (!h) return KID_EINVAL;
  if (!h->calving_on) { h->err = "kid_set_calving_params must be called first"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  const size_t pb = h->ncell * sizeof(double);
  if (stored_ice) KID_HIP(h, hipMemcpyAsync(stored_ice, calv_plane(h, CALV_STORED_ICE), KID_NCLASSES * pb, hipMemcpyDeviceToHost, h->stream));
  if (stored_heat) KID_HIP(h, hipMemcpyAsync(stored_heat, calv_plane(h, CALV_STORED_HEAT), pb, hipMemcpyDeviceToHost, h->stream));
  if (rmean_calving) KID_HIP(h, hipMemcpyAsync(rmean_calving, calv_plane(h, CALV_RMEAN), pb, hipMemcpyDeviceToHost, h->stream));
  if (rmean_calving_hflx) KID_HIP(h, hipMemcpyAsync(rmean_calving_hflx, calv_plane(h, CALV_RMEAN_HFLX), pb, hipMemcpyDeviceToHost, h->stream));
  if (real_calving) KID_HIP(h, hipMemcpyAsync(real_calving, calv_plane(h, CALV_REAL), KID_NCLASSES * pb, hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_get_calving(kid_handle *h, double *calving, double *calving_hflx) {
  if (!h) return KID_EINVAL;
  if (!h->calving_on) { h->err = "kid_set_calving_params must be called first"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  const size_t pb = h->ncell * sizeof(double);
  if (calving) KID_HIP(h, hipMemcpyAsync(calving, calv_plane(h, CALV_CALVING), pb, hipMemcpyDeviceToHost, h->stream));
  if (calving_hflx) KID_HIP(h, hipMemcpyAsync(calving_hflx, calv_plane(h, CALV_HFLX), pb, hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_calving(kid_handle *h, const kid_calving_in *in, double *scalars) {
  if (!h || !in || !in->calving || !in->calving_hflx) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_calving"); if (rc_h) return rc_h; }
  if (!h->calving_on) { h->err = "kid_set_calving_params must be called first"; return KID_EINVAL; }
  if (need_static(h)) return KID_EINVAL;
  if (!h->params.old_interp_flds_order && !h->forc.have_forcing) { h->err = "new bergs interpolate the forcing (IB:6353): set it before kid_calving"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }   // new rows must start in the hot lane
  { const int rc = refresh_tables(h); if (rc) return rc; }
  const kid_grid_desc &d = h->gd;
  const size_t n0 = (size_t)(d.iec - d.isc + 1) * (d.jec - d.jsc + 1);
  CalvingDev a{};
  if (in->on_device) { a.calving_in = in->calving; a.hflx_in = in->calving_hflx; }
  else {
    { const int rc = ingest_stage_reserve(h, 2 * n0); if (rc) return rc; }
    KID_HIP(h, hipMemcpyAsync(h->d_ingest_stage, in->calving, n0 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KID_HIP(h, hipMemcpyAsync(h->d_ingest_stage + n0, in->calving_hflx, n0 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a.calving_in = h->d_ingest_stage; a.hflx_in = h->d_ingest_stage + n0;
  }
  a.calving = calv_plane(h, CALV_CALVING); a.hflx = calv_plane(h, CALV_HFLX);
  a.stored_ice = calv_plane(h, CALV_STORED_ICE); a.stored_heat = calv_plane(h, CALV_STORED_HEAT); a.real_calving = calv_plane(h, CALV_REAL);
  a.rmean_calving = calv_plane(h, CALV_RMEAN); a.rmean_hflx = calv_plane(h, CALV_RMEAN_HFLX);
  a.area = h->d_static[KID_G_AREA]; a.msk = h->d_static[KID_G_MSK]; a.lat = h->d_static[KID_G_LAT];
  a.scal = h->d_calv_scal; a.calved_flag = h->d_calv_flag;
  a.ni = h->ni; a.nj = h->nj; a.ic0 = d.isc - d.isd; a.ic1 = d.iec - d.isd; a.jc0 = d.jsc - d.jsd; a.jc1 = d.jec - d.jsd;
  a.dt = h->params.dt; a.cp = h->calv_params;
  const kid_calving_params &cp = h->calv_params;
  if (cp.tau_calving > 0.) {  // IB:6020-6028
    a.do_rmean = 1; a.init_rmean = h->rmean_init ? 0 : 1; a.init_rmean_hflx = h->rmean_hflx_init ? 0 : 1;
    h->rmean_init = h->rmean_hflx_init = true;
    const double tau = cp.tau_calving / (365. * 24 * 60 * 60);
    a.alpha = tau / (tau + a.dt);
    if (a.alpha != 0.) { if (a.alpha > 0.5) { a.beta = a.dt / (tau + a.dt); a.alpha = 1. - a.beta; } else a.beta = 1. - a.alpha; }
  }
  a.first_call = (h->calving_first_call && !cp.restarted) ? 1 : 0;
  if (a.first_call) h->calving_first_call = false;
  a.rd_s = 1.; a.rd_n = 1.;
  for (int k = 0; k < KID_NCLASSES; ++k) { a.rd_s = a.rd_s - cp.distribution_s[k]; a.rd_n = a.rd_n - cp.distribution_n[k]; }  // IB:6199-6200
  unsigned long long *d_reserve = reinterpret_cast<unsigned long long *>(h->d_calv_scal + KID_NCALV_SCALARS);
  KID_HIP(h, hipMemsetAsync(h->d_calv_scal, 0, (KID_NCALV_SCALARS + 1) * sizeof(double), h->stream));
  const int nb_acc = (int)((h->ncell + 255) / 256), nb_calve = (int)((n0 + 255) / 256);
  a.part = h->d_calv_part;
  hipLaunchKernelGGL(calving_accumulate_kernel, dim3(nb_acc), dim3(256), 0, h->stream, a);
  {
    CalvFinish f{a.part, nb_acc, CALV_PART_ACC, a.scal, {}, nullptr};
    const int dst[CALV_PART_ACC] = {KID_CS_NET_CALVING_RECEIVED, KID_CS_NET_INCOMING_CALVING, KID_CS_NET_INCOMING_CALVING_HEAT,
                                    a.first_call ? KID_CS_STORED_START : -1, a.first_call ? KID_CS_STORED_HEAT_START : -1,
                                    KID_CS_NET_CALVING_USED, KID_CS_NET_INCOMING_CALVING_HEAT_USED, KID_CS_UNUSED_CALVING};
    for (int q = 0; q < CALV_PART_ACC; ++q) f.dst[q] = dst[q];
    hipLaunchKernelGGL(calving_finish_kernel, dim3(CALV_PART_ACC), dim3(256), 0, h->stream, f);
  }
  const CalveCtx cx{d_reserve, h->d_iceberg_counter, (long long)h->n, (long long)h->capacity, id_iNg(d), id_ij0(d), h->d_calv_list};
  a.part = h->d_calv_part + (size_t)nb_acc * CALV_PART_ACC;
  hipLaunchKernelGGL(calve_count_kernel, dim3((unsigned)((n0 + 1023) / 1024)), dim3(1024), 0, h->stream, dev_grid(h), h->d_params, a, cx);
  CalveCtx cx_emit = cx;
  if (h->auto_growth != 0.) {
    // auto-reserve: the count pass has reserved every row the call appends; read that word (the one extra synchronisation of
    // the mode), grow, and hand the new capacity and field pointers to the emit pass
    unsigned long long word = 0ull;
    KID_HIP(h, hipGetLastError());
    KID_HIP(h, hipMemcpyAsync(&word, d_reserve, sizeof(word), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    const int rc_a = auto_reserve(h, h->n + (int64_t)(word & 0xffffffffull), "kid_calving");
    if (rc_a) return rc_a;   // (the buckets keep their ice: nothing was emitted)
    cx_emit.capacity = (long long)h->capacity;
  }
  hipLaunchKernelGGL(calve_emit_kernel, dim3(nb_calve), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->bp, a, cx_emit);
  {
    CalvFinish f{a.part, nb_calve, CALV_PART_CALVE, a.scal, {}, d_reserve};
    f.dst[0] = KID_CS_NET_CALVING_TO_BERGS; f.dst[1] = KID_CS_NET_HEAT_TO_BERGS; f.dst[2] = KID_CS_ERROR_COUNT; f.dst[3] = KID_CS_NBERGS_CALVED;
    for (int k = 0; k < KID_NCLASSES; ++k) { f.dst[4 + k] = KID_CS_NBERGS_CALVED_BY_CLASS_S + k; f.dst[4 + KID_NCLASSES + k] = KID_CS_NBERGS_CALVED_BY_CLASS_N + k; }
    hipLaunchKernelGGL(calving_finish_kernel, dim3(CALV_PART_CALVE), dim3(256), 0, h->stream, f);
  }
  KID_HIP(h, hipGetLastError());
  // the population grew: the host needs the new size before the next launch (pinned mirror: one asynchronous copy)
  KID_HIP(h, hipMemcpyAsync(h->calv_host, h->d_calv_scal, (KID_NCALV_SCALARS + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  const int appended = (int)(reinterpret_cast<const unsigned long long *>(h->calv_host + KID_NCALV_SCALARS)[0] & 0xffffffffull);
  if (scalars) for (int q = 0; q < KID_NCALV_SCALARS; ++q) scalars[q] = h->calv_host[q];
  return rows_appended(h, appended, nullptr, "calving ran out of capacity: create the handle with room for new bergs");
}
