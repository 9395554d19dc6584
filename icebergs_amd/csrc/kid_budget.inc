// kid_budget.inc -- mass and heat budgets on the resident state: kid_budget (the budget block of icebergs_run, IB:5702-5727),
// kid_stock (icebergs_stock_pe, IB:8102-8133) and kid_incr_mass (icebergs_incr_mass, IB:6046-6074).
// Included by kid_hip.hip after kid_bond_init.inc (it uses repro_static_order of kid_repro.inc).
//
// One sweep serves every quantity.  budget_berg_kernel: a lane per row, the nine fields of the row loaded in one batch, the
// terms of sum_mass / sum_heat (FW:6606-6666) formed for the rows that count -- alive, cell on the computational domain, the
// test of bergs_chksum (kid_chksum.inc) -- and +0 for the others.  budget_cell_kernel: a lane per computational cell, the ten
// classes of grd%stored_ice added in class order, and grd%stored_heat.  Both reduce a block of 256 the same way: a butterfly
// over the 64 lanes of a wave, the four wave sums through LDS as (w0 + w1) + (w2 + w3), one partial per quantity and block.
// budget_finish_kernel, one block: thread t adds the partials t, t + 256, ... in turn, then the same block tree.
// No floating-point atomics anywhere: the shape of the sum depends on the number of rows (cells) only, so two calls on the same
// resident state give the same bits.  The berg count rides the same tree as a double: a sum of ones below 2^53 is exact.
// Reproducible mode: `order` holds the rows in the static order of kid_repro.inc with the rows that count first (a stable
// one-bit radix pass), lane q takes row order[q].  The rows that count then sit at positions 0 .. m-1 whatever the layout, and
// everything behind them adds +0, which changes no bit of a tree whose sums start from +0: the result is a function of the set
// of bergs only.  It is not the reference's serial sum (FW:6617-6631 adds one berg after the other); the two differ by rounding.
namespace {

enum { BUD_NBERGS = 0, BUD_FLOATING_MASS, BUD_ICEBERGS_MASS, BUD_BERGY_MASS, BUD_FL_BITS_MASS, BUD_FLOATING_HEAT, BUD_NQ_BERG,
       BUD_STORED = BUD_NQ_BERG, BUD_STORED_HEAT, BUD_NQ, BUD_NQ_CELL = BUD_NQ - BUD_NQ_BERG,
       BUD_NET_HEAT_TO_OCEAN = BUD_NQ, BUD_NBERGS_MELTED, BUD_NBERGS_CALVED_FL, BUD_NSPEEDING_TICKETS, BUD_NRES };

// NQ sums over a block of 256, every thread gets them (one barrier; lds is written once per call of the kernel)
template <int NQ>
__device__ __forceinline__ void budget_block_sum(double (&x)[NQ], double (*lds)[4]) {
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) x[k] = x[k] + __shfl_xor(x[k], d);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) lds[k][threadIdx.x >> 6] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NQ; ++k) x[k] = (lds[k][0] + lds[k][1]) + (lds[k][2] + lds[k][3]);
}

struct BudgetRows { const int32_t *alive, *ine, *jne; const double *mass, *mass_scaling, *mass_of_bits, *mass_of_fl_bits, *mass_of_fl_bergy_bits, *heat_density; };

// part[k * nblk + block]: quantity k of this block's 256 rows
__global__ void __launch_bounds__(256) budget_berg_kernel(const BudgetRows r, const int *__restrict__ order, const long long n, const int isc, const int iec,
                                                          const int jsc, const int jec, double *__restrict__ part, const int nblk) {
  __shared__ double lds[BUD_NQ_BERG][4];
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  const bool in = q < n;
  const long long k = in ? (order ? (long long)order[q] : q) : 0ll;
  int32_t alive = 0, i = 0, j = 0;
  double mass = 0., ms = 0., bits = 0., flb = 0., flbb = 0., hd = 0.;
  if (in) {
    alive = r.alive[k]; i = r.ine[k]; j = r.jne[k];
    mass = r.mass[k]; ms = r.mass_scaling[k]; bits = r.mass_of_bits[k]; flb = r.mass_of_fl_bits[k]; flbb = r.mass_of_fl_bergy_bits[k]; hd = r.heat_density[k];
  }
  const bool on = in && alive != 0 && i >= isc && i <= iec && j >= jsc && j <= jec;   // FW:6617-6619: the lists of the computational cells
  const double dm = (mass + bits + flb + flbb) * ms;                                   // FW:6627, 6659
  double x[BUD_NQ_BERG];
  x[BUD_NBERGS] = on ? 1. : 0.;                          // count_bergs, IB:5727
  x[BUD_FLOATING_MASS] = on ? dm : 0.;                   // FW:6627
  x[BUD_ICEBERGS_MASS] = on ? mass * ms : 0.;            // FW:6621
  x[BUD_BERGY_MASS] = on ? (bits + flbb) * ms : 0.;      // FW:6623
  x[BUD_FL_BITS_MASS] = on ? flb * ms : 0.;              // FW:6625
  x[BUD_FLOATING_HEAT] = on ? dm * hd : 0.;              // FW:6661
  budget_block_sum<BUD_NQ_BERG>(x, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int f = 0; f < BUD_NQ_BERG; ++f) part[(size_t)f * nblk + blockIdx.x] = x[f];
  }
}

// sum(grd%stored_ice(isc:iec,jsc:jec,:)) (IB:5703, 8120) and sum(grd%stored_heat(isc:iec,jsc:jec)) (IB:5706): a lane per
// computational cell (the order of Fortran's sum intrinsic is the compiler's; here: classes first, then the cell tree)
__global__ void __launch_bounds__(256) budget_cell_kernel(const double *__restrict__ stored_ice, const double *__restrict__ stored_heat, const size_t ncell, const int ci0,
                                                          const int cj0, const int nic, const int njc, const int ni, double *__restrict__ part, const int nblk) {
  __shared__ double lds[BUD_NQ_CELL][4];
  const int t = blockIdx.x * 256 + threadIdx.x;
  double x[BUD_NQ_CELL] = {0., 0.};
  if (t < nic * njc) {
    const size_t c = (size_t)(ci0 + t % nic) + (size_t)(cj0 + t / nic) * (size_t)ni;
    double v[KID_NCLASSES];
#pragma unroll
    for (int k = 0; k < KID_NCLASSES; ++k) v[k] = stored_ice[(size_t)k * ncell + c];
    double s = v[0];
#pragma unroll
    for (int k = 1; k < KID_NCLASSES; ++k) s = s + v[k];
    x[0] = s;
    x[1] = stored_heat[c];
  }
  budget_block_sum<BUD_NQ_CELL>(x, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int f = 0; f < BUD_NQ_CELL; ++f) part[(size_t)f * nblk + blockIdx.x] = x[f];
  }
}

// one block: the block partials in a fixed order, and the step scalars the handle keeps, into the BUD_NRES doubles the host reads
__global__ void __launch_bounds__(256) budget_finish_kernel(const double *__restrict__ part_b, const int nblk_b, const double *__restrict__ part_c, const int nblk_c,
                                                            const double *__restrict__ totals, double *__restrict__ res) {
  __shared__ double lds[BUD_NQ][4];
  double x[BUD_NQ];
#pragma unroll
  for (int f = 0; f < BUD_NQ_BERG; ++f) {
    double v = 0.;
    for (int q = threadIdx.x; q < nblk_b; q += 256) v = v + part_b[(size_t)f * nblk_b + q];
    x[f] = v;
  }
#pragma unroll
  for (int f = 0; f < BUD_NQ_CELL; ++f) {
    double v = 0.;
    for (int q = threadIdx.x; q < nblk_c; q += 256) v = v + part_c[(size_t)f * nblk_c + q];
    x[BUD_NQ_BERG + f] = v;
  }
  budget_block_sum<BUD_NQ>(x, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int f = 0; f < BUD_NQ; ++f) res[f] = x[f];
    res[BUD_NET_HEAT_TO_OCEAN] = totals[KID_S_NET_HEAT_TO_OCEAN];
    res[BUD_NBERGS_MELTED] = totals[KID_S_NBERGS_MELTED];
    res[BUD_NBERGS_CALVED_FL] = totals[KID_S_NBERGS_CALVED_FL];
    res[BUD_NSPEEDING_TICKETS] = totals[KID_S_NSPEEDING_TICKETS];
  }
}

// reproducible mode: rows in static order, key 0 for the rows that count and 1 for the others (one stable radix pass follows)
__global__ void __launch_bounds__(256) budget_live_key_kernel(const int32_t *__restrict__ alive, const int32_t *__restrict__ ine, const int32_t *__restrict__ jne,
                                                              const int *__restrict__ srows, const int isc, const int iec, const int jsc, const int jec,
                                                              unsigned *__restrict__ keys, int *__restrict__ rows, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const int k = srows[q];
  const int i = ine[k], j = jne[k];
  keys[q] = (alive[k] != 0 && i >= isc && i <= iec && j >= jsc && j <= jec) ? 0u : 1u;
  rows[q] = k;
}

// icebergs_incr_mass, IB:6066-6068: the caller's plane covers the computational domain, grd%spread_mass the data domain
__global__ void __launch_bounds__(256) budget_incr_mass_kernel(double *__restrict__ mass, const double *__restrict__ spread_mass, const int ci0, const int cj0,
                                                               const int nic, const int njc, const int ni) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nic * njc) return;
  mass[t] = mass[t] + spread_mass[(size_t)(ci0 + t % nic) + (size_t)(cj0 + t / nic) * (size_t)ni];
}

}  // namespace

// device block of the sweep, sized once by the handle's capacity and grid: the berg partials, the cell partials, the results
static int budget_ensure(kid_handle *h) {
  if (h->d_budget) return KID_OK;
  const size_t nb_b = ((size_t)h->capacity + 255) / 256;
  const size_t nb_c = ((size_t)(h->gd.iec - h->gd.isc + 1) * (size_t)(h->gd.jec - h->gd.jsc + 1) + 255) / 256;
  KID_HIP(h, h->mem.dev(h->d_budget, (size_t)BUD_NQ_BERG * nb_b + (size_t)BUD_NQ_CELL * nb_c + BUD_NRES));
  return KID_OK;
}

static int budget_sweep(kid_handle *h, double res[BUD_NRES]) {
  { const int rc_e = rows_enter(h, ROWS_READ); if (rc_e) return rc_e; }
  { const int rc = budget_ensure(h); if (rc) return rc; }
  const kid_grid_desc &d = h->gd;
  const kid_params &p = h->params;
  const long long n = h->n;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1;
  const size_t nb_cap = ((size_t)h->capacity + 255) / 256;
  const int nblk_b = (int)((n + 255) / 256), nblk_c = h->d_calv_state ? (nic * njc + 255) / 256 : 0;
  double *part_b = h->d_budget, *part_c = part_b + (size_t)BUD_NQ_BERG * nb_cap;
  double *d_res = part_c + (size_t)BUD_NQ_CELL * (size_t)((nic * njc + 255) / 256);
  const dim3 block(256);
  const int *order = nullptr;
  if (n > 0 && h->repro && !(p.mts || p.interactive_icebergs_on || p.footloose)) {
    { const int rc = repro_static_order(h); if (rc) return rc; }
    hipLaunchKernelGGL(budget_live_key_kernel, dim3((unsigned)nblk_b), block, 0, h->stream, (const int32_t *)h->bp.i[KID_BI_ALIVE], (const int32_t *)h->bp.i[KID_BI_INE],
                       (const int32_t *)h->bp.i[KID_BI_JNE], (const int *)h->rp.srows, d.isc, d.iec, d.jsc, d.jec, h->rp.k32[0], h->rp.rows[0], n);
    size_t bytes = h->rp.tmp.bytes;
    KID_HIP(h, rocprim::radix_sort_pairs(h->rp.tmp.p, bytes, h->rp.k32[0], h->rp.k32[1], h->rp.rows[0], h->rp.rows[1], (size_t)n, 0, 1, h->stream));
    order = h->rp.rows[1];
  }
  if (nblk_b > 0) {
    const BudgetRows r{h->bp.i[KID_BI_ALIVE], h->bp.i[KID_BI_INE], h->bp.i[KID_BI_JNE], h->bp.f[KID_B_MASS], h->bp.f[KID_B_MASS_SCALING], h->bp.f[KID_B_MASS_OF_BITS],
                       h->bp.f[KID_B_MASS_OF_FL_BITS], h->bp.f[KID_B_MASS_OF_FL_BERGY_BITS], h->bp.f[KID_B_HEAT_DENSITY]};
    hipLaunchKernelGGL(budget_berg_kernel, dim3((unsigned)nblk_b), block, 0, h->stream, r, order, n, d.isc, d.iec, d.jsc, d.jec, part_b, nblk_b);
  }
  if (nblk_c > 0)
    hipLaunchKernelGGL(budget_cell_kernel, dim3((unsigned)nblk_c), block, 0, h->stream, (const double *)calv_plane(h, CALV_STORED_ICE), (const double *)calv_plane(h, CALV_STORED_HEAT),
                       h->ncell, d.isc - d.isd, d.jsc - d.jsd, nic, njc, h->ni, part_c, nblk_c);
  hipLaunchKernelGGL(budget_finish_kernel, dim3(1), block, 0, h->stream, (const double *)part_b, nblk_b, (const double *)part_c, nblk_c, (const double *)h->d_totals, d_res);
  KID_HIP(h, hipGetLastError());
  KID_HIP(h, hipMemcpyAsync(res, d_res, BUD_NRES * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // the one read: 96 bytes
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

extern "C" int kid_budget(kid_handle *h, kid_budget_out *out) {
  if (!h || !out) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_budget"); if (rc_h) return rc_h; }
  double res[BUD_NRES];
  const int rc = budget_sweep(h, res);
  if (rc) return rc;
  out->nbergs = (int64_t)res[BUD_NBERGS];
  out->nbergs_melted = (int64_t)res[BUD_NBERGS_MELTED];
  out->nbergs_calved_fl = (int64_t)res[BUD_NBERGS_CALVED_FL];
  out->nspeeding_tickets = (int64_t)res[BUD_NSPEEDING_TICKETS];
  out->floating_mass = res[BUD_FLOATING_MASS];
  out->icebergs_mass = res[BUD_ICEBERGS_MASS];
  out->bergy_mass = res[BUD_BERGY_MASS];
  out->fl_bits_mass = res[BUD_FL_BITS_MASS];
  out->floating_heat = res[BUD_FLOATING_HEAT];
  out->stored = res[BUD_STORED];
  out->stored_heat = res[BUD_STORED_HEAT];
  out->net_heat_to_ocean = res[BUD_NET_HEAT_TO_OCEAN];
  return KID_OK;
}

extern "C" int kid_stock(kid_handle *h, int32_t index, double *value) {
  if (!h || !value) return KID_EINVAL;
  *value = 0.0;   // `case default`, IB:8128-8129
  { const int rc_h = halo_rows_refuse(h, "kid_stock"); if (rc_h) return rc_h; }
  if (index != KID_STOCK_WATER && index != KID_STOCK_HEAT) { h->err = "kid_stock: index is neither KID_STOCK_WATER nor KID_STOCK_HEAT"; return KID_EINVAL; }
  double res[BUD_NRES];
  const int rc = budget_sweep(h, res);
  if (rc) return rc;
  const double berg_mass = res[BUD_FLOATING_MASS];   // sum_mass(bergs), IB:8119, 8124
  const double stored_mass = res[BUD_STORED];        // IB:8120, 8125
  if (index == KID_STOCK_WATER) *value = stored_mass + berg_mass;   // IB:8121
  else *value = -(stored_mass + berg_mass) * h->params.HLF;         // IB:8126
  return KID_OK;
}

extern "C" int kid_incr_mass(kid_handle *h, double *mass, int32_t on_device, int32_t ni, int32_t nj) {
  if (!h || !mass) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_incr_mass"); if (rc_h) return rc_h; }
  const kid_grid_desc &d = h->gd;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1;
  if (ni != nic || nj != njc) { h->err = "kid_incr_mass: the plane must cover the computational domain (isc:iec, jsc:jec)"; return KID_EINVAL; }
  if (!h->params.add_weight_to_ocean) return KID_OK;   // IB:6057
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  const size_t bytes = (size_t)nic * (size_t)njc * sizeof(double);
  double *plane = mass;
  if (!on_device) {
    if (!h->d_budget_plane) KID_HIP(h, h->mem.dev(h->d_budget_plane, bytes / sizeof(double)));
    plane = h->d_budget_plane;
    KID_HIP(h, hipMemcpyAsync(plane, mass, bytes, hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(budget_incr_mass_kernel, dim3((unsigned)((nic * njc + 255) / 256)), dim3(256), 0, h->stream, plane, (const double *)(h->d_out + (size_t)KID_O_SPREAD_MASS * h->ncell),
                     d.isc - d.isd, d.jsc - d.jsd, nic, njc, h->ni);
  KID_HIP(h, hipGetLastError());
  if (!on_device) {
    KID_HIP(h, hipMemcpyAsync(mass, plane, bytes, hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
  }
  return KID_OK;
}
