// kid_repro.inc -- reproducible per-cell sums (kid_set_reproducible_sums, the device side of `parallel_reprod`).
// Included by kid_hip.hip after kid_mts_host.inc (it reuses the key kernels of the MTS traversal order).
//
// The default scatter-add (kid_thermo.hpp) sums each wave's runs in lane order and adds the run sums with fp64 atomics, so
// a plane's last bits depend on which wave arrives first and on how the rows are laid out.  In this mode every per-cell sum
// is a function of the set of bergs only (cdna guide, appendix B, "scatter / gather"):
//   1. the staging instance of berg_kernel (STAGE = true) stores every contribution: stage[slot * cap + row], plus the
//      row's cell (key) and the slots it wrote (mask);
//   2. the rows are put in the reference's traversal order: a static order by the `inorder` keys (start_year, start_day,
//      start_mass, start_lon, start_lat; FW:4318-4359) with the berg id as the last key, rebuilt only when rows change,
//      then one stable radix pass by the cell the row contributed to;
//   3. the fold: one thread per (cell, plane group) adds the staged values of the cell's rows in that order onto what the
//      plane holds -- the oracle's acc = acc + x, a strict left fold; a cell's list is never split;
//   4. net_heat_to_ocean: the per-cell sums of the berg terms, reduced over the cells by a tree of fixed shape.
// The counters among the step scalars are sums of integers and exact whatever the order.
namespace {

// the static order: the berg id as the least significant key (stands in for the oracle's row index)
__global__ void __launch_bounds__(256) repro_key_id_kernel(const int64_t *__restrict__ id, const int *__restrict__ rows, unsigned long long *__restrict__ keys, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q < n) keys[q] = (unsigned long long)id[rows[q]] ^ 0x8000000000000000ull;
}
// cell of every row in canonical order; rows outside the launch's range or without a contribution sort last (key = ncell)
__global__ void __launch_bounds__(256) repro_cell_key_kernel(const int32_t *__restrict__ skey, const int *__restrict__ srows, unsigned *__restrict__ keys,
                                                             int *__restrict__ rows, const long long n, const long long k0, const long long k1, const unsigned dead) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const int r = srows[q];
  const int c = (r >= k0 && r < k1) ? skey[r] : -1;
  keys[q] = c >= 0 ? (unsigned)c : dead;
  rows[q] = r;
}
// cell_start[c] = first position of cell c in the sorted order, for c = 0 .. ncell (cell_start[ncell]: the first row left out)
__global__ void __launch_bounds__(256) repro_cell_start_kernel(const unsigned *__restrict__ keys, int *__restrict__ cs, const long long n, const unsigned ncell) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const unsigned c = keys[q];
  const unsigned lo = (q == 0) ? 0u : keys[q - 1] + 1u;   // cells (keys[q-1], c] start at q
  for (unsigned cc = lo; cc <= c; ++cc) cs[cc] = (int)q;
  if (q == n - 1) for (unsigned cc = c + 1u; cc <= ncell; ++cc) cs[cc] = (int)n;
}

// A group of planes one fold thread owns for its cell.  kind 0: up to four planes staged as values (plane < 0: the berg's
// heat term, summed into cell_heat); kind 1 + v: the nine planes of on-ocean quantity v, formed from the staged factors.
enum { KID_FOLD_MAXG = 16 };
struct FoldGroup { int kind, n, plane[4]; };
struct FoldTab { int ng; FoldGroup g[KID_FOLD_MAXG]; };
// The rows of a cell are walked in batches (KID_FOLD_B rows: their order entries, masks and values are all loaded before the
// first add), so that a thread waits for memory once per batch, not three times per row; the adds stay one after the other.
#define KID_FOLD_B 8
__global__ void __launch_bounds__(256) repro_fold_kernel(const FoldTab ft, const int *__restrict__ order, const int *__restrict__ cs, const double *__restrict__ val,
                                                         const unsigned long long *__restrict__ mask, const long long cap, double *__restrict__ acc,
                                                         const size_t ncell, double *__restrict__ cell_heat) {
  const long long t = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (t >= (long long)ft.ng * (long long)ncell) return;
  const int gi = (int)(t / (long long)ncell);
  const size_t c = (size_t)(t - (long long)gi * (long long)ncell);
  const FoldGroup &G = ft.g[gi];
  const int b = cs[c], e = cs[c + 1];
  const size_t scap = (size_t)cap;
  if (G.kind == 0) {
    double a[4];
    int slot[4];
    unsigned touched = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pl = j < G.n ? G.plane[j] : 0;
      slot[j] = (j < G.n) ? (pl < 0 ? KID_ST_HEAT : stage_slot(pl)) : 63;
      a[j] = (j < G.n && pl >= 0 && b < e) ? acc[(size_t)pl * ncell + c] : 0.;
    }
    for (int i0 = b; i0 < e; i0 += KID_FOLD_B) {
      int r[KID_FOLD_B];
      unsigned long long m[KID_FOLD_B];
      double x[KID_FOLD_B][4];
#pragma unroll
      for (int u = 0; u < KID_FOLD_B; ++u) r[u] = (i0 + u < e) ? order[i0 + u] : -1;
#pragma unroll
      for (int u = 0; u < KID_FOLD_B; ++u) m[u] = (r[u] >= 0) ? mask[r[u]] : 0ull;
#pragma unroll
      for (int u = 0; u < KID_FOLD_B; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[u][j] = ((m[u] >> slot[j]) & 1ull) ? val[(size_t)slot[j] * scap + (size_t)r[u]] : 0.;
#pragma unroll
      for (int u = 0; u < KID_FOLD_B; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((m[u] >> slot[j]) & 1ull) { a[j] = a[j] + x[u][j]; touched |= 1u << j; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= G.n) continue;
      if (G.plane[j] < 0) cell_heat[c] = a[j];
      else if (touched & (1u << j)) acc[(size_t)G.plane[j] * ncell + c] = a[j];
    }
    return;
  }
  if (b == e) return;
  const int v = G.kind - 1;
  const int base = on_ocean_family(v).first;
  double a[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) a[s] = acc[(size_t)(base + s) * ncell + c];
  bool touched = false;
  constexpr int B = KID_FOLD_B / 2;   // eleven values per row
  for (int i0 = b; i0 < e; i0 += B) {
    int r[B];
    bool on[B];
    double x[B], f[B], w[B][9];
#pragma unroll
    for (int u = 0; u < B; ++u) r[u] = (i0 + u < e) ? order[i0 + u] : -1;
#pragma unroll
    for (int u = 0; u < B; ++u) on[u] = (r[u] >= 0) && ((mask[r[u]] >> (KID_ST_VAR + v)) & 1ull);
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const size_t rr = on[u] ? (size_t)r[u] : 0;
      x[u] = on[u] ? val[(size_t)(KID_ST_VAR + v) * scap + rr] : 0.;
      f[u] = on[u] ? val[(size_t)KID_ST_IFU * scap + rr] : 0.;
#pragma unroll
      for (int s = 0; s < 9; ++s) w[u][s] = on[u] ? val[(size_t)(KID_ST_W + s) * scap + rr] : 0.;
    }
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (!on[u]) continue;
#pragma unroll
      for (int s = 0; s < 9; ++s) a[s] = a[s] + on_ocean_term(w[u][s], x[u], f[u]);
      touched = true;
    }
  }
  if (touched) {
#pragma unroll
    for (int s = 0; s < 9; ++s) acc[(size_t)(base + s) * ncell + c] = a[s];
  }
}
// net_heat_to_ocean over the cells: a pairwise tree inside each block of 256 cells, then one block adds the block sums
// (thread t: blocks t, t + 256, ... in turn) and reduces its 256 threads the same way.  The shape depends on ncell only.
__device__ __forceinline__ double repro_block_sum(double v, double *lds) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) v = v + __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
__global__ void __launch_bounds__(256) repro_heat_part_kernel(const double *__restrict__ cell_heat, const long long ncell, double *__restrict__ part) {
  __shared__ double lds[4];
  const long long t = (long long)blockIdx.x * 256ll + threadIdx.x;
  const double s = repro_block_sum(t < ncell ? cell_heat[t] : 0., lds);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void __launch_bounds__(256) repro_heat_finish_kernel(const double *__restrict__ part, const int nparts, double *__restrict__ scal) {
  __shared__ double lds[4];
  double v = 0.;
  for (int q = threadIdx.x; q < nparts; q += 256) v = v + part[q];
  const double s = repro_block_sum(v, lds);
  if (threadIdx.x == 0) scal[KID_S_NET_HEAT_TO_OCEAN] = scal[KID_S_NET_HEAT_TO_OCEAN] + s;
}

}  // namespace

// switching the mode off returns all of its memory: the mode has an owner of its own
static int repro_free(kid_handle *h) {
  h->rp = kid_handle::Repro{};
  KID_HIP(h, (hipError_t)h->rp_mem.free_all());
  return KID_OK;
}
// the buffers of the mode, sized by the handle's capacity and grid (allocated once, when the switch is turned on)
static int repro_alloc(kid_handle *h) {
  if (h->rp.stage) return KID_OK;
  const size_t cap = (size_t)h->capacity, nc = h->ncell;
  const size_t nparts = (nc + 255) / 256;
  KID_HIP(h, h->rp_mem.dev(h->rp.stage, (size_t)KID_ST_N * cap));
  KID_HIP(h, h->rp_mem.dev(h->rp.key, cap));
  KID_HIP(h, h->rp_mem.dev(h->rp.mask, cap));
  KID_HIP(h, h->rp_mem.dev(h->rp.srows, cap));
  for (int q = 0; q < 2; ++q) { KID_HIP(h, h->rp_mem.dev(h->rp.k64[q], cap)); KID_HIP(h, h->rp_mem.dev(h->rp.rows[q], cap)); KID_HIP(h, h->rp_mem.dev(h->rp.k32[q], cap)); }
  KID_HIP(h, h->rp_mem.dev(h->rp.cs, nc + 1));
  KID_HIP(h, h->rp_mem.dev(h->rp.cell_heat, nc));
  KID_HIP(h, h->rp_mem.dev(h->rp.part, nparts));
  size_t b64 = 0, b32 = 0;
  KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b64, h->rp.k64[0], h->rp.k64[1], h->rp.rows[0], h->rp.rows[1], cap, 0, 64, h->stream));
  KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b32, h->rp.k32[0], h->rp.k32[1], h->rp.rows[0], h->rp.rows[1], cap, 0, 32, h->stream));
  KID_HIP(h, h->rp_mem.reserve(h->rp.tmp, std::max(b64, b32)));
  h->rp.srows_n = -1;
  return KID_OK;
}
// The switches the mode does not cover yet; checked when it is turned on and again at every launch (kid_set_params may turn
// them on later).  The message names the switch.
static int repro_refuse(kid_handle *h) {
  if (!h->repro) return KID_OK;
  const kid_params &p = h->params;
  const char *sw = p.mts ? "mts" : (p.interactive_icebergs_on ? "interactive_icebergs_on" : (p.footloose ? "footloose" : nullptr));
  if (!sw) return KID_OK;
  h->err = std::string("reproducible sums (kid_set_reproducible_sums) are not implemented together with ") + sw + "; turn one of them off";
  return KID_EUNSUPPORTED;
}
// rows [0, n) in canonical order: five stable passes by the `inorder` keys on top of one by the id (LSD: least significant first)
static int repro_static_order(kid_handle *h) {
  const long long n = h->n;
  if (h->rp.srows_n == n) return KID_OK;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  int cur = 0;
  hipLaunchKernelGGL(mts_iota_kernel, grid, block, 0, h->stream, h->rp.rows[cur], n);
  const int f64_keys[4] = {KID_B_START_LAT, KID_B_START_LON, KID_B_START_MASS, KID_B_START_DAY};
  for (int pass = 0; pass < 6; ++pass) {
    if (pass == 0) hipLaunchKernelGGL(repro_key_id_kernel, grid, block, 0, h->stream, (const int64_t *)h->bp.id, (const int *)h->rp.rows[cur], h->rp.k64[0], n);
    else if (pass < 5) hipLaunchKernelGGL(mts_key_f64_kernel, grid, block, 0, h->stream, (const double *)h->bp.f[f64_keys[pass - 1]], (const int *)h->rp.rows[cur], h->rp.k64[0], n);
    else hipLaunchKernelGGL(mts_key_i32_kernel, grid, block, 0, h->stream, (const int32_t *)h->bp.i[KID_BI_START_YEAR], (const int *)h->rp.rows[cur], h->rp.k64[0], n);
    size_t bytes = h->rp.tmp.bytes;
    KID_HIP(h, rocprim::radix_sort_pairs(h->rp.tmp.p, bytes, h->rp.k64[0], h->rp.k64[1], h->rp.rows[cur], h->rp.rows[cur ^ 1], (size_t)n, 0, 64, h->stream));
    cur ^= 1;
  }
  KID_HIP(h, hipMemcpyAsync(h->rp.srows, h->rp.rows[cur], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  KID_HIP(h, hipGetLastError());
  h->rp.srows_n = n;
  return KID_OK;
}
// After a staging launch over rows [k0, k0 + klen): order, fold, heat.  thermo / spread: which kinds of planes it may have staged.
static int repro_fold(kid_handle *h, bool thermo, bool spread, long long k0, long long klen) {
  const long long n = h->n;
  if (n == 0) return KID_OK;
  { const int rc = repro_static_order(h); if (rc) return rc; }
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const unsigned ncell = (unsigned)h->ncell;
  hipLaunchKernelGGL(repro_cell_key_kernel, grid, block, 0, h->stream, (const int32_t *)h->rp.key, (const int *)h->rp.srows, h->rp.k32[0], h->rp.rows[0], n, k0, k0 + klen, ncell);
  const unsigned bits = 32u - (unsigned)__builtin_clz(ncell);   // keys 0 .. ncell
  size_t bytes = h->rp.tmp.bytes;
  KID_HIP(h, rocprim::radix_sort_pairs(h->rp.tmp.p, bytes, h->rp.k32[0], h->rp.k32[1], h->rp.rows[0], h->rp.rows[1], (size_t)n, 0, bits, h->stream));
  hipLaunchKernelGGL(repro_cell_start_kernel, grid, block, 0, h->stream, (const unsigned *)h->rp.k32[1], h->rp.cs, n, ncell);
  // every plane the launch may have written (the row masks say which it did write)
  FoldTab ft{};
  auto add_value = [&ft](int plane) {
    if (ft.ng == 0 || ft.g[ft.ng - 1].kind != 0 || ft.g[ft.ng - 1].n == 4) { ft.g[ft.ng].kind = 0; ft.g[ft.ng].n = 0; ++ft.ng; }
    FoldGroup &G = ft.g[ft.ng - 1];
    G.plane[G.n++] = plane;
  };
  if (thermo) add_value(-1);
  for (int pl = 0; pl < KID_NACC; ++pl)   // (the on-ocean families are folded as groups of nine, below)
    if (!ON_OCEAN_ALL.contains(pl) && plane_range_live(pl, 1, h->params.pass_fields_to_ocean_model, h->params.diag_mask)) add_value(pl);
  if (spread) {
    ft.g[ft.ng].kind = 1; ft.g[ft.ng].n = ON_OCEAN_SLOTS; ++ft.ng;
    if (h->flags.footprint) for (int v = 1; v < 4; ++v) { ft.g[ft.ng].kind = 1 + v; ft.g[ft.ng].n = ON_OCEAN_SLOTS; ++ft.ng; }
  }
  const long long nt = (long long)ft.ng * (long long)h->ncell;
  hipLaunchKernelGGL(repro_fold_kernel, dim3((unsigned)((nt + 255) / 256)), block, 0, h->stream, ft, (const int *)h->rp.rows[1], (const int *)h->rp.cs,
                     (const double *)h->rp.stage, (const unsigned long long *)h->rp.mask, (long long)h->capacity, h->d_acc, h->ncell, h->rp.cell_heat);
  if (thermo) {
    const int nparts = (int)((h->ncell + 255) / 256);
    hipLaunchKernelGGL(repro_heat_part_kernel, dim3((unsigned)nparts), block, 0, h->stream, (const double *)h->rp.cell_heat, (long long)h->ncell, h->rp.part);
    hipLaunchKernelGGL(repro_heat_finish_kernel, dim3(1), block, 0, h->stream, (const double *)h->rp.part, nparts, h->d_acc - KID_NSCALAR);
  }
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}

extern "C" int kid_set_reproducible_sums(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  if (!on) {
    if (!h->repro) return KID_OK;
    h->repro = false;
    KID_HIP(h, hipStreamSynchronize(h->stream));
    return repro_free(h);
  }
  h->repro = true;
  int rc = repro_refuse(h);
  if (!rc) rc = lanes_drain(h);   // the slow-lane schedule is not used in this mode
  if (!rc) rc = rebin_flush(h);   // nor is the re-binning instance of the hot build
  if (!rc) rc = repro_alloc(h);
  if (rc) { (void)repro_free(h); h->repro = false; }
  return rc;
}
