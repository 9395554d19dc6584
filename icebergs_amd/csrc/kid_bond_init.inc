// kid_bond_init.inc -- initialize_iceberg_bonds (IB:356-441) and count_bonds (FW:5172-5285) on the resident population.
// Included by kid_hip.hip after kid_mts_host.inc (it uses the traversal order and the bond tables of the MTS path).
//
// The reference tests every berg against every other berg of the data domain and puts each new bond at the head of the
// berg's list (form_a_bond FW:4866-4877): a berg's new partners end up in reverse traversal order, in front of the bonds
// it had.  Here one lane per berg walks a window of cells through cell_start[] / order[] -- cells j outer, i inner, the
// sorted list inside a cell, i.e. ascending rank -- so its candidates arrive in traversal order and "insert at the head"
// is a shift through six registers.  Two passes: bond_init_kernel<false> counts (nothing is written when some berg would
// hold more than max_bonds), bond_init_kernel<true> moves the old slots back and writes the new ones, slot-major; a lane
// writes only its own slots, so there are no atomics on the tables.  bond_slots_kernel then fills bother_slot.
//
// The window.  Two bergs that bond are closer than D = the largest threshold of the call (length, or 2.5 x the largest
// radius), measured with the pair metric of convert_from_grid_to_meters (IB:444-459) at the mean latitude.  If their cells
// are m columns apart, the m - 1 columns between them are spanned whole, so (m - 1) * ext_x < D where ext_x is a lower
// bound of the width in metres that the pair metric gives any cell of the data domain; the same for rows.  The half-width
// is ceil(D / ext) + 1 cells (the + 1 also absorbs a berg that sits a rounding error outside the cell it is filed under),
// clamped to the data domain.  ext comes from the smallest positive dx / dy of the static grid and from the corner
// coordinates (bond_extents): on a lat-lon grid the narrowest column at the latitude closest to a pole, which bounds the
// metric of every pair because cos falls towards the poles.  A grid whose corner longitudes depend on j (or latitudes on
// i), or one that was never given a static grid, gets the whole domain as its window: slow, never wrong.

namespace {

struct BondInitArgs { int from_radii; double length, rdenom; int wi, wj; };
enum { BI_WORST = 0, BI_NFORMED = 1, BI_NBONDS = 2, BI_UNMATCHED = 3, BI_RMAX = 4, BI_WORDS = 5 };

// the pair test IB:413-431.  Correctly rounded square roots and no contraction whatever the build's flags say: a pair must
// not change sides because of an approximate instruction (this is not a flop-bound loop).
__device__ __forceinline__ double bond_radius(double length, double width, double rdenom) { return __dsqrt_rn(length * width * rdenom); }
__device__ __forceinline__ bool bond_pair_test(const DevGrid &g, const kid_params &p, const BondInitArgs &a, double lon1, double lat1, double radius1,
                                               double lon2, double lat2, double length2, double width2) {
#pragma clang fp contract(off)
  const double dlon = lon1 - lon2, dlat = lat1 - lat2;
  const double lat_ref = 0.5 * (lat1 + lat2);
  double dx_dlon, dy_dlat; grid_to_meters(g, p, lat_ref, dx_dlon, dy_dlat);
  const double r_dist_x = dlon * dx_dlon, r_dist_y = dlat * dy_dlat;
  const double r_dist = __dsqrt_rn((r_dist_x * r_dist_x) + (r_dist_y * r_dist_y));
  if (a.from_radii) return r_dist < 1.25 * (radius1 + bond_radius(length2, width2, a.rdenom));
  return r_dist < a.length;
}

// largest radius of a live berg (the threshold of manually_initialize_bonds_from_radii is 1.25 (radius1 + radius2))
__global__ void __launch_bounds__(256) bond_rmax_kernel(const BergPtrs *__restrict__ bt, const long long n, const double rdenom, unsigned long long *__restrict__ words) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const BergPtrs &b = *bt;
  double r = 0.;
  if (k < n && MI(KID_BI_ALIVE, k) != 0) r = bond_radius(MF(KID_B_LENGTH, k), MF(KID_B_WIDTH, k), rdenom);
  if (!(r > 0.)) r = 0.;
  for (int d = 32; d > 0; d >>= 1) r = dmax(r, __shfl_xor(r, d));
  if ((threadIdx.x & 63) == 0 && r > 0.) atomicMax(words + BI_RMAX, (unsigned long long)__double_as_longlong(r));   // (positive doubles order as their bit patterns)
}

template <bool WRITE>
__global__ void __launch_bounds__(256) bond_init_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt,
                                                        const long long n, const BondInitArgs a, unsigned long long *__restrict__ words) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const BergPtrs &b = *bt; const kid_params &p = *pp; const MtsDev &m = *mt;
  const bool live = k < n && MI(KID_BI_ALIVE, k) != 0;
  int nnew = 0, old = 0;
  int c0 = -1, c1 = -1, c2 = -1, c3 = -1, c4 = -1, c5 = -1;   // the last six candidates, the most recent first
  if (live) {
    old = m.bcount[k];
    const long long idk = b.id[k];
    const double lon1 = MF(KID_B_LON, k), lat1 = MF(KID_B_LAT, k);
    const double radius1 = a.from_radii ? bond_radius(MF(KID_B_LENGTH, k), MF(KID_B_WIDTH, k), a.rdenom) : 0.;
    const int ine = MI(KID_BI_INE, k), jne = MI(KID_BI_JNE, k);
    const int j0 = max(jne - a.wj, g.jsd), j1 = min(jne + a.wj, g.jed), i0 = max(ine - a.wi, g.isd), i1 = min(ine + a.wi, g.ied);
    for (int gj = j0; gj <= j1; ++gj) {
      // the cells (i0 .. i1, gj) are neighbours in the traversal order: one range of order[]
      const int qa = m.cell_start[g.idx(i0, gj)], qb = m.cell_start[g.idx(i1, gj) + 1];
      for (int q = qa; q < qb; ++q) {
        const int o = m.order[q];
        const long long ido = b.id[o];
        if (ido == idk) continue;                                            // IB:400
        bool already = false;                                                // IB:401-411
        for (int s = 0; s < old; ++s) already = already || m.bother_id[MB_S(s, k)] == ido;
        if (already) continue;
        if (!bond_pair_test(g, p, a, lon1, lat1, radius1, MF(KID_B_LON, o), MF(KID_B_LAT, o), MF(KID_B_LENGTH, o), MF(KID_B_WIDTH, o))) continue;
        c5 = c4; c4 = c3; c3 = c2; c2 = c1; c1 = c0; c0 = o;                  // form_a_bond: the new bond goes to the head
        ++nnew;
      }
    }
  }
  if constexpr (!WRITE) {
    if (live && old + nnew > m.mb) atomicMax(words + BI_WORST, ((unsigned long long)(unsigned)(old + nnew) << 32) | (unsigned long long)(unsigned)k);
    unsigned long long s = (unsigned long long)nnew;
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(words + BI_NFORMED, s);
  } else {
    if (!live) return;
    const int total = old + nnew;   // <= mb <= 6: the counting pass has checked every berg
    if (nnew > 0) {
      for (int s = old - 1; s >= 0; --s) {   // the bonds the berg had keep their order, behind the new ones
        const size_t from = MB_S(s, k), to = MB_S(s + nnew, k);
        m.bother_id[to] = m.bother_id[from]; m.bbroken[to] = m.bbroken[from]; m.bother_row[to] = m.bother_row[from];
        for (int f = 0; f < KID_NBOND_F64; ++f) m.bf[f][to] = m.bf[f][from];
      }
#define KID_BI_PUT(s, c)                                                                                                    \
      if ((s) < nnew) {                                                                                                     \
        const size_t at = MB_S(s, k);                                                                                       \
        m.bother_id[at] = b.id[c]; m.bbroken[at] = 0; m.bother_row[at] = (c);                                               \
        for (int f = 0; f < KID_NBOND_F64; ++f) m.bf[f][at] = 0.;                                                           \
      }
      KID_BI_PUT(0, c0) KID_BI_PUT(1, c1) KID_BI_PUT(2, c2) KID_BI_PUT(3, c3) KID_BI_PUT(4, c4) KID_BI_PUT(5, c5)
#undef KID_BI_PUT
      m.bcount[k] = total;
    }
    MI(KID_BI_N_BONDS, k) = total;   // assign_n_bonds FW:4617-4637
  }
}

// count_bonds FW:5172-5285 with check_bond_quality: bond records of the bergs on the computational domain, and those whose
// partner is not resident ("not associated") or holds no bond back to this berg ("not matching")
__global__ void __launch_bounds__(256) bond_count_kernel(const DevGrid g, const BergPtrs *__restrict__ bt, const MtsDev *__restrict__ mt, const long long n,
                                                         unsigned long long *__restrict__ words) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const BergPtrs &b = *bt; const MtsDev &m = *mt;
  unsigned long long nb = 0, bad = 0;
  if (k < n && MI(KID_BI_ALIVE, k) != 0) {
    const int i = MI(KID_BI_INE, k), j = MI(KID_BI_JNE, k);
    if (i >= g.isc && i <= g.iec && j >= g.jsc && j <= g.jec) {
      const int cnt = m.bcount[k];
      const long long idk = b.id[k];
      for (int s = 0; s < cnt; ++s) {
        ++nb;
        const int o = m.bother_row[MB_S(s, k)];
        bool good = false;
        if (o >= 0 && MI(KID_BI_ALIVE, o) != 0) {
          const int co = m.bcount[o];
          for (int t = 0; t < co; ++t) good = good || (m.bother_id[MB_S(t, o)] == idk && m.bother_row[MB_S(t, o)] >= 0);
        }
        if (!good) ++bad;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) { nb += __shfl_xor(nb, d); bad += __shfl_xor(bad, d); }
  if ((threadIdx.x & 63) == 0) {
    if (nb) atomicAdd(words + BI_NBONDS, nb);
    if (bad) atomicAdd(words + BI_UNMATCHED, bad);
  }
}

}  // namespace

// lower bounds of the extent in metres (as the pair metric measures it) of any cell of the data domain, ext[0] zonal and
// ext[1] meridional; 0 = unknown, the window is then the whole domain.  One read of four grid planes per static grid.
static int bond_extents(kid_handle *h, double ext[2]) {
  if (h->bond_ext_valid) { ext[0] = h->bond_ext[0]; ext[1] = h->bond_ext[1]; return KID_OK; }
  ext[0] = ext[1] = 0.;
  if (h->forc.have_static) {
    const size_t nc = h->ncell;
    const int ni = h->ni, nj = h->nj;
    std::vector<double> dx(nc), dy(nc), lon(nc), lat(nc);
    KID_HIP(h, hipMemcpyAsync(dx.data(), h->d_static[KID_G_DX], nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(dy.data(), h->d_static[KID_G_DY], nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(lon.data(), h->d_static[KID_G_LON], nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(lat.data(), h->d_static[KID_G_LAT], nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    // corners: lon a strictly increasing function of i alone, lat of j alone -- otherwise a cell index says nothing
    // about a coordinate difference and the window stays the whole domain
    bool axes = ni >= 2 && nj >= 2;
    double dlon_min = INFINITY, dlat_min = INFINITY, alat_max = 0.;
    for (int j = 0; j < nj && axes; ++j)
      for (int i = 0; i < ni; ++i) {
        const size_t c = (size_t)i + (size_t)j * ni;
        if (lon[c] != lon[i] || lat[c] != lat[(size_t)j * ni]) { axes = false; break; }
        alat_max = std::max(alat_max, fabs(lat[c]));
      }
    for (int i = 1; i < ni && axes; ++i) { const double d = lon[i] - lon[i - 1]; if (!(d > 0.)) axes = false; dlon_min = std::min(dlon_min, d); }
    for (int j = 1; j < nj && axes; ++j) { const double d = lat[(size_t)j * ni] - lat[(size_t)(j - 1) * ni]; if (!(d > 0.)) axes = false; dlat_min = std::min(dlat_min, d); }
    if (axes) {
      double ex = dlon_min, ey = dlat_min;
      if (h->gd.grid_is_latlon) {
        const double m_per_deg = (h->params.pi / 180.) * h->params.Rearth;
        ex = dlon_min * m_per_deg * cos(alat_max * (h->params.pi / 180.));
        ey = dlat_min * m_per_deg;
      }
      for (size_t c = 0; c < nc; ++c) {
        if (dx[c] > 0. && dx[c] < ex) ex = dx[c];
        if (dy[c] > 0. && dy[c] < ey) ey = dy[c];
      }
      if (ex > 0. && ey > 0. && std::isfinite(ex) && std::isfinite(ey)) { ext[0] = ex; ext[1] = ey; }
    }
  }
  h->bond_ext[0] = ext[0]; h->bond_ext[1] = ext[1]; h->bond_ext_valid = true;
  return KID_OK;
}
static int bond_half_width(double thr, double ext, int ncells) {
  if (!(thr > 0.)) return 0;
  if (!(ext > 0.)) return ncells;
  const double w = ceil(thr / ext) + 1.;
  return w < (double)ncells ? (int)w : ncells;
}
static int bond_words(kid_handle *h) {
  if (!h->d_bond_words) KID_HIP(h, h->mem.dev(h->d_bond_words, BI_WORDS));
  KID_HIP(h, hipMemsetAsync(h->d_bond_words, 0, BI_WORDS * sizeof(unsigned long long), h->stream));
  return KID_OK;
}

extern "C" int kid_initialize_bonds(kid_handle *h, int32_t from_radii, double length, int64_t *nformed) {
  if (!h) return KID_EINVAL;
  if (nformed) *nformed = 0;
  if (!h->params.iceberg_bonds_on) { h->err = "kid_initialize_bonds needs iceberg_bonds_on"; return KID_EINVAL; }
  if (h->params.max_bonds > KID_MAX_BONDS || (h->mts_ready && h->mb > KID_MAX_BONDS)) { h->err = "max_bonds out of range"; return KID_EINVAL; }
  { const int rc_e = rows_enter(h, ROWS_CHANGE); if (rc_e) return rc_e; }
  int rc = mts_ensure_default(h);
  if (rc) return rc;
  const long long n = h->n;
  if (n == 0) { h->have_bonds = true; h->visited = false; return KID_OK; }
  // a population uploaded since the tables were last used has no bonds, whatever the tables still hold
  if (!h->have_bonds) KID_HIP(h, hipMemsetAsync(h->mts.bcount, 0, (size_t)n * sizeof(int32_t), h->stream));
  rc = mts_refresh(h);   // the pointer tables the order kernels read
  if (rc) return rc;
  rc = mts_build_order(h);
  if (rc) return rc;
  rc = mts_refresh(h);
  if (rc) return rc;
  rc = bond_words(h);
  if (rc) return rc;
  BondInitArgs a{};
  a.from_radii = from_radii ? 1 : 0; a.length = length;
  a.rdenom = h->params.hexagonal_icebergs ? 1. / (2. * sqrt(3.)) : 1. / 4.;   // IB:374-381
  const BergPtrs *bt = h->d_bp; const MtsDev *mt = h->d_mts; const kid_params *pp = h->d_params;
  unsigned long long words[BI_WORDS] = {};
  double thr = length;
  if (a.from_radii) {
    hipLaunchKernelGGL(bond_rmax_kernel, MTS_GRID(n), bt, n, a.rdenom, h->d_bond_words);
    KID_HIP(h, hipMemcpyAsync(words + BI_RMAX, h->d_bond_words + BI_RMAX, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    double rmax; memcpy(&rmax, words + BI_RMAX, sizeof(double));
    thr = 2.5 * rmax * (1. + 1.e-12);   // >= 1.25 (radius1 + radius2) of every pair
  }
  double ext[2];
  rc = bond_extents(h, ext);
  if (rc) return rc;
  a.wi = bond_half_width(thr, ext[0], h->ni); a.wj = bond_half_width(thr, ext[1], h->nj);
  const DevGrid g = dev_grid(h);
  hipLaunchKernelGGL(bond_init_kernel<false>, MTS_GRID(n), g, pp, bt, mt, n, a, h->d_bond_words);
  KID_HIP(h, hipGetLastError());
  KID_HIP(h, hipMemcpyAsync(words, h->d_bond_words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));   // 16 bytes: the worst berg, the bonds formed
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if (words[BI_WORST] != 0ull) {
    const long long row = (long long)(words[BI_WORST] & 0xffffffffull), cnt = (long long)(words[BI_WORST] >> 32);
    int64_t id = 0;
    KID_HIP(h, hipMemcpy(&id, h->bp.id + row, sizeof(int64_t), hipMemcpyDeviceToHost));
    h->err = "kid_initialize_bonds: a berg would hold " + std::to_string(cnt) + " bonds, more than max_bonds = " + std::to_string(h->mb) + " (berg id " + std::to_string((long long)id) +
             "); no bond was formed";
    return KID_ECAPACITY;
  }
  hipLaunchKernelGGL(bond_init_kernel<true>, MTS_GRID(n), g, pp, bt, mt, n, a, h->d_bond_words);
  hipLaunchKernelGGL(bond_slots_kernel, MTS_GRID(n), bt, mt, n);
  KID_HIP(h, hipGetLastError());
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->have_bonds = true; h->visited = false; h->labels_stale = true;
  if (nformed) *nformed = (int64_t)words[BI_NFORMED];
  return KID_OK;
}

extern "C" int kid_count_bonds(kid_handle *h, int64_t *nbonds, int64_t *unmatched) {
  if (!h) return KID_EINVAL;
  if (nbonds) *nbonds = 0;
  if (unmatched) *unmatched = 0;
  { const int rc_e = rows_enter(h, ROWS_READ); if (rc_e) return rc_e; }
  if (!h->have_bonds || !h->mts_ready || h->n == 0) return KID_OK;
  int rc = mts_refresh(h);
  if (rc) return rc;
  rc = bond_words(h);
  if (rc) return rc;
  const long long n = h->n;
  hipLaunchKernelGGL(bond_count_kernel, MTS_GRID(n), dev_grid(h), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n, h->d_bond_words);
  KID_HIP(h, hipGetLastError());
  unsigned long long words[2] = {0ull, 0ull};
  KID_HIP(h, hipMemcpyAsync(words, h->d_bond_words + BI_NBONDS, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));   // one 16-byte read
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if (nbonds) *nbonds = (int64_t)words[0];
  if (unmatched) *unmatched = (int64_t)words[1];
  return KID_OK;
}
