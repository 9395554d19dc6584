// kid_chksum.inc -- bergs_chksum (FW:6889-6987) with berg_chksum (FW:6990-7068), time_hash / pos_hash (FW:4364-4376) and
// FMS's mpp_chksum on the resident structure of arrays: the line icebergs_save_restart prints (IB:8145) and the reference's
// regression tests record ("chksum=... chksum2=... chksum3=... chksum4=... chksum5=... #=...", tests/collision_tests/README:13-22).
//
// A diagnostic, evaluated on the host from a download of the population, in the reference's traversal order (computational
// cells j-outer / i-inner, `inorder` inside a cell, FW:4318-4359).  The source is followed to the letter, quirks included,
// because the quirks decide the numbers:
//   * the row index i and chksum5 start over in every cell (FW:6919): fld(i,:) keeps the i-th berg of the LAST cell that
//     had an i-th berg, chksum5 is the last cell's sum (0 when that cell is empty: all recorded values are 0);
//   * berg_chksum's transfer(rtmp, i8) has a scalar mold and no size: its result is ONE default integer, the low word of
//     rtmp(1) = lon, and itmp(1:36) are 36 copies of it (FW:7055);
//   * mpp_chksum (FMS, not in the reference tree) = wrap-around 64-bit sum of the IEEE bit patterns, narrowed to a default
//     integer on assignment (FW:6950 with FW:6895: kept as the low 32 bits, which is what the recorded values are).
// What the numbers cannot be is the reference's own: they are sums of bit patterns of a run compiled with another
// compiler; the berg count "#" is the part of the line that is comparable (tests/test_chksum.py).
static inline int32_t chk_low32(uint64_t s) { return (int32_t)(uint32_t)s; }
static inline uint64_t chk_bits(double x) { uint64_t u; std::memcpy(&u, &x, sizeof(u)); return u; }

extern "C" int kid_bergs_chksum(kid_handle *h, int64_t out[6]) {
  if (!h || !out) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_bergs_chksum"); if (rc_h) return rc_h; }
  { const int rc_e = rows_enter(h, ROWS_READ); if (rc_e) return rc_e; }
  const size_t n = (size_t)h->n;
  static const int F[] = {KID_B_LON, KID_B_LAT, KID_B_UVEL, KID_B_VVEL, KID_B_MASS, KID_B_THICKNESS, KID_B_WIDTH, KID_B_LENGTH, KID_B_AXN, KID_B_AYN,
                          KID_B_BXN, KID_B_BYN, KID_B_UVEL_OLD, KID_B_VVEL_OLD, KID_B_LON_OLD, KID_B_LAT_OLD, KID_B_START_DAY, KID_B_START_LON,
                          KID_B_START_LAT, KID_B_START_MASS, KID_B_HALO_BERG, KID_B_STATIC_BERG};
  enum { NF = sizeof(F) / sizeof(F[0]) };
  std::vector<std::vector<double>> f(NF, std::vector<double>(n));
  std::vector<int32_t> ine(n), jne(n), alive(n), syear(n);
  std::vector<int64_t> id(n);
  for (int q = 0; q < NF; ++q) if (n) KID_HIP(h, hipMemcpyAsync(f[q].data(), h->bp.f[F[q]], n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (n) {
    KID_HIP(h, hipMemcpyAsync(ine.data(), h->bp.i[KID_BI_INE], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(jne.data(), h->bp.i[KID_BI_JNE], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(alive.data(), h->bp.i[KID_BI_ALIVE], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(syear.data(), h->bp.i[KID_BI_START_YEAR], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(id.data(), h->bp.id, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  enum { LON, LAT, UVEL, VVEL, MASS, THICK, WIDTH, LENGTH, AXN, AYN, BXN, BYN, UOLD, VOLD, LONOLD, LATOLD, SDAY, SLON, SLAT, SMASS, HALO, STATIC };
  const kid_grid_desc &d = h->gd;
  // the bergs of the computational domain in traversal order
  std::vector<int64_t> rows;
  for (size_t k = 0; k < n; ++k)
    if (alive[k] && ine[k] >= d.isc && ine[k] <= d.iec && jne[k] >= d.jsc && jne[k] <= d.jec) rows.push_back((int64_t)k);
  std::sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) {
    if (jne[a] != jne[b]) return jne[a] < jne[b];
    if (ine[a] != ine[b]) return ine[a] < ine[b];
    if (syear[a] != syear[b]) return syear[a] < syear[b];
    if (f[SDAY][a] != f[SDAY][b]) return f[SDAY][a] < f[SDAY][b];
    if (f[SMASS][a] != f[SMASS][b]) return f[SMASS][a] < f[SMASS][b];
    if (f[SLON][a] != f[SLON][b]) return f[SLON][a] < f[SLON][b];
    if (f[SLAT][a] != f[SLAT][b]) return f[SLAT][a] < f[SLAT][b];
    return a < b;
  });
  const size_t nb = std::max<size_t>(rows.size(), 1);   // nbergs = max(count_bergs, 1), FW:6906-6908
  std::vector<double> fld(nb * 19, 0.), fld2(nb * 19, 0.), tmp(h->ncell, 0.);
  std::vector<int32_t> icnt(h->ncell, 0);
  auto berg_chksum = [&](int64_t k) -> int32_t {   // FW:6990-7068
    uint32_t itmp[43];
    const uint32_t w = (uint32_t)chk_bits(f[LON][k]);                  // transfer(rtmp, i8): the low word of rtmp(1)
    for (int q = 0; q < 36; ++q) itmp[q] = w;
    itmp[36] = (uint32_t)(int32_t)f[HALO][k]; itmp[37] = (uint32_t)(int32_t)f[STATIC][k]; itmp[38] = (uint32_t)syear[k];
    itmp[39] = (uint32_t)ine[k]; itmp[40] = (uint32_t)jne[k];
    itmp[41] = (uint32_t)(int32_t)(id[k] >> 32); itmp[42] = (uint32_t)(int32_t)(id[k] & 0xFFFFFFFFll);   // split_id FW:7285-7296
    uint32_t c1 = 0, c2 = 0, c3 = 0;
    for (uint32_t q = 1; q <= 43; ++q) { c1 += itmp[q - 1]; c2 += itmp[q - 1] * q; c3 += itmp[q - 1] * q * q; }
    return (int32_t)(c1 + c2 + c3);
  };
  uint32_t ichk5 = 0;
  size_t r = 0;
  for (int gj = d.jsc; gj <= d.jec; ++gj)
    for (int gi = d.isc; gi <= d.iec; ++gi) {
      size_t i = 0; ichk5 = 0;
      for (; r < rows.size() && jne[rows[r]] == gj && ine[rows[r]] == gi; ++r) {
        const int64_t k = rows[r];
        const int32_t iberg = berg_chksum(k);
        const double time_hash = f[SDAY][k] + 366. * (double)syear[k], pos_hash = f[SLON][k] + 360. * (f[SLAT][k] + 90.);
        double *row = &fld[i * 19];
        const int src[16] = {LON, LAT, UVEL, VVEL, MASS, THICK, WIDTH, LENGTH, AXN, AYN, BXN, BYN, UOLD, VOLD, LONOLD, LATOLD};
        for (int q = 0; q < 16; ++q) row[q] = f[src[q]][k];
        row[16] = time_hash; row[17] = pos_hash; row[18] = (double)iberg;
        const size_t c = (size_t)(gi - d.isd) + (size_t)(gj - d.jsd) * (size_t)h->ni;
        icnt[c] += 1;
        for (int q = 0; q < 19; ++q) fld2[i * 19 + q] = row[q] * (double)icnt[c];
        tmp[c] = tmp[c] + time_hash * pos_hash + log(f[MASS][k]);
        ichk5 += (uint32_t)iberg;
        ++i;
      }
    }
  uint64_t s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (size_t q = 0; q < fld.size(); ++q) { s1 += chk_bits(fld[q]); s2 += chk_bits(fld2[q]); }
  for (int gj = d.jsd; gj <= d.jed; ++gj)
    for (int gi = d.isd; gi <= d.ied; ++gi) {
      const uint64_t u = chk_bits(tmp[(size_t)(gi - d.isd) + (size_t)(gj - d.jsd) * (size_t)h->ni]);
      s3 += u;
      if (gi >= d.isc && gi <= d.iec && gj >= d.jsc && gj <= d.jec) s4 += u;
    }
  out[0] = chk_low32(s1); out[1] = chk_low32(s2); out[2] = chk_low32(s3); out[3] = chk_low32(s4); out[4] = (int32_t)ichk5;
  out[5] = (int64_t)rows.size();
  return KID_OK;
}
