// kid_chksum_device.inc -- the reference's checksums on the resident state: kid_bergs_chksum_device (bergs_chksum, FW:6889-6987)
// and kid_checksum_gridded (checksum_gridded with grd_chksum2 / grd_chksum3, FW:6685-6886).  Included by kid_hip.hip after
// kid_chksum.inc, whose kid_bergs_chksum stays the checker: a download and a host sort, held against the oracle.
//
// Gridded fields.  One sweep serves all 59 of them: chkd_sweep_kernel, grid (blocks, fields), a block takes 2048 consecutive
// elements of a field's computational domain (k outer, j, i inner), a thread eight of them 256 apart, added in turn; the lanes of
// a wave by a butterfly, the four waves through LDS as (w0 + w1) + (w2 + w3); chkd_finish_kernel, one block per field: thread
// t takes the block partials t, t + 256, ... in turn, then the same block tree.  No atomics: the shape depends on the grid
// only, so two calls on the same state give the same bits.  The mean is formed on the host between the two passes (the second
// sums (x - mean)**2, FW:6866-6872), so the mean that is printed is the one the deviation is taken about.
//
// Bergs.  The order of the reference's traversal (computational cells j outer / i inner, `inorder` inside a cell, the row as
// the last tie: kid_chksum.inc's comparator) is built by stable LSD radix passes as in repro_static_order, from an identity
// permutation, with two differences: no id key, and keys that take -0.0 for +0.0 as `<` does.  From the order:
//   * cs[c], the first position of computational cell c, hence a berg's rank r in its cell and the per-cell counts;
//   * fld(i,:) keeps the i-th berg of the LAST cell that had one (kid_chksum.inc): a berg of rank r in cell c is still there at
//     the end iff r >= max(count(c')) over the cells after c -- an exclusive suffix maximum, taken as a prefix scan of the
//     reversed counts.  Such a berg adds the bit patterns of its 19 values to chksum and of the values times (r + 1) to
//     chksum2: wrap-around integer sums, so integer atomics in any order;
//   * chksum5 = the 32-bit wrap sum of berg_chksum over the last cell (iec, jec);
//   * chksum3 = chksum4 need log(mass).  The device's log and the host's differ in the last bit now and then and the integers
//     must not depend on who computed them, so the logarithm is the host's std::log, as in kid_bergs_chksum: the device hands
//     over mass and time_hash * pos_hash of the bergs in traversal order (16 bytes a berg) and cs; the host folds
//     t = (t + th * ph) + log(m) per cell (kid_chksum.inc:86).
// -ffp-contract=off (Makefile) keeps time_hash, pos_hash and their product the two roundings each that the host makes.
// Every block is temporary, from the handle's owner, sized by h->n or by the grid, and gone on return.
namespace {

enum { CHKD_EPB = 2048, CHKD_EPT = CHKD_EPB / 256 };
struct ChkField { const double *p; int nk, present; };   // plane k of the field at p + k * ncell; p == nullptr: planes of zeros
struct ChkTab { ChkField f[KID_NCHK]; };
struct ChkMeans { double m[KID_NCHK]; };
struct ChkDom { int ci0, cj0, nic, njc, ni, isc, jsc; long long ncell; };   // ci0 = isc - isd, cj0 = jsc - jsd
enum { CHKD_SUM = 0, CHKD_SUMSQ, CHKD_MIN, CHKD_MAX, CHKD_SD, CHKD_ND, CHKD_NPD = 4, CHKD_NU = 2 };   // doubles / words of a field's result; a partial of pass 1 holds CHKD_NPD doubles

__device__ __forceinline__ unsigned long long chkd_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double chkd_wave_sum(double v) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) v = v + __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ double chkd_wave_min(double v) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) v = fmin(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ double chkd_wave_max(double v) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) v = fmax(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ unsigned long long chkd_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) v += (unsigned long long)__shfl_xor((long long)v, d);
  return v;
}
// what one block made of its elements (or partials): every thread of the block calls it, thread 0 holds the result
struct ChkdAcc { double s, s2, mn, mx; unsigned long long c1, c2; };
__device__ __forceinline__ void chkd_block_reduce(ChkdAcc &a, double (*ld)[4], unsigned long long (*lu)[4]) {
  a.s = chkd_wave_sum(a.s); a.s2 = chkd_wave_sum(a.s2); a.mn = chkd_wave_min(a.mn); a.mx = chkd_wave_max(a.mx);
  a.c1 = chkd_wave_sum(a.c1); a.c2 = chkd_wave_sum(a.c2);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    ld[0][w] = a.s; ld[1][w] = a.s2; ld[2][w] = a.mn; ld[3][w] = a.mx; lu[0][w] = a.c1; lu[1][w] = a.c2;
  }
  __syncthreads();
  a.s = (ld[0][0] + ld[0][1]) + (ld[0][2] + ld[0][3]);
  a.s2 = (ld[1][0] + ld[1][1]) + (ld[1][2] + ld[1][3]);
  a.mn = fmin(fmin(ld[2][0], ld[2][1]), fmin(ld[2][2], ld[2][3]));
  a.mx = fmax(fmax(ld[3][0], ld[3][1]), fmax(ld[3][2], ld[3][3]));
  a.c1 = (lu[0][0] + lu[0][1]) + (lu[0][2] + lu[0][3]);
  a.c2 = (lu[1][0] + lu[1][1]) + (lu[1][2] + lu[1][3]);
}
__device__ __forceinline__ long long chkd_count(const ChkField &F, const ChkDom &g) { return F.present ? (long long)g.nic * g.njc * F.nk : 0ll; }

// PASS 1: sum, sum of squares, min, max, the two bit-pattern sums.  PASS 2: the sum of (x - mean)**2 (in `s`).
// pd[(f * nblk + b) * CHKD_NPD + q], pu[(f * nblk + b) * CHKD_NU + q]; a block beyond its field's elements writes nothing
// (the finish kernel reads the field's own blocks only).
template <int PASS>
__global__ void __launch_bounds__(256) chkd_sweep_kernel(const ChkTab tab, const ChkMeans means, const ChkDom g, double *__restrict__ pd, unsigned long long *__restrict__ pu, const int nblk) {
  __shared__ double ld[4][4];
  __shared__ unsigned long long lu[2][4];
  const int f = blockIdx.y;
  const ChkField F = tab.f[f];
  const long long ncomp = (long long)g.nic * g.njc, N = chkd_count(F, g);
  const long long base = (long long)blockIdx.x * CHKD_EPB;
  if (base >= N) return;   // (the whole block)
  const double mean = PASS == 2 ? means.m[f] : 0.;
  ChkdAcc a{0., 0., __builtin_inf(), -__builtin_inf(), 0ull, 0ull};
#pragma unroll
  for (int u = 0; u < CHKD_EPT; ++u) {
    const long long e = base + (long long)u * 256ll + threadIdx.x;
    if (e >= N) continue;
    const int k = (int)(e / ncomp);
    const int cc = (int)(e - (long long)k * ncomp);
    const int dj = cc / g.nic, di = cc - dj * g.nic;
    const double x = F.p ? F.p[(size_t)k * (size_t)g.ncell + (size_t)(g.ci0 + di) + (size_t)(g.cj0 + dj) * (size_t)g.ni] : 0.;
    if (PASS == 1) {
      const double w = (double)((g.isc + di) + 2 * (g.jsc + dj) + 3 * k);   // FW:6856, 6792 (k from 1 there)
      a.s = a.s + x; a.s2 = a.s2 + x * x;
      a.mn = fmin(a.mn, x); a.mx = fmax(a.mx, x);
      a.c1 += chkd_bits(x); a.c2 += chkd_bits(x * w);
    } else {
      const double dx = x - mean;
      a.s = a.s + dx * dx;
    }
  }
  chkd_block_reduce(a, ld, lu);
  if (threadIdx.x == 0) {
    const size_t o = (size_t)f * (size_t)nblk + blockIdx.x;
    if (PASS == 1) {
      pd[o * CHKD_NPD + CHKD_SUM] = a.s; pd[o * CHKD_NPD + CHKD_SUMSQ] = a.s2; pd[o * CHKD_NPD + CHKD_MIN] = a.mn; pd[o * CHKD_NPD + CHKD_MAX] = a.mx;
      pu[o * CHKD_NU + 0] = a.c1; pu[o * CHKD_NU + 1] = a.c2;
    } else pd[o * CHKD_NPD + CHKD_SUM] = a.s;
  }
}
// one block per field: rd[f * CHKD_ND + q], ru[f * CHKD_NU + q]; a field that is not present gives zeros
template <int PASS>
__global__ void __launch_bounds__(256) chkd_finish_kernel(const ChkTab tab, const ChkDom g, const double *__restrict__ pd, const unsigned long long *__restrict__ pu, const int nblk,
                                                          double *__restrict__ rd, unsigned long long *__restrict__ ru) {
  __shared__ double ld[4][4];
  __shared__ unsigned long long lu[2][4];
  const int f = blockIdx.x;
  const long long N = chkd_count(tab.f[f], g);
  const int nb = (int)((N + CHKD_EPB - 1) / CHKD_EPB);
  ChkdAcc a{0., 0., __builtin_inf(), -__builtin_inf(), 0ull, 0ull};
  for (int q = threadIdx.x; q < nb; q += 256) {
    const size_t o = (size_t)f * (size_t)nblk + (size_t)q;
    a.s = a.s + pd[o * CHKD_NPD + CHKD_SUM];
    if (PASS == 1) {
      a.s2 = a.s2 + pd[o * CHKD_NPD + CHKD_SUMSQ];
      a.mn = fmin(a.mn, pd[o * CHKD_NPD + CHKD_MIN]); a.mx = fmax(a.mx, pd[o * CHKD_NPD + CHKD_MAX]);
      a.c1 += pu[o * CHKD_NU + 0]; a.c2 += pu[o * CHKD_NU + 1];
    }
  }
  chkd_block_reduce(a, ld, lu);
  if (threadIdx.x == 0) {
    if (PASS == 1) {
      rd[f * CHKD_ND + CHKD_SUM] = a.s; rd[f * CHKD_ND + CHKD_SUMSQ] = a.s2;
      rd[f * CHKD_ND + CHKD_MIN] = nb ? a.mn : 0.; rd[f * CHKD_ND + CHKD_MAX] = nb ? a.mx : 0.;
      ru[f * CHKD_NU + 0] = a.c1; ru[f * CHKD_NU + 1] = a.c2;
    } else rd[f * CHKD_ND + CHKD_SD] = a.s;
  }
}

// ---- bergs ----
// the key of mts_key_f64_kernel with -0.0 taken for +0.0: the host comparator's `!=` and `<` do not tell them apart
__global__ void __launch_bounds__(256) chkd_key_f64_kernel(const double *__restrict__ fld, const int *__restrict__ rows, unsigned long long *__restrict__ keys, const long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  unsigned long long u = chkd_bits(fld[rows[q]]);
  if (u == 0x8000000000000000ull) u = 0ull;
  keys[q] = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
// position of the row's cell in the traversal (j outer, i inner over the computational domain); `dead` for a row that does
// not count: dead, or live with its cell outside the computational domain
__global__ void __launch_bounds__(256) chkd_key_cell_kernel(const int32_t *__restrict__ alive, const int32_t *__restrict__ ine, const int32_t *__restrict__ jne, const int *__restrict__ rows,
                                                            unsigned *__restrict__ keys, const long long n, const int isc, const int iec, const int jsc, const int jec, const unsigned dead) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const int r = rows[q];
  const int i = ine[r], j = jne[r];
  const bool on = alive[r] != 0 && i >= isc && i <= iec && j >= jsc && j <= jec;
  keys[q] = on ? (unsigned)((j - jsc) * (iec - isc + 1) + (i - isc)) : dead;
}
// counts from the cell starts: reversed for the suffix maximum, and as the plane icnt of the '# of bergs/cell' record
__global__ void __launch_bounds__(256) chkd_counts_kernel(const int *__restrict__ cs, int *__restrict__ rev, double *__restrict__ plane, const ChkDom g) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int ncomp = g.nic * g.njc;
  if (c >= ncomp) return;
  const int cnt = cs[c + 1] - cs[c];
  rev[ncomp - 1 - c] = cnt;
  if (plane) { const int dj = c / g.nic, di = c - dj * g.nic; plane[(size_t)(g.ci0 + di) + (size_t)(g.cj0 + dj) * (size_t)g.ni] = (double)cnt; }
}
struct ChkdRows { const double *f[16]; const double *sday, *slon, *slat, *halo, *stat; const int32_t *syear, *ine, *jne; const int64_t *id; };
// berg_chksum, kid_chksum.inc:59-69 (FW:6990-7068)
__device__ __forceinline__ int32_t chkd_berg_chksum(const ChkdRows &R, const double lon, const int32_t syear, const long long k) {
  uint32_t itmp[43];
  const uint32_t w = (uint32_t)chkd_bits(lon);
#pragma unroll
  for (int q = 0; q < 36; ++q) itmp[q] = w;
  const int64_t id = R.id[k];
  itmp[36] = (uint32_t)(int32_t)R.halo[k]; itmp[37] = (uint32_t)(int32_t)R.stat[k]; itmp[38] = (uint32_t)syear;
  itmp[39] = (uint32_t)R.ine[k]; itmp[40] = (uint32_t)R.jne[k];
  itmp[41] = (uint32_t)(int32_t)(id >> 32); itmp[42] = (uint32_t)(int32_t)(id & 0xFFFFFFFFll);
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (uint32_t q = 1; q <= 43; ++q) { c1 += itmp[q - 1]; c2 += itmp[q - 1] * q; c3 += itmp[q - 1] * q * q; }
  return (int32_t)(c1 + c2 + c3);
}
// a lane per position q of the order.  hand[q] = mass, hand[n + q] = time_hash * pos_hash for the positions that count;
// words[0..2] += chksum, chksum2, chksum5
__global__ void __launch_bounds__(256) chkd_berg_kernel(const ChkdRows R, const unsigned *__restrict__ keys, const int *__restrict__ rows, const int *__restrict__ cs,
                                                        const int *__restrict__ smax_rev, const long long n, const int ncomp, double *__restrict__ hand,
                                                        unsigned long long *__restrict__ words) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  unsigned long long c1 = 0ull, c2 = 0ull, c5 = 0ull;
  const unsigned c = q < n ? keys[q] : (unsigned)ncomp;
  if (c < (unsigned)ncomp) {
    const long long k = rows[q];
    const int r = (int)(q - (long long)cs[c]);
    const int32_t syear = R.syear[k];
    const double sday = R.sday[k], slon = R.slon[k], slat = R.slat[k];
    const double time_hash = sday + 366. * (double)syear, pos_hash = slon + 360. * (slat + 90.);   // FW:4364-4376
    double v[19];
    v[4] = R.f[4][k];   // mass
    hand[q] = v[4];
    hand[n + q] = time_hash * pos_hash;
    const bool kept = r >= smax_rev[ncomp - 1 - (int)c], last = c == (unsigned)(ncomp - 1);
    if (kept || last) {
      v[0] = R.f[0][k];
      const int32_t iberg = chkd_berg_chksum(R, v[0], syear, k);
      if (last) c5 = (unsigned long long)(uint32_t)iberg;
      if (kept) {
#pragma unroll
        for (int s = 1; s < 16; ++s) if (s != 4) v[s] = R.f[s][k];
        v[16] = time_hash; v[17] = pos_hash; v[18] = (double)iberg;
        const double w = (double)(r + 1);
#pragma unroll
        for (int s = 0; s < 19; ++s) { c1 += chkd_bits(v[s]); c2 += chkd_bits(v[s] * w); }
      }
    }
  }
  c1 = chkd_wave_sum(c1); c2 = chkd_wave_sum(c2); c5 = chkd_wave_sum(c5);
  if (__lane_id() == 0) {
    if (c1) atomicAdd(words + 0, c1);
    if (c2) atomicAdd(words + 1, c2);
    if (c5) atomicAdd(words + 2, c5);
  }
}

static ChkDom chkd_dom(const kid_handle *h) {
  const kid_grid_desc &d = h->gd;
  return ChkDom{d.isc - d.isd, d.jsc - d.jsd, d.iec - d.isc + 1, d.jec - d.jsc + 1, h->ni, d.isc, d.jsc, (long long)h->ncell};
}

// records of fields [0, nf) of `tab` into out[0 .. nf)
static int chkd_planes(kid_handle *h, const ChkTab &tab, int nf, kid_grd_chksum *out) {
  const ChkDom g = chkd_dom(h);
  const long long ncomp = (long long)g.nic * g.njc;
  int maxnk = 1;
  for (int f = 0; f < nf; ++f) if (tab.f[f].present) maxnk = std::max(maxnk, tab.f[f].nk);
  const int nblk = (int)((ncomp * maxnk + CHKD_EPB - 1) / CHKD_EPB);
  double *blk = nullptr;
  const size_t npart = (size_t)nf * (size_t)nblk;
  KID_HIP(h, h->mem.dev(blk, npart * (CHKD_NPD + CHKD_NU) + (size_t)nf * (CHKD_ND + CHKD_NU)));
  double *pd = blk, *rd = blk + npart * (CHKD_NPD + CHKD_NU);
  unsigned long long *pu = (unsigned long long *)(blk + npart * CHKD_NPD), *ru = (unsigned long long *)(rd + (size_t)nf * CHKD_ND);
  std::vector<double> res((size_t)nf * (CHKD_ND + CHKD_NU));
  ChkMeans means{};
  const dim3 grid((unsigned)nblk, (unsigned)nf), block(256);
  hipLaunchKernelGGL(chkd_sweep_kernel<1>, grid, block, 0, h->stream, tab, means, g, pd, pu, nblk);
  hipLaunchKernelGGL(chkd_finish_kernel<1>, dim3((unsigned)nf), block, 0, h->stream, tab, g, (const double *)pd, (const unsigned long long *)pu, nblk, rd, ru);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(res.data(), rd, res.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) {
    for (int f = 0; f < nf; ++f) {
      const long long N = tab.f[f].present ? ncomp * tab.f[f].nk : 0;
      means.m[f] = N ? res[(size_t)f * CHKD_ND + CHKD_SUM] / (double)N : 0.;   // FW:6864
    }
    hipLaunchKernelGGL(chkd_sweep_kernel<2>, grid, block, 0, h->stream, tab, means, g, pd, pu, nblk);
    hipLaunchKernelGGL(chkd_finish_kernel<2>, dim3((unsigned)nf), block, 0, h->stream, tab, g, (const double *)pd, (const unsigned long long *)pu, nblk, rd, ru);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(res.data(), rd, res.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  const hipError_t e2 = h->mem.drop(blk);
  KID_HIP(h, e);
  KID_HIP(h, e2);
  for (int f = 0; f < nf; ++f) {
    kid_grd_chksum &o = out[f];
    o = kid_grd_chksum{};
    if (!tab.f[f].present) continue;
    const double *d = &res[(size_t)f * CHKD_ND];
    uint64_t u[2];
    std::memcpy(u, &res[(size_t)nf * CHKD_ND + (size_t)f * CHKD_NU], sizeof(u));
    const double cnt = (double)(ncomp * tab.f[f].nk);
    o.chksum = chk_low32(u[0]); o.chksum2 = chk_low32(u[1]);
    o.minv = d[CHKD_MIN]; o.maxv = d[CHKD_MAX];
    o.mean = means.m[f];
    o.rms = std::sqrt(d[CHKD_SUMSQ] / cnt);   // FW:6865
    o.sd = std::sqrt(d[CHKD_SD] / cnt);       // FW:6872
    o.present = 1;
  }
  return KID_OK;
}

struct ChkdTmp { unsigned long long *k64[2] = {nullptr, nullptr}, *words = nullptr; int *rows[2] = {nullptr, nullptr}, *cs = nullptr, *rev = nullptr, *smax = nullptr;
                 double *hand = nullptr, *plane = nullptr; Scratch tmp; };
static hipError_t chkd_tmp_free(kid_handle *h, ChkdTmp &t) {
  hipError_t first = hipSuccess;
  auto note = [&first](hipError_t e) { if (first == hipSuccess) first = e; };
  for (int q = 0; q < 2; ++q) { note(h->mem.drop(t.k64[q])); note(h->mem.drop(t.rows[q])); }
  note(h->mem.drop(t.words)); note(h->mem.drop(t.cs)); note(h->mem.drop(t.rev)); note(h->mem.drop(t.smax)); note(h->mem.drop(t.hand)); note(h->mem.drop(t.plane));
  note((hipError_t)h->mem.release(&t.tmp.p));
  t.tmp.bytes = 0;
  return first;
}

static int chkd_bergs(kid_handle *h, ChkdTmp &t, int64_t out[6], kid_grd_chksum *per_cell) {
  const kid_grid_desc &d = h->gd;
  const ChkDom g = chkd_dom(h);
  const long long n = h->n;
  const int ncomp = g.nic * g.njc;
  const dim3 block(256), grid_n((unsigned)((n + 255) / 256)), grid_c((unsigned)((ncomp + 255) / 256));
  for (int q = 0; q < 6; ++q) out[q] = 0;
  if (per_cell) KID_HIP(h, h->mem.dev(t.plane, h->ncell, 0));
  std::vector<int> cs;
  uint64_t words[3] = {0, 0, 0};
  const bool timing = h->dbg.chksum_timing;
  double t_ms[3] = {0., 0., 0.};   // device work, the 16 B/berg transfer, the host fold
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
  if (n > 0) {
    const auto t0 = now();
    const size_t sn = (size_t)n;
    for (int q = 0; q < 2; ++q) { KID_HIP(h, h->mem.dev(t.k64[q], sn)); KID_HIP(h, h->mem.dev(t.rows[q], sn)); }
    KID_HIP(h, h->mem.dev(t.cs, (size_t)ncomp + 1));
    KID_HIP(h, h->mem.dev(t.rev, (size_t)ncomp));
    KID_HIP(h, h->mem.dev(t.smax, (size_t)ncomp));
    KID_HIP(h, h->mem.dev(t.hand, 2 * sn));
    KID_HIP(h, h->mem.dev(t.words, 3, 0));
    unsigned *k32[2] = {(unsigned *)t.k64[0], (unsigned *)t.k64[1]};
    size_t b64 = 0, b32 = 0, bsc = 0;
    KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b64, t.k64[0], t.k64[1], t.rows[0], t.rows[1], sn, 0, 64, h->stream));
    KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b32, k32[0], k32[1], t.rows[0], t.rows[1], sn, 0, 32, h->stream));
    KID_HIP(h, rocprim::exclusive_scan(nullptr, bsc, t.rev, t.smax, 0, (size_t)ncomp, rocprim::maximum<int>(), h->stream));
    KID_HIP(h, h->mem.reserve(t.tmp, std::max(std::max(b64, b32), bsc)));
    // the order: least significant key first, every pass stable, on top of the identity (the row is the last tie)
    int cur = 0;
    hipLaunchKernelGGL(mts_iota_kernel, grid_n, block, 0, h->stream, t.rows[cur], n);
    const int f64_keys[4] = {KID_B_START_LAT, KID_B_START_LON, KID_B_START_MASS, KID_B_START_DAY};
    for (int pass = 0; pass < 5; ++pass) {
      if (pass < 4) hipLaunchKernelGGL(chkd_key_f64_kernel, grid_n, block, 0, h->stream, (const double *)h->bp.f[f64_keys[pass]], (const int *)t.rows[cur], t.k64[0], n);
      else hipLaunchKernelGGL(mts_key_i32_kernel, grid_n, block, 0, h->stream, (const int32_t *)h->bp.i[KID_BI_START_YEAR], (const int *)t.rows[cur], t.k64[0], n);
      size_t bytes = t.tmp.bytes;
      KID_HIP(h, rocprim::radix_sort_pairs(t.tmp.p, bytes, t.k64[0], t.k64[1], t.rows[cur], t.rows[cur ^ 1], sn, 0, 64, h->stream));
      cur ^= 1;
    }
    hipLaunchKernelGGL(chkd_key_cell_kernel, grid_n, block, 0, h->stream, (const int32_t *)h->bp.i[KID_BI_ALIVE], (const int32_t *)h->bp.i[KID_BI_INE], (const int32_t *)h->bp.i[KID_BI_JNE],
                       (const int *)t.rows[cur], k32[0], n, d.isc, d.iec, d.jsc, d.jec, (unsigned)ncomp);
    {
      const unsigned bits = 32u - (unsigned)__builtin_clz((unsigned)ncomp);   // keys 0 .. ncomp
      size_t bytes = t.tmp.bytes;
      KID_HIP(h, rocprim::radix_sort_pairs(t.tmp.p, bytes, k32[0], k32[1], t.rows[cur], t.rows[cur ^ 1], sn, 0, bits, h->stream));
      cur ^= 1;
    }
    hipLaunchKernelGGL(repro_cell_start_kernel, grid_n, block, 0, h->stream, (const unsigned *)k32[1], t.cs, n, (unsigned)ncomp);
    hipLaunchKernelGGL(chkd_counts_kernel, grid_c, block, 0, h->stream, (const int *)t.cs, t.rev, t.plane, g);
    {
      size_t bytes = t.tmp.bytes;
      KID_HIP(h, rocprim::exclusive_scan(t.tmp.p, bytes, t.rev, t.smax, 0, (size_t)ncomp, rocprim::maximum<int>(), h->stream));
    }
    ChkdRows R{};
    static const int F16[16] = {KID_B_LON, KID_B_LAT, KID_B_UVEL, KID_B_VVEL, KID_B_MASS, KID_B_THICKNESS, KID_B_WIDTH, KID_B_LENGTH, KID_B_AXN, KID_B_AYN,
                                KID_B_BXN, KID_B_BYN, KID_B_UVEL_OLD, KID_B_VVEL_OLD, KID_B_LON_OLD, KID_B_LAT_OLD};
    for (int s = 0; s < 16; ++s) R.f[s] = h->bp.f[F16[s]];
    R.sday = h->bp.f[KID_B_START_DAY]; R.slon = h->bp.f[KID_B_START_LON]; R.slat = h->bp.f[KID_B_START_LAT];
    R.halo = h->bp.f[KID_B_HALO_BERG]; R.stat = h->bp.f[KID_B_STATIC_BERG];
    R.syear = h->bp.i[KID_BI_START_YEAR]; R.ine = h->bp.i[KID_BI_INE]; R.jne = h->bp.i[KID_BI_JNE]; R.id = h->bp.id;
    hipLaunchKernelGGL(chkd_berg_kernel, grid_n, block, 0, h->stream, R, (const unsigned *)k32[1], (const int *)t.rows[cur], (const int *)t.cs, (const int *)t.smax, n, ncomp, t.hand, t.words);
    KID_HIP(h, hipGetLastError());
    cs.resize((size_t)ncomp + 1);
    KID_HIP(h, hipMemcpyAsync(cs.data(), t.cs, cs.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(words, t.words, sizeof(words), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    t_ms[0] = ms_since(t0);
    const size_t m = (size_t)cs[(size_t)ncomp];   // the rows that count
    std::vector<double> mass(m), thph(m);
    const auto t1 = now();
    if (m) {
      KID_HIP(h, hipMemcpyAsync(mass.data(), t.hand, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      KID_HIP(h, hipMemcpyAsync(thph.data(), t.hand + sn, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      KID_HIP(h, hipStreamSynchronize(h->stream));
    }
    t_ms[1] = ms_since(t1);
    const auto t2 = now();
    uint64_t s3 = 0;
    for (int c = 0; c < ncomp; ++c) {
      if (cs[(size_t)c + 1] == cs[(size_t)c]) continue;   // grd%tmp stays +0.0: no bits
      double tmp = 0.;
      for (int q = cs[(size_t)c]; q < cs[(size_t)c + 1]; ++q) tmp = tmp + thph[(size_t)q] + std::log(mass[(size_t)q]);   // kid_chksum.inc:86
      s3 += chk_bits(tmp);
    }
    t_ms[2] = ms_since(t2);
    out[0] = chk_low32(words[0]); out[1] = chk_low32(words[1]);
    out[2] = chk_low32(s3); out[3] = chk_low32(s3);   // the halo of grd%tmp holds +0.0: chksum3 = chksum4 on one PE
    out[4] = (int32_t)(uint32_t)words[2];
    out[5] = (int64_t)m;
  }
  if (per_cell) {   // FW:6978-6979
    ChkTab tab{};
    tab.f[0] = ChkField{t.plane, 1, 1};
    const int rc = chkd_planes(h, tab, 1, per_cell);
    if (rc) return rc;
  }
  if (timing) fprintf(stderr, "kid_bergs_chksum_device: n %lld, device %.3f ms, transfer %.3f ms, host log fold %.3f ms\n", n, t_ms[0], t_ms[1], t_ms[2]);
  return KID_OK;
}

}  // namespace

extern "C" int kid_bergs_chksum_device(kid_handle *h, int64_t out[6], kid_grd_chksum *per_cell) {
  if (!h || !out) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_bergs_chksum_device"); if (rc_h) return rc_h; }
  { const int rc_e = rows_enter(h, ROWS_READ); if (rc_e) return rc_e; }
  ChkdTmp t;
  const int rc = chkd_bergs(h, t, out, per_cell);
  const hipError_t e = chkd_tmp_free(h, t);
  if (rc) return rc;
  KID_HIP(h, e);
  return KID_OK;
}

extern "C" int kid_checksum_gridded(kid_handle *h, kid_grd_chksum *out, int32_t n_out) {
  if (!h || !out) return KID_EINVAL;
  if (n_out < KID_NCHK) { h->err = "kid_checksum_gridded: out must hold KID_NCHK records"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  ChkTab tab{};
  auto set = [&tab](int which, const double *p, int nk, bool present) { tab.f[which] = ChkField{present ? p : nullptr, nk, present ? 1 : 0}; };
  // forcing: the planes kid_get_forcing returns, each once it has been given; grd%calving, grd%calving_hflx: kid_get_calving
  static const int forc[11][2] = {{KID_CHK_UO, KID_F_UO}, {KID_CHK_VO, KID_F_VO}, {KID_CHK_UA, KID_F_UA}, {KID_CHK_VA, KID_F_VA}, {KID_CHK_UI, KID_F_UI}, {KID_CHK_VI, KID_F_VI},
                                  {KID_CHK_SSH, KID_F_SSH}, {KID_CHK_SST, KID_F_SST}, {KID_CHK_SSS, KID_F_SSS}, {KID_CHK_HI, KID_F_HI}, {KID_CHK_CN, KID_F_CN}};
  for (const auto &m : forc) set(m[0], h->d_forcing[m[1]], 1, forcing_held(h, m[1]));
  const bool calv = h->calving_on && h->d_calv_state;
  set(KID_CHK_CALVING, calv ? calv_plane(h, CALV_CALVING) : nullptr, 1, calv);
  set(KID_CHK_CALVING_HFLX, calv ? calv_plane(h, CALV_HFLX) : nullptr, 1, calv);
  set(KID_CHK_STORED_ICE, calv ? calv_plane(h, CALV_STORED_ICE) : nullptr, KID_NCLASSES, calv);
  set(KID_CHK_RMEAN_CALVING, calv ? calv_plane(h, CALV_RMEAN) : nullptr, 1, calv);
  set(KID_CHK_RMEAN_CALVING_HFLX, calv ? calv_plane(h, CALV_RMEAN_HFLX) : nullptr, 1, calv);
  set(KID_CHK_STORED_HEAT, calv ? calv_plane(h, CALV_STORED_HEAT) : nullptr, 1, calv);
  // state: the accumulator planes of kid_get_accumulators; a plane the step neither zeroes nor fills (plane_range_live, kid_planes.hpp) reads as zeros
  auto acc = [&](int which, int plane, int nk) {
    const bool live = plane_range_live(plane, nk, h->params.pass_fields_to_ocean_model, h->params.diag_mask);
    tab.f[which] = ChkField{live ? h->d_acc + (size_t)plane * h->ncell : nullptr, nk, 1};
  };
  constexpr int S = ON_OCEAN_SLOTS;
  static const int accs[][3] = {{KID_CHK_MASS, KID_A_MASS, 1}, {KID_CHK_MASS_ON_OCEAN, KID_A_MASS_ON_OCEAN, S}, {KID_CHK_AREA_ON_OCEAN, KID_A_AREA_ON_OCEAN, S},
    {KID_CHK_UVEL_ON_OCEAN, KID_A_UVEL_ON_OCEAN, S}, {KID_CHK_VVEL_ON_OCEAN, KID_A_VVEL_ON_OCEAN, S}, {KID_CHK_MELT_B, KID_A_MELT_BUOY, 1}, {KID_CHK_MELT_E, KID_A_MELT_EROS, 1},
    {KID_CHK_MELT_V, KID_A_MELT_CONV, 1}, {KID_CHK_BERGY_SRC, KID_A_BERGY_SRC, 1}, {KID_CHK_BERGY_MELT, KID_A_BERGY_MELT, 1}, {KID_CHK_BERGY_MASS, KID_A_BERGY_MASS, 1},
    {KID_CHK_FL_BITS_SRC, KID_A_FL_BITS_SRC, 1}, {KID_CHK_FL_BITS_MELT, KID_A_FL_BITS_MELT, 1}, {KID_CHK_FL_BITS_MASS, KID_A_FL_BITS_MASS, 1},
    {KID_CHK_FL_BERGY_BITS_MASS, KID_A_FL_BERGY_BITS_MASS, 1}, {KID_CHK_U_ICEBERG, KID_A_U_ICEBERG, 1}, {KID_CHK_V_ICEBERG, KID_A_V_ICEBERG, 1}, {KID_CHK_VAREA, KID_A_VIRTUAL_AREA, 1},
    {KID_CHK_FLOATING_MELT, KID_A_FLOATING_MELT, 1}, {KID_CHK_BERG_MELT, KID_A_BERG_MELT, 1}, {KID_CHK_MELT_BY_CLASS, KID_A_MELT_BY_CLASS, KID_NCLASSES},
    {KID_CHK_MELT_B_FL, KID_A_MELT_BUOY_FL, 1}, {KID_CHK_MELT_E_FL, KID_A_MELT_EROS_FL, 1}, {KID_CHK_MELT_V_FL, KID_A_MELT_CONV_FL, 1},
    {KID_CHK_FL_PARENT_MELT, KID_A_FL_PARENT_MELT, 1}, {KID_CHK_FL_CHILD_MELT, KID_A_FL_CHILD_MELT, 1}};
  for (const auto &m : accs) acc(m[0], m[1], m[2]);
  static const int outs[5][2] = {{KID_CHK_SPREAD_MASS, KID_O_SPREAD_MASS}, {KID_CHK_SPREAD_AREA, KID_O_SPREAD_AREA}, {KID_CHK_SPREAD_UVEL, KID_O_SPREAD_UVEL},
                                 {KID_CHK_SPREAD_VVEL, KID_O_SPREAD_VVEL}, {KID_CHK_USTAR_ICEBERG, KID_O_USTAR_ICEBERG}};
  for (const auto &m : outs) set(m[0], h->d_out + (size_t)m[1] * h->ncell, 1, true);
  // static: the planes of kid_set_static_grid, in the enum's order (lonc and latc are optional there)
  for (int k = 0; k < KID_NGRID_STATIC; ++k) set(KID_CHK_LON + k, h->d_static[k], 1, h->forc.have_static && ((k != KID_G_LONC && k != KID_G_LATC) || h->forc.have_centres));
  return chkd_planes(h, tab, KID_NCHK, out);
}
