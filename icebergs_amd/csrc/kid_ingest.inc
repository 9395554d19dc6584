// kid_ingest.inc -- forcing ingest on the device (SURVEY.md 8f N1): the block of icebergs_run that turns the coupler's
// arguments into grd%uo .. grd%hi, /root/reference/src/icebergs.F90:5236-5383, and invert_tau_for_du IB:8272-8296.
// Four tiny per-cell launches on the handle's stream, in the reference's order of effects:
//   ingest_sstmax_kernel : maxval(sst*msk) over the computational domain (the Kelvin test, IB:5340)
//   ingest_write_kernel  : every assignment / stagger interpolation into the planes + invert_tau_for_du on the whole plane
//   ingest_wrap_kernel   : mpp_update_domains as ONE rank sees it: halo columns of a zonally cyclic domain take the
//                          column one period away; a closed domain keeps its halo (cells the block does not write keep
//                          their previous content, as grd%* do)
//   ingest_scrub_kernel  : land (msk<0.5) and NaN scrub, IB:5364-5383
// The phases stay separate launches because the wrap reads interior cells the scrub rewrites.
struct IngestArgs {
  const double *uo, *vo, *ui, *vi, *tauxa, *tauya, *ssh, *sst, *cn, *hi, *sss;
  double *out[KID_NFORCING];
  const double *msk;
  unsigned long long *sstmax_key;
  int ni, nj;                       // data-domain extents
  int ic0, ic1, jc0, jc1;           // computational domain as 0-based data-domain offsets (inclusive)
  int u_ni, u_nj, v_ni, v_nj, taux_ni, taux_nj, tauy_ni, tauy_nj;
  int Iu_off, ju_off, iv_off, Jv_off;       // C-grid velocity offsets, IB:5246-5249, rebased to 0-based (i - isd) indices
  int tIu_off, tju_off, tiv_off, tJv_off;   // same for the stresses, IB:5270-5273
  int vel_stagger, stress_stagger, tau_is_velocity, cyclic_x;
};

// order-preserving map of a double to an unsigned key (so the maximum is one integer atomic)
__device__ __forceinline__ unsigned long long ingest_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ingest_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(256) ingest_sstmax_kernel(IngestArgs a) {
  const int nic = a.ic1 - a.ic0 + 1, njc = a.jc1 - a.jc0 + 1;
  unsigned long long best = 0ull;  // below the key of every number
  for (int j = blockIdx.x; j < njc; j += gridDim.x) {  // one row of the computational domain per workgroup pass
    const double *sst = a.sst + (size_t)j * nic, *msk = a.msk + (size_t)a.ic0 + (size_t)(j + a.jc0) * a.ni;
    for (int i = threadIdx.x; i < nic; i += blockDim.x) {
      const double v = sst[i] * msk[i];
      if (v == v) { const unsigned long long k = ingest_key(v); best = k > best ? k : best; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o > best ? o : best; }
  __shared__ unsigned long long wave_best[4];
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic per workgroup: same-address 64-bit atomics serialise
    for (int w = 1; w < 4; ++w) best = wave_best[w] > best ? wave_best[w] : best;
    if (best) atomicMax(a.sstmax_key, best);
  }
}

// value of the zero-initialised, zonally updated work copy uC_tmp / uA_tmp (IB:5274-5285, 5296-5302) at data cell (i, j)
__device__ __forceinline__ double ingest_tau_tmp(const IngestArgs &a, const double *tau, int tni, int ioff, int joff, int i, int j) {
  if (j < a.jc0 || j > a.jc1) return 0.;
  const int nic = a.ic1 - a.ic0 + 1;
  if (i < a.ic0) { if (!a.cyclic_x) return 0.; i += nic; } else if (i > a.ic1) { if (!a.cyclic_x) return 0.; i -= nic; }
  return tau[(size_t)(i + ioff) + (size_t)(j + joff) * tni];
}

__global__ void __launch_bounds__(256) ingest_write_kernel(IngestArgs a) {
  const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (c >= (long long)a.ni * a.nj) return;
  const int i = (int)(c % a.ni), j = (int)(c / a.ni);
  const int nic = a.ic1 - a.ic0 + 1;
  const bool in_c = i >= a.ic0 && i <= a.ic1 && j >= a.jc0 && j <= a.jc1;           // (isc:iec, jsc:jec)
  const bool in_c1 = i >= a.ic0 - 1 && i <= a.ic1 + 1 && j >= a.jc0 - 1 && j <= a.jc1 + 1;  // (isc-1:iec+1, jsc-1:jec+1)
  const bool in_sw = i >= a.ic0 - 1 && i <= a.ic1 && j >= a.jc0 - 1 && j <= a.jc1;  // (isc-1:iec, jsc-1:jec)
  double mask = 0.;
  if (in_sw) mask = fmin(fmin(a.msk[c], a.msk[c + 1]), fmin(a.msk[c + a.ni], a.msk[c + a.ni + 1]));  // IB:5254
  const size_t h1 = in_c1 ? (size_t)(i - (a.ic0 - 1)) + (size_t)(j - (a.jc0 - 1)) * (nic + 2) : 0;   // index in a one-cell-halo input
  const size_t h0 = in_c ? (size_t)(i - a.ic0) + (size_t)(j - a.jc0) * nic : 0;                       // index in a computational-domain input
  if (a.vel_stagger == KID_BGRID_NE) {  // IB:5236-5243
    if (in_c1) { a.out[KID_F_UO][c] = a.uo[h1]; a.out[KID_F_VO][c] = a.vo[h1]; a.out[KID_F_UI][c] = a.ui[h1]; a.out[KID_F_VI][c] = a.vi[h1]; }
  } else if (in_sw) {  // C-grid, IB:5250-5259
    const size_t pu = (size_t)(i + a.Iu_off) + (size_t)(j + a.ju_off) * a.u_ni, pv = (size_t)(i + a.iv_off) + (size_t)(j + a.Jv_off) * a.v_ni;
    a.out[KID_F_UO][c] = mask * 0.5 * (a.uo[pu] + a.uo[pu + a.u_ni]);
    a.out[KID_F_UI][c] = mask * 0.5 * (a.ui[pu] + a.ui[pu + a.u_ni]);
    a.out[KID_F_VO][c] = mask * 0.5 * (a.vo[pv] + a.vo[pv + 1]);
    a.out[KID_F_VI][c] = mask * 0.5 * (a.vi[pv] + a.vi[pv + 1]);
  }
  double ua = a.out[KID_F_UA][c], va = a.out[KID_F_VA][c];  // cells the block does not write keep what they held
  if (a.stress_stagger == KID_BGRID_NE) {  // IB:5264-5267
    if (in_c) { ua = a.tauxa[h0]; va = a.tauya[h0]; }
  } else if (in_sw) {
    if (a.stress_stagger == KID_CGRID_NE) {  // IB:5286-5292
      ua = mask * 0.5 * (ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i, j) + ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i, j + 1));
      va = mask * 0.5 * (ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i, j) + ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i + 1, j));
    } else {  // A-grid, IB:5303-5311
      ua = mask * 0.25 * ((ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i, j) + ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i + 1, j + 1)) +
                          (ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i + 1, j) + ingest_tau_tmp(a, a.tauxa, a.taux_ni, a.tIu_off, a.tju_off, i, j + 1)));
      va = mask * 0.25 * ((ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i, j) + ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i + 1, j + 1)) +
                          (ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i + 1, j) + ingest_tau_tmp(a, a.tauya, a.tauy_ni, a.tiv_off, a.tJv_off, i, j + 1)));
    }
  }
  if (!a.tau_is_velocity) {  // invert_tau_for_du over the whole plane, IB:5321-5323, 8272-8296
    const double tau2 = ua * ua + va * va, cddvmod = sqrt(0.0015 * sqrt(tau2));
    if (cddvmod != 0.) { ua = ua / cddvmod; va = va / cddvmod; } else { ua = 0.; va = 0.; }
  }
  a.out[KID_F_UA][c] = ua; a.out[KID_F_VA][c] = va;
  if (in_c1) { a.out[KID_F_SSH][c] = a.ssh[h1]; a.out[KID_F_CN][c] = a.cn[h1]; a.out[KID_F_HI][c] = a.hi[h1]; }  // IB:5329, 5348, 5350
  if (in_c) {
    const bool kelvin = ingest_unkey(*a.sstmax_key) > 120.0;  // IB:5340-5345 (an all-NaN field leaves the key at 0 = "not Kelvin")
    a.out[KID_F_SST][c] = (*a.sstmax_key && kelvin) ? a.sst[h0] - 273.15 : a.sst[h0];
    a.out[KID_F_SSS][c] = a.sss ? a.sss[h0] : -1.0;           // IB:5354-5357
  }
}

__global__ void __launch_bounds__(256) ingest_wrap_kernel(IngestArgs a) {  // IB:5240, 5243, 5318-5319, 5326, 5339, 5346, 5349, 5351
  const int nic = a.ic1 - a.ic0 + 1, nhalo = a.ni - nic;  // halo columns of a row: [0, ic0) and (ic1, ni)
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)nhalo * a.nj) return;
  const int q = (int)(t % nhalo), j = (int)(t / nhalo);
  const int i = q < a.ic0 ? q : a.ic1 + 1 + (q - a.ic0);
  const int src = i < a.ic0 ? i + nic : i - nic;
  const size_t c = (size_t)i + (size_t)j * a.ni, s = (size_t)src + (size_t)j * a.ni;
#pragma unroll
  for (int k = 0; k < KID_NFORCING; ++k) if (k != KID_F_SSS) a.out[k][c] = a.out[k][s];  // grd%sss is never updated
}

__global__ void __launch_bounds__(256) ingest_scrub_kernel(IngestArgs a) {  // IB:5364-5383
  const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (c >= (long long)a.ni * a.nj) return;
  const bool land = a.msk[c] < 0.5;
#pragma unroll
  for (int k = 0; k < KID_NFORCING; ++k) {
    if (k == KID_F_SSH) continue;  // ssh is neither masked nor scrubbed
    const double v = a.out[k][c];
    if (land || v != v) a.out[k][c] = 0.;
  }
}

// host arrays pass through one device block, shared with kid_calving; a kernel may still read the block it outgrows
static int ingest_stage_reserve(kid_handle *h, size_t count) {
  if (count <= h->ingest_stage_count) return KID_OK;
  if (h->d_ingest_stage) { KID_HIP(h, hipStreamSynchronize(h->stream)); KID_HIP(h, h->mem.drop(h->d_ingest_stage)); }
  h->ingest_stage_count = 0;
  KID_HIP(h, h->mem.dev(h->d_ingest_stage, count));
  h->ingest_stage_count = count;
  return KID_OK;
}
static int ingest_stage(kid_handle *h, const kid_forcing_in *in, const size_t cnt[11], const double *src[11], const double *dev[11]) {
  size_t total = 0;
  for (int k = 0; k < 11; ++k) total += src[k] ? cnt[k] : 0;
  if (in->on_device) { for (int k = 0; k < 11; ++k) dev[k] = src[k]; return KID_OK; }
  { const int rc = ingest_stage_reserve(h, total); if (rc) return rc; }
  size_t off = 0;
  for (int k = 0; k < 11; ++k) {
    if (!src[k]) { dev[k] = nullptr; continue; }
    KID_HIP(h, hipMemcpyAsync(h->d_ingest_stage + off, src[k], cnt[k] * sizeof(double), hipMemcpyHostToDevice, h->stream));
    dev[k] = h->d_ingest_stage + off; off += cnt[k];
  }
  return KID_OK;
}

int kid_ingest_forcing(kid_handle *h, const kid_forcing_in *in) {
  if (!h || !in) return KID_EINVAL;
  if (need_static(h)) return KID_EINVAL;
  const kid_grid_desc &d = h->gd;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1;
  if (d.isc - 1 < d.isd || d.iec + 1 > d.ied || d.jsc - 1 < d.jsd || d.jec + 1 > d.jed) { h->err = "forcing ingest needs a halo of at least one cell"; return KID_EINVAL; }
  if (in->cyclic_x && (d.isc - d.isd > nic || d.ied - d.iec > nic)) { h->err = "halo wider than the zonal period"; return KID_EINVAL; }
  if (!in->uo || !in->vo || !in->ui || !in->vi || !in->tauxa || !in->tauya || !in->ssh || !in->sst || !in->cn || !in->hi) { h->err = "forcing ingest: a required array is NULL"; return KID_EINVAL; }
  IngestArgs a{};
  a.ni = h->ni; a.nj = h->nj;
  a.ic0 = d.isc - d.isd; a.ic1 = d.iec - d.isd; a.jc0 = d.jsc - d.jsd; a.jc1 = d.jec - d.jsd;
  a.u_ni = in->u_ni; a.u_nj = in->u_nj; a.v_ni = in->v_ni; a.v_nj = in->v_nj;
  a.taux_ni = in->taux_ni; a.taux_nj = in->taux_nj; a.tauy_ni = in->tauy_ni; a.tauy_nj = in->tauy_nj;
  a.vel_stagger = in->vel_stagger; a.stress_stagger = in->stress_stagger; a.tau_is_velocity = in->tau_is_velocity; a.cyclic_x = in->cyclic_x;
  // Fortran offsets (1-based input index = model index + off) -> 0-based input index = 0-based data index + off0
  auto rebase = [](int size, int c0, int c1, int sd) { return (size - (c1 - c0)) / 2 - c0 + 1 + sd - 1; };
  if (in->vel_stagger == KID_BGRID_NE) {
    if (in->u_ni != nic + 2 || in->u_nj != njc + 2 || in->v_ni != nic + 2 || in->v_nj != njc + 2) { h->err = "B-grid velocities must cover (isc-1:iec+1, jsc-1:jec+1)"; return KID_EINVAL; }
  } else if (in->vel_stagger == KID_CGRID_NE) {
    a.Iu_off = rebase(in->u_ni, d.isc, d.iec, d.isd); a.ju_off = rebase(in->u_nj, d.jsc, d.jec, d.jsd);
    a.iv_off = rebase(in->v_ni, d.isc, d.iec, d.isd); a.Jv_off = rebase(in->v_nj, d.jsc, d.jec, d.jsd);
    // the loop (isc-1:iec, jsc-1:jec) reads uo(Iu, ju:ju+1) and vo(iv:iv+1, Jv)
    if (a.ic0 - 1 + a.Iu_off < 0 || a.ic1 + a.Iu_off > in->u_ni - 1 || a.jc0 - 1 + a.ju_off < 0 || a.jc1 + 1 + a.ju_off > in->u_nj - 1 ||
        a.ic0 - 1 + a.iv_off < 0 || a.ic1 + 1 + a.iv_off > in->v_ni - 1 || a.jc0 - 1 + a.Jv_off < 0 || a.jc1 + a.Jv_off > in->v_nj - 1) {
      h->err = "C-grid velocity extents do not cover the interpolation stencil"; return KID_EINVAL;
    }
  } else { h->err = "Unrecognized value of stagger!"; return KID_EINVAL; }  // IB:5261
  if (in->stress_stagger == KID_BGRID_NE || in->stress_stagger == KID_AGRID) {
    if (in->taux_ni != nic || in->taux_nj != njc || in->tauy_ni != nic || in->tauy_nj != njc) { h->err = "wind stress must cover the computational domain"; return KID_EINVAL; }
    a.tIu_off = a.tiv_off = -a.ic0; a.tju_off = a.tJv_off = -a.jc0;
  } else if (in->stress_stagger == KID_CGRID_NE) {
    a.tIu_off = rebase(in->taux_ni, d.isc, d.iec, d.isd); a.tju_off = rebase(in->taux_nj, d.jsc, d.jec, d.jsd);
    a.tiv_off = rebase(in->tauy_ni, d.isc, d.iec, d.isd); a.tJv_off = rebase(in->tauy_nj, d.jsc, d.jec, d.jsd);
    if (a.ic0 + a.tIu_off < 0 || a.ic1 + a.tIu_off > in->taux_ni - 1 || a.jc0 + a.tju_off < 0 || a.jc1 + a.tju_off > in->taux_nj - 1 ||
        a.ic0 + a.tiv_off < 0 || a.ic1 + a.tiv_off > in->tauy_ni - 1 || a.jc0 + a.tJv_off < 0 || a.jc1 + a.tJv_off > in->tauy_nj - 1) {
      h->err = "C-grid stress extents do not cover the computational domain"; return KID_EINVAL;
    }
  } else { h->err = "Unrecognized value of stress_stagger!"; return KID_EINVAL; }  // IB:5315
  KID_HIP(h, hipSetDevice(h->device));
  const size_t nu = (size_t)in->u_ni * in->u_nj, nv = (size_t)in->v_ni * in->v_nj, n1 = (size_t)(nic + 2) * (njc + 2), n0 = (size_t)nic * njc;
  const size_t cnt[11] = {nu, nv, nu, nv, (size_t)in->taux_ni * in->taux_nj, (size_t)in->tauy_ni * in->tauy_nj, n1, n0, n1, n1, n0};
  const double *src[11] = {in->uo, in->vo, in->ui, in->vi, in->tauxa, in->tauya, in->ssh, in->sst, in->cn, in->hi, in->sss};
  const double *dev[11] = {};
  { const int rc = ingest_stage(h, in, cnt, src, dev); if (rc) return rc; }
  a.uo = dev[0]; a.vo = dev[1]; a.ui = dev[2]; a.vi = dev[3]; a.tauxa = dev[4]; a.tauya = dev[5];
  a.ssh = dev[6]; a.sst = dev[7]; a.cn = dev[8]; a.hi = dev[9]; a.sss = dev[10];
  for (int k = 0; k < KID_NFORCING; ++k) a.out[k] = h->d_forcing[k];
  a.msk = h->d_static[KID_G_MSK];
  if (!h->d_ingest_key) KID_HIP(h, h->mem.dev(h->d_ingest_key, 1));
  a.sstmax_key = h->d_ingest_key;
  KID_HIP(h, hipMemsetAsync(h->d_ingest_key, 0, sizeof(unsigned long long), h->stream));
  const int nb_c = std::min(njc, 512), nb = (int)((h->ncell + 255) / 256);
  hipLaunchKernelGGL(ingest_sstmax_kernel, dim3(nb_c), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(ingest_write_kernel, dim3(nb), dim3(256), 0, h->stream, a);
  if (in->cyclic_x && h->ni > nic) {
    const size_t nw = (size_t)(h->ni - nic) * h->nj;
    hipLaunchKernelGGL(ingest_wrap_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, h->stream, a);
  }
  hipLaunchKernelGGL(ingest_scrub_kernel, dim3(nb), dim3(256), 0, h->stream, a);
  KID_HIP(h, hipGetLastError());
  return forcing_given(h, (1u << KID_NFORCING) - 1u, nullptr, !in->on_device);  // every plane; the per-cell records the berg kernels read
}

int kid_get_forcing(kid_handle *h, double *const fields[KID_NFORCING]) {
  if (!h || !fields) return KID_EINVAL;
  if (!h->forc.have_planes) { h->err = "the handle holds no forcing planes (kid_set_forcing with all fields, or kid_ingest_forcing)"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  for (int k = 0; k < KID_NFORCING; ++k)
    if (fields[k]) KID_HIP(h, hipMemcpyAsync(fields[k], h->d_forcing[k], h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}
