// kid_mts_host.inc -- host side of the multiple-time-stepping / DEM path (included inside extern "C" in kid_hip.hip)

#define MTS_GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, h->stream

static int mts_ensure(kid_handle *h, int mb) {
  if (h->mts_ready && h->mb == mb) return KID_OK;
  if (h->mts_ready) { h->err = "max_bonds cannot change after the bond tables exist"; return KID_EINVAL; }
  const size_t cap = (size_t)h->capacity, nb = (size_t)(mb > 0 ? mb : 1) * cap;
  KID_HIP(h, h->mem.dev(h->mts.bcount, cap, 0));
  KID_HIP(h, h->mem.dev(h->mts.bother_id, nb, 0));
  KID_HIP(h, h->mem.dev(h->mts.bbroken, nb, 0));
  for (int32_t **q : {&h->mts.bother_row, &h->mts.bother_slot}) KID_HIP(h, h->mem.dev(*q, nb, 0xff));   // -1: no partner row known
  for (auto &field : h->mts.bf) KID_HIP(h, h->mem.dev(field, nb, 0));
  for (int32_t **q : {&h->mts.rank, &h->mts.order, &h->mts.label, &h->mts.root_flag, &h->mts.root_scan}) KID_HIP(h, h->mem.dev(*q, cap));
  for (int32_t **q : {&h->mts.cell_start, &h->mts.cell_conglom}) KID_HIP(h, h->mem.dev(*q, h->ncell + 2));
  KID_HIP(h, h->mem.dev(h->mts.red, MR_COUNT, 0));
  KID_HIP(h, h->mem.dev(h->mts.rec, 3 * 8 * cap, 0));
  for (int q = 0; q < 2; ++q) { KID_HIP(h, h->mem.dev(h->d_key64[q], cap)); KID_HIP(h, h->mem.dev(h->d_rows[q], cap)); }
  KID_HIP(h, h->mem.dev(h->d_last_key, cap)); KID_HIP(h, h->mem.dev(h->d_order_flag, 4, 0));   // [0] order changed, [1] bond lists changed, [2] lanes of the fused sub-step kernel that timed out
  KID_HIP(h, h->mem.dev(h->d_bond_sig, cap, 0));
  h->order_n = -1; h->mts_shadow_valid = false; h->labels_stale = true;
  size_t b1 = 0, b2 = 0;
  KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b1, h->d_key64[0], h->d_key64[1], h->d_rows[0], h->d_rows[1], cap, 0, 64, h->stream));
  KID_HIP(h, rocprim::exclusive_scan(nullptr, b2, h->mts.root_flag, h->mts.root_scan, 0, cap, rocprim::plus<int>(), h->stream));
  KID_HIP(h, h->mem.reserve(h->mts_tmp, b1 > b2 ? b1 : b2));
  KID_HIP(h, h->mem.dev(h->d_mts, 1));
  h->mts.stride = (long long)h->capacity; h->mts.mb = mb; h->mts.nperm = 0;
  h->mts.lonc = h->d_static[KID_G_LONC]; h->mts.latc = h->d_static[KID_G_LATC]; h->mts.glon = h->d_static[KID_G_LON];
  h->mb = mb; h->mts_ready = true; h->mts_dirty = true;
  KID_HIP(h, hipStreamSynchronize(h->stream));  // the fills above, before a launch on another stream could read the tables
  return KID_OK;
}
// the tables with the namelist's max_bonds slots (at least one), unless they exist already
static int mts_ensure_default(kid_handle *h) {
  return h->mts_ready ? KID_OK : mts_ensure(h, h->params.max_bonds > 0 ? h->params.max_bonds : 1);
}
static int mts_refresh(kid_handle *h) {  // derived constants + the device copy of the table
  int rc = refresh_tables(h);
  if (rc) return rc;
  const kid_params &p = h->params;
  MtsDev &m = h->mts;
  m.dem_K_damp = 2. * p.dem_spring_coef / (3. * (1. - pow(p.poisson, 2.)));   // FW:1436
  m.constant_area = p.constant_length * p.constant_width;                       // FW:1453-1463
  if (p.hexagonal_icebergs) m.constant_radius = sqrt(m.constant_area / (2. * sqrt(3.)));
  else if (p.iceberg_bonds_on) m.constant_radius = 0.5 * sqrt(m.constant_area);
  else m.constant_radius = sqrt(m.constant_area / p.pi);
  m.mts_fast_dt = p.dt / (double)p.mts_sub_steps;                               // FW:1301
  if (!h->mts_shadow_valid || memcmp(&h->mts_shadow, &h->mts, sizeof(MtsDev)) != 0) {   // (every step would otherwise pay a copy + a stream sync for an identical table)
    KID_HIP(h, hipMemcpyAsync(h->d_mts, &h->mts, sizeof(MtsDev), hipMemcpyHostToDevice, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(&h->mts_shadow, &h->mts, sizeof(MtsDev)); h->mts_shadow_valid = true;
  }
  h->mts_dirty = false;
  return KID_OK;
}

int kid_upload_bonds(kid_handle *h, const kid_bond_soa *host) {
  if (!h || !host || !host->count || !host->other_id) return KID_EINVAL;
  if (host->n != h->n) { h->err = "kid_upload_bonds: upload the bergs first (row counts differ)"; return KID_EINVAL; }
  if (host->max_bonds < 1 || host->max_bonds > KID_MAX_BONDS) { h->err = "max_bonds out of range"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  int rc = mts_ensure(h, host->max_bonds);
  if (rc) return rc;
  const size_t n = (size_t)h->n, cap = (size_t)h->capacity;
  const int mb = h->mb;
  // connect_all_bonds (FW:4963-5125): rows of the bond partners, from the ids
  std::vector<int64_t> ids(n);
  std::vector<int32_t> alive(n);
  KID_HIP(h, hipMemcpy(ids.data(), h->bp.id, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  KID_HIP(h, hipMemcpy(alive.data(), h->bp.i[KID_BI_ALIVE], n * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::unordered_map<int64_t, int32_t> row_of;
  row_of.reserve(n * 2);
  for (size_t k = 0; k < n; ++k) if (alive[k]) row_of[ids[k]] = (int32_t)k;
  std::vector<int32_t> orow((size_t)mb * n, -1), oslot((size_t)mb * n, -1);
  for (size_t k = 0; k < n; ++k) {
    if (host->count[k] < 0 || host->count[k] > mb) { h->err = "bond count exceeds max_bonds"; return KID_EINVAL; }
    for (int s = 0; s < host->count[k]; ++s) {
      auto it = row_of.find(host->other_id[(size_t)s * n + k]);
      if (it != row_of.end()) orow[(size_t)s * n + k] = it->second;
    }
  }
  for (size_t k = 0; k < n; ++k)
    for (int s = 0; s < host->count[k]; ++s) {
      const int32_t o = orow[(size_t)s * n + k];
      if (o < 0) continue;
      for (int t = 0; t < host->count[o]; ++t) if (host->other_id[(size_t)t * n + o] == ids[k]) { oslot[(size_t)s * n + k] = t; break; }
    }
  KID_HIP(h, hipMemcpyAsync(h->mts.bcount, host->count, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  for (int s = 0; s < mb; ++s) {
    KID_HIP(h, hipMemcpyAsync(h->mts.bother_id + s * cap, host->other_id + s * n, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    if (host->broken) KID_HIP(h, hipMemcpyAsync(h->mts.bbroken + s * cap, host->broken + s * n, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    else KID_HIP(h, hipMemsetAsync(h->mts.bbroken + s * cap, 0, n * sizeof(int32_t), h->stream));
    KID_HIP(h, hipMemcpyAsync(h->mts.bother_row + s * cap, orow.data() + s * n, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    KID_HIP(h, hipMemcpyAsync(h->mts.bother_slot + s * cap, oslot.data() + s * n, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    for (int f = 0; f < KID_NBOND_F64; ++f) {
      if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(h->mts.bf[f] + s * cap, host->f64[f] + s * n, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      else KID_HIP(h, hipMemsetAsync(h->mts.bf[f] + s * cap, 0, n * sizeof(double), h->stream));
    }
  }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->have_bonds = true;
  h->visited = false;
  return KID_OK;
}

int kid_download_bonds(kid_handle *h, kid_bond_soa *host) {
  if (!h || !host) return KID_EINVAL;
  if (!h->have_bonds) { h->err = "no bonds were uploaded"; return KID_EINVAL; }
  if (host->n < h->n || host->max_bonds != h->mb) { h->err = "host bond SoA has the wrong shape"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)host->n, nn = (size_t)h->n, cap = (size_t)h->capacity;
  if (host->count) KID_HIP(h, hipMemcpyAsync(host->count, h->mts.bcount, nn * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  for (int s = 0; s < h->mb; ++s) {
    if (host->other_id) KID_HIP(h, hipMemcpyAsync(host->other_id + s * n, h->mts.bother_id + s * cap, nn * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (host->broken) KID_HIP(h, hipMemcpyAsync(host->broken + s * n, h->mts.bbroken + s * cap, nn * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    for (int f = 0; f < KID_NBOND_F64; ++f)
      if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(host->f64[f] + s * n, h->mts.bf[f] + s * cap, nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

// lanes of the fused sub-step kernel that gave up polling (d_order_flag[2]): that step is incomplete and the caller must know
static int mts_report_timeout(kid_handle *h, int lanes) {
  (void)hipMemsetAsync(h->d_order_flag + 2, 0, sizeof(int), h->stream);
  h->err = "the fused MTS sub-step kernel timed out: " + std::to_string(lanes) + " lanes never saw their neighbours' records (the grid was not co-resident?); "
           "the step it belongs to is incomplete (rows hold the state of the last sub-step each berg finished)";
  return KID_EHIP;
}
static int mts_check_timeout(kid_handle *h) {   // (after a stream synchronisation: one 4-byte read)
  if (!h->mts_ready || !h->d_order_flag || !h->fused_ran) return KID_OK;
  int lanes = 0;
  KID_HIP(h, hipMemcpyAsync(&lanes, h->d_order_flag + 2, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->fused_ran = false;
  return lanes > 0 ? mts_report_timeout(h, lanes) : KID_OK;
}
// traversal order of the reference (cells j-outer/i-inner, `inorder` inside a cell): LSD radix passes
static int mts_build_order(kid_handle *h) {
  const long long n = h->n;
  if (n == 0) { h->mts.nperm = 0; return KID_OK; }
  // the key kernels below read the device copy of the berg table: on a handle's first step nothing has written it yet when
  // kid_set_conglom_ids or the prologue come here before their mts_refresh (single-time-step scheme with contact)
  { const int rc_t = refresh_tables(h); if (rc_t) return rc_t; }
  int cur = 0;
  // The five `inorder` keys (start_lat, start_lon, start_mass, start_day, start_year) never change while bonds exist
  // (rows do not move, nothing re-stamps a bonded berg), only the cell does: the order by those five is built once per
  // upload (five stable passes) and every step adds the one stable pass by cell on top of it.
  // Rows keep their cell for many steps at a time (bonded elements move a fraction of a cell per step), and then the order,
  // the ranks and the cell table of the last call still hold: one comparison of every row's cell key with the key it was
  // sorted by stands in for the sort (the host needs nperm from the device either way: same one synchronisation).
  // The same question is asked of what the conglomerate labelling reads (alive, the bond lists, the bond counts: one
  // signature per berg): while neither the order nor those change, kid_set_conglom_ids has nothing to redo (labels_stale).
  if (h->d_static_rows && h->static_rows_n == n && h->order_n == n && h->mts_shadow_valid) {
    int changed[3] = {0, 0, 0};
    KID_HIP(h, hipMemsetAsync(h->d_order_flag, 0, 2 * sizeof(int), h->stream));
    hipLaunchKernelGGL(mts_key_check_kernel, MTS_GRID(n), dev_grid(h), (const BergPtrs *)h->d_bp, (const unsigned long long *)h->d_last_key, h->d_order_flag, n);
    hipLaunchKernelGGL(bond_signature_kernel, MTS_GRID(n), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, h->d_bond_sig, h->d_order_flag + 1, n);
    KID_HIP(h, hipMemcpyAsync(changed, h->d_order_flag, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    h->fused_ran = false;
    if (changed[2] > 0) return mts_report_timeout(h, changed[2]);
    if (changed[0] || changed[1]) h->labels_stale = true;
    if (!changed[0]) return KID_OK;
  }
  { const int rc_t = mts_check_timeout(h); if (rc_t) return rc_t; }
  h->labels_stale = true;
  h->order_n = -1;
  if (!h->d_static_rows || h->static_rows_n != n) {
    if (h->static_rows_cap < n) KID_HIP(h, h->mem.drop(h->d_static_rows));
    if (!h->d_static_rows) { KID_HIP(h, h->mem.dev(h->d_static_rows, (size_t)h->capacity)); h->static_rows_cap = h->capacity; }
    hipLaunchKernelGGL(mts_iota_kernel, MTS_GRID(n), h->d_rows[cur], n);
    const int f64_keys[4] = {KID_B_START_LAT, KID_B_START_LON, KID_B_START_MASS, KID_B_START_DAY};
    for (int pass = 0; pass < 5; ++pass) {
      if (pass < 4) hipLaunchKernelGGL(mts_key_f64_kernel, MTS_GRID(n), (const double *)h->bp.f[f64_keys[pass]], (const int *)h->d_rows[cur], h->d_key64[0], n);
      else hipLaunchKernelGGL(mts_key_i32_kernel, MTS_GRID(n), (const int32_t *)h->bp.i[KID_BI_START_YEAR], (const int *)h->d_rows[cur], h->d_key64[0], n);
      size_t bytes = h->mts_tmp.bytes;
      KID_HIP(h, rocprim::radix_sort_pairs(h->mts_tmp.p, bytes, h->d_key64[0], h->d_key64[1], h->d_rows[cur], h->d_rows[cur ^ 1], (size_t)n, 0, 64, h->stream));
      cur ^= 1;
    }
    KID_HIP(h, hipMemcpyAsync(h->d_static_rows, h->d_rows[cur], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    h->static_rows_n = n;
  }
  cur = 0;
  KID_HIP(h, hipMemcpyAsync(h->d_rows[cur], h->d_static_rows, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  {
    hipLaunchKernelGGL(mts_key_cell_kernel, MTS_GRID(n), dev_grid(h), (const BergPtrs *)h->d_bp, (const int *)h->d_rows[cur], h->d_key64[0], h->d_last_key, n);
    size_t bytes = h->mts_tmp.bytes;
    KID_HIP(h, rocprim::radix_sort_pairs(h->mts_tmp.p, bytes, h->d_key64[0], h->d_key64[1], h->d_rows[cur], h->d_rows[cur ^ 1], (size_t)n, 0, 64, h->stream));
    cur ^= 1;
  }
  KID_HIP(h, hipMemcpyAsync(h->mts.order, h->d_rows[cur], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  hipLaunchKernelGGL(mts_rank_kernel, MTS_GRID(n), (const int *)h->mts.order, (const unsigned long long *)h->d_key64[1], h->mts.rank, h->mts.cell_start, n, (int)h->ncell);
  KID_HIP(h, hipGetLastError());
  int32_t nperm = 0;
  KID_HIP(h, hipMemcpyAsync(&nperm, h->mts.cell_start + h->ncell, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->mts.nperm = nperm;
  h->order_n = n;
  return KID_OK;
}

static int mts_read_red(kid_handle *h, double *red) {
  KID_HIP(h, hipMemcpyAsync(red, h->mts.red, MR_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}
static int mts_zero_red(kid_handle *h, int first, int count) {
  KID_HIP(h, hipMemsetAsync(h->mts.red + first, 0, (size_t)count * sizeof(double), h->stream));
  return KID_OK;
}

// break_bonds_dem (FW:4713-4799); only_if_detected: guarded on the device by bond_break_detected
static int mts_break_bonds(kid_handle *h, int only_if_detected) {
  const long long n = h->n;
  if (!h->have_bonds || n == 0) return KID_OK;
  if (!h->params.fracture_criterion_stress) {
    if (h->params.frac_thres_n <= 0. && h->params.frac_thres_t <= 0.) return KID_OK;
    h->err = "break_bonds_dem: fracture criterion not supported for DEM (FW:4746)"; return KID_EINVAL;
  }
  hipLaunchKernelGGL(break_mark_kernel, MTS_GRID(n), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n, only_if_detected);
  hipLaunchKernelGGL(bond_delete_kernel, MTS_GRID(n), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n, only_if_detected, 1);
  hipLaunchKernelGGL(bond_slots_kernel, MTS_GRID(n), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}

// set_conglom_ids (FW:2601-2646), i.e. what transfer_mts_bergs (FW:2136-2216) leaves when whole conglomerates are resident
int kid_set_conglom_ids(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  int rc = mts_ensure_default(h);
  if (rc) return rc;
  const long long n = h->n;
  if (n == 0) return KID_OK;
  rc = mts_build_order(h);
  if (rc) return rc;
  rc = mts_refresh(h);
  if (rc) return rc;
  const BergPtrs *bt = h->d_bp; const MtsDev *mt = h->d_mts; const kid_params *pp = h->d_params;
  // nothing the labelling reads has changed since it last ran (mts_build_order has just asked): the ids, and the bond lists
  // pruned with them, are what they would come out as again
  if (!h->labels_stale && !h->dbg.mts_always_label) return KID_OK;
  hipLaunchKernelGGL(conglom_init_kernel, MTS_GRID(n), bt, mt, n);
  // Sweeps until one changes nothing.  Asking the device costs a stream synchronisation (~30 us, against ~5 us for a sweep
  // of a conglomerate that has already converged), so the first batch is as long as the whole iteration was the last time
  // and only its last four sweeps are watched; from then on batches of four.
  {
    int launched = 0, batch = std::max(8, std::min(h->conglom_batch, 4096));
    for (int round = 0; round < 4096; ++round) {
      for (int q = 0; q < batch - 4; ++q) hipLaunchKernelGGL(conglom_propagate_kernel, MTS_GRID(n), pp, bt, mt, n);
      rc = mts_zero_red(h, MR_CHANGED, 1);
      if (rc) return rc;
      for (int q = 0; q < 4; ++q) hipLaunchKernelGGL(conglom_propagate_kernel, MTS_GRID(n), pp, bt, mt, n);
      launched += batch;
      double red[MR_COUNT];
      rc = mts_read_red(h, red);
      if (rc) return rc;
      if (red[MR_CHANGED] == 0.) break;
      batch = 4;
    }
    h->conglom_batch = launched;
  }
  KID_HIP(h, hipMemsetAsync(h->mts.root_flag, 0, (size_t)n * sizeof(int32_t), h->stream));
  hipLaunchKernelGGL(conglom_roots_kernel, MTS_GRID(n), bt, mt, n);
  size_t bytes = h->mts_tmp.bytes;
  KID_HIP(h, rocprim::exclusive_scan(h->mts_tmp.p, bytes, h->mts.root_flag, h->mts.root_scan, 0, (size_t)n, rocprim::plus<int>(), h->stream));
  hipLaunchKernelGGL(conglom_assign_kernel, MTS_GRID(n), bt, mt, n);
  if (h->params.use_broken_bonds_for_substep_contact && h->have_bonds) {
    hipLaunchKernelGGL(conglom_prune_kernel, MTS_GRID(n), pp, bt, mt, n);
    hipLaunchKernelGGL(bond_delete_kernel, MTS_GRID(n), bt, mt, n, 0, 0);
    hipLaunchKernelGGL(bond_slots_kernel, MTS_GRID(n), bt, mt, n);
  }
  // the labelling itself may have pruned bonds: take the signatures of the result, so that the next call compares with it
  KID_HIP(h, hipMemsetAsync(h->d_order_flag, 0, 2 * sizeof(int), h->stream));
  hipLaunchKernelGGL(bond_signature_kernel, MTS_GRID(n), bt, mt, h->d_bond_sig, h->d_order_flag + 1, n);
  h->labels_stale = false;
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}


// what kid_evolve_icebergs_mts and kid_evolve_icebergs_interactive do before their sweeps, when there are bergs
static int mts_prologue(kid_handle *h) {
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  int rc = mts_ensure_default(h);
  if (rc) return rc;
  if (h->params.iceberg_bonds_on && !h->have_bonds) { h->err = "iceberg_bonds_on but no bonds were uploaded (kid_upload_bonds)"; return KID_EINVAL; }
  if (h->n == 0) return KID_OK;
  rc = mts_build_order(h);
  if (rc) return rc;
  rc = mts_refresh(h);
  if (rc) return rc;
  hipLaunchKernelGGL(cell_conglom_kernel, dim3((unsigned)((h->ncell + 255) / 256)), dim3(256), 0, h->stream, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, (int)h->ncell);
  return KID_OK;
}
// the convergence test of the implicit iterations of PART 1 and PART 3; usum: the norm of the previous iterate
static bool mts_converged(const kid_params &p, double usum, const double *red) {
  const double denom = sqrt(usum) + sqrt(red[MR_USUM1]);
  const double normchange = denom > 0 ? 2.0 * sqrt(red[MR_USUM2]) / denom : 0.0;
  return normchange < p.convergence_tolerance;
}
// sub-steps first..last of PART 3 (IB:6788-7050) as plain launches, from after the position update of sub-step `first`
static int mts_plain_substeps(kid_handle *h, int first, int last, bool pair_pass, bool inner_iterates, bool break_each) {
  const DevGrid g = dev_grid(h);
  const BergPtrs *bt = h->d_bp; const MtsDev *mt = h->d_mts; const kid_params *pp = h->d_params;
  const long long n = h->n;
  int rc;
  for (int sub = first; sub <= last; ++sub) {
    if (break_each) { rc = mts_zero_red(h, MR_BREAK, 1); if (rc) return rc; }
    if (!inner_iterates) {
      if (pair_pass) hipLaunchKernelGGL(bond_pass_kernel, MTS_GRID(n * h->mb), g, pp, bt, mt, n, h->mts.mts_fast_dt);
      hipLaunchKernelGGL(mts_velocity_kernel, MTS_GRID(n), g, pp, bt, mt, n, 1);
    } else {
      double usum = 0., red[MR_COUNT];
      rc = mts_zero_red(h, MR_USUM, 3);
      if (rc) return rc;
      for (int jj = 1;; ++jj) {   // until converged (the iterate that converges is the last one), or 1001 iterations
        hipLaunchKernelGGL(mts_velocity_kernel, MTS_GRID(n), g, pp, bt, mt, n, jj);
        rc = mts_read_red(h, red);
        if (rc) return rc;
        if (jj == 1) usum = red[MR_USUM];
        if ((jj > 1 && mts_converged(h->params, usum, red)) || jj > 1000) break;
        usum = red[MR_USUM1];
        hipLaunchKernelGGL(mts_inner_retry_kernel, MTS_GRID(n), bt, mt, n);
        rc = mts_zero_red(h, MR_USUM1, 2);
        if (rc) return rc;
      }
    }
    if (break_each) { rc = mts_break_bonds(h, 1); if (rc) return rc; }
    if (sub < h->params.mts_sub_steps) hipLaunchKernelGGL((mts_substep_own_kernel<true, true>), MTS_GRID(n), g, pp, bt, mt, n);
    else hipLaunchKernelGGL((mts_substep_own_kernel<true, false>), MTS_GRID(n), g, pp, bt, mt, n);
  }
  return KID_OK;
}

// The whole sub-step loop as one cooperative launch of mts_substeps_kernel, from after the position update of the first
// sub-step; `enqueued` stays false when not all the bergs' lanes would be co-resident.  A launch the runtime refuses halves
// the estimate for the next step and this step takes the plain launches.
static int mts_fused_substeps(kid_handle *h, bool &enqueued) {
  const long long n = h->n;
  const bool g4 = h->mb <= 4;
  const void *fn = g4 ? (const void *)mts_substeps_kernel<4> : (const void *)mts_substeps_kernel<8>;
  int &fused_blocks = h->fused_blocks[g4 ? 0 : 1];   // (per kernel variant: <4> and <8> differ in registers, i.e. in occupancy)
  if (fused_blocks == 0) {   // how many workgroups are co-resident (the cooperative launch checks it again)
    int per_cu = 0, ncu = 0;
    KID_HIP(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, MTS_FUSED_BS, 0));
    KID_HIP(h, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
    fused_blocks = std::max(1, std::min(per_cu, 4)) * std::max(1, ncu);
    if (h->dbg.mts_fused_blocks_cap > 0) fused_blocks = std::min(fused_blocks, h->dbg.mts_fused_blocks_cap);
  }
  const long long need_blocks = (n + MTS_FUSED_BS - 1) / MTS_FUSED_BS;
  if (need_blocks > (long long)fused_blocks) return KID_OK;   // one lane per berg, all co-resident; a bigger population fills the chip with the three-launch graph
  enqueued = true;
  KID_HIP(h, hipMemsetD32Async((hipDeviceptr_t)h->mts.rec, (int)0xfff7c0deu, (size_t)3 * 16 * (size_t)n, h->stream));   // every record of the three copies: not yet written
  DevGrid g_arg = dev_grid(h); const kid_params *pp_arg = h->d_params; const BergPtrs *bt_arg = h->d_bp; const MtsDev *mt_arg = h->d_mts;
  long long n_arg = n; int nsub_arg = h->params.mts_sub_steps;
  int poll_arg = h->dbg.mts_poll_limit > 0 ? h->dbg.mts_poll_limit : (int)MTS_POLL_LIMIT; int *to_arg = h->d_order_flag + 2;
  void *args[] = {&g_arg, &pp_arg, &bt_arg, &mt_arg, &n_arg, &nsub_arg, &poll_arg, &to_arg};
  const hipError_t e = hipLaunchCooperativeKernel(fn, dim3((unsigned)need_blocks), dim3(MTS_FUSED_BS), args, 0, h->stream);
  if (e == hipSuccess) { h->fused_ran = true; h->fused_launches++; return KID_OK; }
  if (e != hipErrorCooperativeLaunchTooLarge) { h->err = std::string("hipLaunchCooperativeKernel: ") + hipGetErrorString(e); return KID_EHIP; }
  (void)hipGetLastError();
  fused_blocks = std::max(1, fused_blocks / 2);
  return mts_plain_substeps(h, 1, h->params.mts_sub_steps, true, false, false);
}

// How many times has the sub-step loop of this handle gone out as the one cooperative launch (mts_substeps_kernel) so far?  A hook
// for tests/test_dem_rows_gpu.py, not part of include/kid.h: a case about the fused loop must not pass on the three-launch fall-back.
int kid_mts_fused_launches(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  *count = h->fused_launches;
  return KID_OK;
}

// evolve_icebergs_mts (IB:6576-7078)
int kid_evolve_icebergs_mts(kid_handle *h) {
  if (!h) return KID_EINVAL;
  if (!h->params.mts) { h->err = "kid_evolve_icebergs_mts needs mts=T"; return KID_EINVAL; }
  int rc = mts_prologue(h);
  if (rc || h->n == 0) return rc;
  h->zs.launched_other();   // (writes axn, ayn of any row)
  const kid_params &p = h->params;
  const long long n = h->n;
  const DevGrid g = dev_grid(h);
  const BergPtrs *bt = h->d_bp; const MtsDev *mt = h->d_mts; const kid_params *pp = h->d_params;
  rc = mts_zero_red(h, 0, MR_COUNT);
  if (rc) return rc;
  double red[MR_COUNT];
  // PART 1
  {
    int ii = 0; bool finished = false, had_collision = false, last_iter = !p.force_convergence;
    double usum = 0.;
    while (!finished) {
      ++ii;
      hipLaunchKernelGGL(mts_part1_kernel, MTS_GRID(n), g, pp, bt, mt, n, ii);
      if (p.force_convergence) {
        hipLaunchKernelGGL(mts_part1_old_kernel, MTS_GRID(n), bt, n, last_iter ? 1 : 0);
        rc = mts_read_red(h, red);
        if (rc) return rc;
        if (ii == 1) usum = red[MR_USUM];
        had_collision = had_collision || red[MR_COLLISION] != 0.;
      }
      if (p.force_convergence && !last_iter && had_collision) {
        if (ii > 1 && mts_converged(p, usum, red)) last_iter = true;
        usum = red[MR_USUM1];
      } else finished = true;
      if (last_iter) finished = true;
      if (ii > 1000) finished = true;
      if (!finished) { rc = mts_zero_red(h, MR_USUM1, 2); if (rc) return rc; }
    }
  }
  if (p.dem && !p.break_bonds_on_sub_steps) { rc = mts_break_bonds(h, 0); if (rc) return rc; }
  // PART 2
  hipLaunchKernelGGL(mts_part2_kernel, MTS_GRID(n), pp, bt, n);
  // PART 3
  const bool pair_pass = p.explicit_inner_mts && p.dem && p.iceberg_bonds_on;
  const bool inner_iterates = p.force_convergence && !p.explicit_inner_mts;
  const bool break_each = p.dem && !p.use_broken_bonds_for_substep_contact && p.break_bonds_on_sub_steps;
  // The common configuration (explicit inner steps, no host decision inside the loop) is 3 short launches per sub-step,
  // 90-200 sub-steps per step: captured once into a hipGraph and replayed, so the loop is not bound by launch calls.
  const bool graphable = !inner_iterates && !break_each && h->use_graph;
  hipLaunchKernelGGL((mts_substep_own_kernel<false, true>), MTS_GRID(n), g, pp, bt, mt, n);   // position update of the first sub-step
  // The DEM configuration of the tests and of config 4 (explicit inner steps, DEM bonds, broken bonds as the only sub-step
  // contacts): the whole loop is one cooperative launch (mts_substeps_kernel); everything else replays the captured graph.
  bool fused = false;
  if (graphable && pair_pass && p.use_broken_bonds_for_substep_contact && p.mts_sub_steps >= 1 && h->mb <= 8 && !h->dbg.mts_no_fused) {
    rc = mts_fused_substeps(h, fused);
    if (rc) return rc;
  }
  int first = 1;   // the sub-steps from `first` on are plain launches
  if (!fused && graphable && p.mts_sub_steps > 1) {
    // [pair pass, velocity sweep, own] x (N-1) in graphs of at most MTS_GRAPH_UNITS units, the rest plainly (the beam tests
    // run 1e5 sub-steps per step: one graph of 3e5 nodes is not a reasonable thing to instantiate)
    enum { MTS_GRAPH_UNITS = 2048 };
    const int units = p.mts_sub_steps - 1, per_graph = std::min(units, (int)MTS_GRAPH_UNITS);
    const bool stale = !h->sub_graph_exec || h->sub_graph_n != n || h->sub_graph_steps != per_graph || h->sub_graph_pair != pair_pass ||
                       h->sub_graph_dt != h->mts.mts_fast_dt || h->sub_graph_stream != h->stream;
    if (stale) {
      if (h->sub_graph_exec) { (void)hipGraphExecDestroy(h->sub_graph_exec); h->sub_graph_exec = nullptr; }
      hipGraph_t graph = nullptr;
      KID_HIP(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
      rc = mts_plain_substeps(h, 1, per_graph, pair_pass, false, false);
      if (rc) return rc;
      KID_HIP(h, hipStreamEndCapture(h->stream, &graph));
      KID_HIP(h, hipGraphInstantiate(&h->sub_graph_exec, graph, nullptr, nullptr, 0));
      (void)hipGraphDestroy(graph);
      h->sub_graph_n = n; h->sub_graph_steps = per_graph; h->sub_graph_pair = pair_pass; h->sub_graph_dt = h->mts.mts_fast_dt;
      h->sub_graph_stream = h->stream;
    }
    for (int q = 0; q < units / per_graph; ++q) KID_HIP(h, hipGraphLaunch(h->sub_graph_exec, h->stream));
    first += units / per_graph * per_graph;
  }
  if (!fused) {
    rc = mts_plain_substeps(h, first, p.mts_sub_steps, pair_pass, inner_iterates, break_each);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mts_adjust_kernel, MTS_GRID(n), g, pp, bt, mt, n);
  KID_HIP(h, hipGetLastError());
  return mts_fold_scalars(h);
}

// first visit after an upload: the `Visited` block of icebergs_run (IB:5409-5420)
static int mts_first_visit(kid_handle *h) {
  int rc = kid_interp_gridded_fields_to_bergs(h);
  if (rc) return rc;
  rc = kid_set_conglom_ids(h);
  if (rc) return rc;
  if (h->params.iceberg_bonds_on && h->have_bonds && h->n > 0) {
    hipLaunchKernelGGL(bond_length_kernel, MTS_GRID(h->n), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, (long long)h->n);
    KID_HIP(h, hipGetLastError());
  }
  h->visited = true;
  return KID_OK;
}

static int mts_fold_scalars(kid_handle *h) {
  hipLaunchKernelGGL(mts_fold_kernel, dim3(1), dim3(64), 0, h->stream, (const MtsDev *)h->d_mts, h->d_acc - KID_NSCALAR);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
// quadratic ocean depth at the bergs (IB:4894), after the environment interpolation
static int mts_depth(kid_handle *h) {
  int rc = mts_ensure_default(h);
  if (rc) return rc;
  if (h->n == 0) return KID_OK;
  if (h->mts_dirty || h->tables_dirty) { rc = mts_refresh(h); if (rc) return rc; }
  hipLaunchKernelGGL(mts_depth_kernel, MTS_GRID(h->n), dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, (long long)h->n);
  KID_HIP(h, hipGetLastError());
  return mts_fold_scalars(h);
}

// evolve_icebergs with interacting bergs under the single-time-step scheme (IB:7081-7200): two sweeps
int kid_evolve_icebergs_interactive(kid_handle *h) {
  if (!h) return KID_EINVAL;
  const kid_params &p = h->params;
  if (p.mts || !p.interactive_icebergs_on) { h->err = "kid_evolve_icebergs_interactive: needs interactive_icebergs_on and mts=F"; return KID_EINVAL; }
  int rc = mts_prologue(h);
  if (rc || h->n == 0) return rc;
  h->zs.launched_other();   // (writes axn, ayn of any row)
  const long long n = h->n;
  const DevGrid g = dev_grid(h);
  if (p.Runge_not_Verlet) {
    hipLaunchKernelGGL(sts_ia_rk4_kernel, MTS_GRID(n), g, (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n);
    hipLaunchKernelGGL(sts_ia_rk4_old_kernel, MTS_GRID(n), g, (const BergPtrs *)h->d_bp, n);
  } else {
    hipLaunchKernelGGL(sts_ia_velocity_kernel, MTS_GRID(n), g, (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n);
    hipLaunchKernelGGL(sts_ia_position_kernel, MTS_GRID(n), g, (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, n);
  }
  KID_HIP(h, hipGetLastError());
  h->halo_rows_live = false;   // the second sweep has retired them
  return mts_fold_scalars(h);
}
// adjust_fl_berg_interactivity (IB:2765-2841, called at IB:5486): footloose children (fl_k = -1) out of everybody's contact
// range become interactive (fl_k = -2).  The cell tables it walks are those of the contact searches; rows appended since they
// were built -- the children of this step's kid_footloose_calving -- are sorted in first, as candidates and as partners.
int kid_adjust_fl_berg_interactivity(kid_handle *h, int64_t *promoted) {
  if (!h) return KID_EINVAL;
  if (promoted) *promoted = 0;
  { const int rc_h = halo_rows_refuse(h, "kid_adjust_fl_berg_interactivity"); if (rc_h) return rc_h; }
  const kid_params &p = h->params;
  if (!p.footloose || !p.interactive_icebergs_on || p.mts || h->n == 0) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  int rc = mts_ensure_default(h);
  if (!rc) rc = mts_build_order(h);   // (its own question -- has a row changed its cell, died, or been appended? -- decides whether anything is sorted)
  if (!rc) rc = mts_refresh(h);
  if (rc) return rc;
  if (promoted) {
    if (!h->d_fl_promoted) KID_HIP(h, h->mem.dev(h->d_fl_promoted, 1));
    KID_HIP(h, hipMemsetAsync(h->d_fl_promoted, 0, sizeof(int), h->stream));
  }
  hipLaunchKernelGGL(fl_adjust_interactivity_kernel, MTS_GRID(h->n), dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp,
                     (const MtsDev *)h->d_mts, (long long)h->n, promoted ? h->d_fl_promoted : nullptr);
  KID_HIP(h, hipGetLastError());
  if (promoted) {
    int count = 0;
    KID_HIP(h, hipMemcpyAsync(&count, h->d_fl_promoted, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    *promoted = (int64_t)count;
  }
  return KID_OK;
}
// the `Visited` block for interacting bergs without MTS (IB:5415-5418)
static int sts_ia_first_visit(kid_handle *h) {
  const kid_params &p = h->params;
  int rc = KID_OK;
  if ((p.contact_distance > 0.) || (p.contact_spring_coef != p.spring_coef)) { rc = kid_set_conglom_ids(h); if (rc) return rc; }
  if (p.iceberg_bonds_on && h->have_bonds && h->n > 0) {
    rc = mts_ensure(h, h->mb); if (rc) return rc;
    rc = mts_refresh(h); if (rc) return rc;
    hipLaunchKernelGGL(bond_length_kernel, MTS_GRID(h->n), (const BergPtrs *)h->d_bp, (const MtsDev *)h->d_mts, (long long)h->n);
    KID_HIP(h, hipGetLastError());
  }
  h->visited = true;
  return KID_OK;
}

// hexagon orientation of every berg from its bonds, right before the mass spreading (IB:4003-4004)
static int bond_orientations(kid_handle *h) {
  const kid_params &p = h->params;
  const bool want = p.hexagonal_icebergs && p.iceberg_bonds_on && p.rotate_icebergs_for_mass_spreading && h->have_bonds && h->n > 0;
  if (!want) {
    if (h->bp.orient) { h->bp.orient = nullptr; h->tables_dirty = true; }
    return KID_OK;
  }
  if (!h->d_orient) KID_HIP(h, h->mem.dev(h->d_orient, (size_t)h->capacity));
  int rc = mts_ensure(h, h->mb);
  if (rc) return rc;
  if (h->bp.orient != h->d_orient) { h->bp.orient = h->d_orient; h->tables_dirty = true; }
  rc = mts_refresh(h);
  if (rc) return rc;
  hipLaunchKernelGGL(bond_orientation_kernel, MTS_GRID(h->n), dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp,
                     (const MtsDev *)h->d_mts, (long long)h->n, h->d_orient);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
