// nxs_thermo_forcing.inl -- host side of nxs_dyn_thermo_forcing_* (include/nxs_dyn.h; the kernels are in nxs_thermo_forcing_kernels.inl).  Textually included by
// nxs_dyn.hip inside its extern "C" block, behind nxs_slab.inl.  The pool is the ThermoForcing group (release_thermo_forcing, called by release_mesh): after
// nxs_dyn_set_mesh and nxs_dyn_regrid every snapshot and every target set is missing again.

static const char *const tf_name[TF_ROWS] = {"tair", "mslp", "Qsw_in", "humidity", "longwave", "precip", "snow", "ocean_temp", "ocean_salt", "mld"};

// the device row the launches read for forcing row k, and the mask that says it was given on this mesh
static double **tf_live_row(nxs_dyn_handle *h, int k) { return k < FLUX_ATM_ROWS ? &h->d_flux_atm[k] : &h->d_col_forcing[k - FLUX_ATM_ROWS]; }
static bool tf_live_have(const nxs_dyn_handle *h, int k) {
    return k < FLUX_ATM_ROWS ? (h->flux_atm_have >> k) & 1u : (h->col_forcing_have >> (k - FLUX_ATM_ROWS)) & 1u;
}
static_assert(FLUX_ATM_ROWS + COL_FORCING_ROWS == TF_ROWS, "nxs_dyn_flux_atmosphere + nxs_dyn_column_forcing are the ten rows");

// a buffer of the pool that grows with what is asked of it (the grid's axes and data); the smaller one is given back first
static int tf_reserve(nxs_dyn_handle *h, double **p, size_t *cap, size_t count) {
    if (*p && *cap >= count) return NXS_OK;
    if (*p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));   // (the last ingest may still read it)
        auto it = std::find(h->tf_allocs.begin(), h->tf_allocs.end(), (void *)*p);
        if (it != h->tf_allocs.end()) h->tf_allocs.erase(it);
        (void)hipFree(*p);
        *p = nullptr; *cap = 0;
    }
    if (int rc = dev_alloc(h, h->tf_allocs, p, count)) return rc;
    *cap = count;
    return NXS_OK;
}

int nxs_dyn_thermo_forcing_pair(nxs_dyn_handle *h, const nxs_dyn_thermo_forcing_rows *s0, const nxs_dyn_thermo_forcing_rows *s1) try {
    if (!h || !s0) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_pair before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne;
    const nxs_dyn_thermo_forcing_rows *snap[2] = {s0, s1};
    RowCopy rows[2 * TF_ROWS];
    int n = 0;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < TF_ROWS; ++k) {
            const double *src = snap[s] ? snap[s]->row[k] : nullptr;
            if (!src) continue;
            if (!h->tf_snap[s][k]) { if (int rc = dev_alloc(h, h->tf_allocs, &h->tf_snap[s][k], Ne)) return rc; }
            rows[n++] = RowCopy{h->tf_snap[s][k], src, Ne * sizeof(double), tf_name[k]};
        }
    if (int rc = copy_rows(h, rows, n, hipMemcpyHostToDevice)) return rc;
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < TF_ROWS; ++k) if (snap[s] && snap[s]->row[k]) h->tf_have[s] |= 1u << k;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_pair"); }

int nxs_dyn_thermo_forcing_time(nxs_dyn_handle *h, const struct nxs_dyn_thermo_forcing_time *t) try {   // ExternalData::get, externaldata.cpp:324-439
    if (!h || !t) return NXS_ERR_INVALID;
    for (int k = 0; k < TF_ROWS; ++k)
        if (t->mode[k] != NXS_TF_OFF && t->mode[k] != NXS_TF_LINEAR && t->mode[k] != NXS_TF_STEP)
            return fail(h, NXS_ERR_INVALID, "thermo_forcing_time: unknown mode %d of row %s", t->mode[k], tf_name[k]);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_time before set_mesh");
    for (int k = 0; k < TF_ROWS; ++k) {
        const unsigned bit = 1u << k;
        if (t->mode[k] == NXS_TF_LINEAR && !((h->tf_have[0] & bit) && (h->tf_have[1] & bit)))
            return fail(h, NXS_ERR_STATE, "thermo_forcing_time: row %s is LINEAR and a snapshot of it is missing on this mesh (present: 0x%x, 0x%x; nxs_dyn_thermo_forcing_pair / "
                                          "_ingest after set_mesh / regrid)", tf_name[k], h->tf_have[0], h->tf_have[1]);
        if (t->mode[k] == NXS_TF_STEP && !(h->tf_have[0] & bit))
            return fail(h, NXS_ERR_STATE, "thermo_forcing_time: row %s is STEP and its snapshot 0 is missing on this mesh (present: 0x%x)", tf_name[k], h->tf_have[0]);
    }
    HIPCHK(h, hipSetDevice(h->device));
    TfBlend b{};
    b.Ne = h->dm.Ne;
    for (int k = 0; k < TF_ROWS; ++k) {
        if (t->mode[k] == NXS_TF_OFF) continue;
        double **live = tf_live_row(h, k);   // (in the state pool like an uploaded row: made when first written)
        if (!*live) { if (int rc = dev_alloc(h, h->state_allocs, live, (size_t)h->dm.Ne)) return rc; }
        b.row[b.nrows++] = TfRow{h->tf_snap[0][k], t->mode[k] == NXS_TF_LINEAR ? h->tf_snap[1][k] : nullptr, *live, t->fcoeff0[k], t->fcoeff1[k], t->factor[k], t->bias[k], t->mode[k]};
    }
    if (b.nrows == 0) return NXS_OK;
    hipLaunchKernelGGL(k_thermo_forcing_blend, dim3(nblocks((b.Ne + 1) / 2), b.nrows), dim3(BLOCK), 0, h->stream, b);
    HIPCHK(h, hipGetLastError());
    for (int k = 0; k < TF_ROWS; ++k) {
        if (t->mode[k] == NXS_TF_OFF) continue;
        if (k < FLUX_ATM_ROWS) h->flux_atm_have |= 1u << k; else h->col_forcing_have |= 1u << (k - FLUX_ATM_ROWS);
    }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_time"); }

int nxs_dyn_thermo_forcing_targets(nxs_dyn_handle *h, int32_t set, const double *RX, const double *RY) try {
    if (!h || !RX || !RY) return NXS_ERR_INVALID;
    if (set < 0 || set >= TF_SETS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_targets: set = %d (0 .. %d)", set, TF_SETS - 1);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_targets before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne;
    if (!h->tf_rx[set]) {
        if (int rc = dev_alloc(h, h->tf_allocs, &h->tf_rx[set], Ne)) return rc;
        if (int rc = dev_alloc(h, h->tf_allocs, &h->tf_ry[set], Ne)) return rc;
    }
    h->tf_targets_have &= ~(1u << set);
    const RowCopy rows[2] = {{h->tf_rx[set], RX, Ne * sizeof(double), "RX"}, {h->tf_ry[set], RY, Ne * sizeof(double), "RY"}};
    if (int rc = copy_rows(h, rows, 2, hipMemcpyHostToDevice)) return rc;
    h->tf_targets_have |= 1u << set;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_targets"); }

int nxs_dyn_thermo_forcing_ingest(nxs_dyn_handle *h, int32_t set, const nxs_dyn_forcing_grid *g, const double *data, int32_t N_data, const int32_t *row,
                                  const int32_t *snapshot) try {   // loadDataset's InterpFromGridToMeshx, externaldata.cpp:1436
    if (!h || !g || !data || !row || !snapshot || !g->x_in || !g->y_in) return NXS_ERR_INVALID;
    if (set < 0 || set >= TF_SETS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: set = %d (0 .. %d)", set, TF_SETS - 1);
    const int M = g->M, N = g->N;
    if (M < 2 || N < 2) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: a %d x %d grid: nothing to be done", M, N);
    if (N_data < 1 || N_data > TF_MAX_COLUMNS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: N_data = %d (1 .. %d)", N_data, TF_MAX_COLUMNS);
    if (g->interp != NXS_INTERP_TRIANGLE && g->interp != NXS_INTERP_BILINEAR && g->interp != NXS_INTERP_NEAREST)
        return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: Interpolation %d not supported yet", g->interp);
    unsigned seen[2] = {0, 0};
    for (int j = 0; j < N_data; ++j) {
        if (row[j] == -1) continue;
        if (row[j] < 0 || row[j] >= TF_ROWS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: column %d goes to row %d (-1 .. %d)", j, row[j], TF_ROWS - 1);
        if (snapshot[j] != 0 && snapshot[j] != 1) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: column %d goes to snapshot %d (0 or 1)", j, snapshot[j]);
        if (seen[snapshot[j]] & (1u << row[j])) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: two columns go to snapshot %d of row %s", snapshot[j], tf_name[row[j]]);
        seen[snapshot[j]] |= 1u << row[j];
    }
    std::vector<double> x(N), y(M);
    if (!g2m_centres(g->x_in, g->x_rows, g->y_in, g->y_rows, M, N, x.data(), y.data()))
        return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest: x and y vectors length should be 1 or 0 more than data number of rows.");
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_ingest before set_mesh");
    if (!(h->tf_targets_have & (1u << set))) return fail(h, NXS_ERR_STATE, "thermo_forcing_ingest: set %d has no targets on this mesh (nxs_dyn_thermo_forcing_targets after set_mesh / regrid)", set);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne, cells = (size_t)M * N * N_data;
    if (int rc = tf_reserve(h, &h->tf_gx, &h->tf_gx_cap, N)) return rc;
    if (int rc = tf_reserve(h, &h->tf_gy, &h->tf_gy_cap, M)) return rc;
    if (int rc = tf_reserve(h, &h->tf_data, &h->tf_data_cap, cells)) return rc;
    TfIngest a{};
    a.g = G2M{h->tf_gx, h->tf_gy, N, M, M, N, N_data, (int)Ne, g->interp, g->row_major != 0, g2m_monotone(x.data(), N), g2m_monotone(y.data(), M), g->default_value};
    a.rx = h->tf_rx[set]; a.ry = h->tf_ry[set];
    for (int j = 0; j < N_data; ++j) {
        if (row[j] < 0) continue;
        double **dst = &h->tf_snap[snapshot[j]][row[j]];
        if (!*dst) { if (int rc = dev_alloc(h, h->tf_allocs, dst, Ne)) return rc; }
        a.dst[j] = *dst;
    }
    const RowCopy up[3] = {{h->tf_gx, x.data(), (size_t)N * sizeof(double), "x"}, {h->tf_gy, y.data(), (size_t)M * sizeof(double), "y"}, {h->tf_data, data, cells * sizeof(double), "data"}};
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (an earlier ingest may still read the grid buffers)
    for (int k = 0; k < 3; ++k) { if (k == 2) pin_host_buffer(h, up[k].src, up[k].bytes); HIPCHK(h, hipMemcpyAsync(up[k].dst, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream)); }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // x, y are this call's; data is free on return
    hipLaunchKernelGGL(k_thermo_forcing_ingest, dim3(nblocks((int)Ne)), dim3(BLOCK), 0, h->stream, a, (const double *)h->tf_data);
    HIPCHK(h, hipGetLastError());
    h->tf_have[0] |= seen[0]; h->tf_have[1] |= seen[1];
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_ingest"); }

int nxs_dyn_thermo_forcing_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_thermo_forcing_rows *out) try {
    if (!h || !out) return NXS_ERR_INVALID;
    if (which < 0 || which > 2) return fail(h, NXS_ERR_INVALID, "thermo_forcing_get: which = %d (0, 1: the snapshots; 2: the rows the launches read)", which);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_get before set_mesh");
    const double *dev[TF_ROWS];
    for (int k = 0; k < TF_ROWS; ++k) {
        const bool have = which == 2 ? tf_live_have(h, k) : ((h->tf_have[which] >> k) & 1u) != 0;
        if (out->row[k] && !have) return fail(h, NXS_ERR_STATE, "thermo_forcing_get: row %s of %s is missing on this mesh", tf_name[k], which == 2 ? "the launches' rows" : which ? "snapshot 1" : "snapshot 0");
        dev[k] = which == 2 ? *tf_live_row(h, k) : h->tf_snap[which][k];
    }
    HIPCHK(h, hipSetDevice(h->device));
    return download_rows(h, out->row, dev, TF_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_get"); }
