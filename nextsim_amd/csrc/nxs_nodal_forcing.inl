// nxs_nodal_forcing.inl -- host side of nxs_mapx_* and nxs_dyn_forcing_* / nxs_dyn_set_forcing_time_rows / nxs_dyn_set_element_depth (include/nxs_dyn.h; the
// kernels are in nxs_nodal_forcing_kernels.inl).  Textually included by nxs_dyn.hip inside its extern "C" block, behind nxs_nesting.inl.  The snapshots are the
// ForcingPair group's (release_forcing_pair); the targets and the uploaded grid are the NodalForcing group (release_nodal_forcing, called by release_mesh): after
// nxs_dyn_set_mesh and nxs_dyn_regrid every snapshot and every target set is missing again.

static const char *const nf_name[NF_ROWS] = {"wind_u", "wind_v", "ocean_u", "ocean_v", "ssh"};
static const char *const nf_group_name[NF_GROUPS] = {"wind", "ocean", "ssh"};
static const unsigned NF_ALL_HALF_ROWS = (1u << (2 * NF_ROWS)) - 1u;

// where half-row `row` of snapshot s lives in the ForcingPair group: f_snap = wind0, wind1, ocean0, ocean1, ssh0, ssh1; V at offset Nn
static double *nf_half_row(nxs_dyn_handle *h, int s, int row) { return h->f_snap[2 * (row >> 1) + s] + ((row & 1) && row < NXS_NF_SSH ? (size_t)h->dm.Nn : 0); }
static unsigned nf_bit(int s, int row) { return 1u << (s * NF_ROWS + row); }
// the six vectors, made together as nxs_dyn_set_forcing_pair makes them
static int nf_ensure_snapshots(nxs_dyn_handle *h) {
    if (h->f_snap[0]) return NXS_OK;
    const size_t Nn = h->dm.Nn;
    const size_t len[6] = {2 * Nn, 2 * Nn, 2 * Nn, 2 * Nn, Nn, Nn};
    for (int k = 0; k < 6; ++k) { if (int rc = dev_alloc(h, h->forcing_allocs, &h->f_snap[k], len[k])) return rc; }
    return NXS_OK;
}
// the step's forcing is complete: wind, ocean and ssh were written and the element depth is there
static void nf_forcing_given(nxs_dyn_handle *h) { if (h->have_depth && h->live_forcing == 7u) h->have_forcing = true; }

// a buffer of the pool that grows with what is asked of it (tf_reserve's rule)
static int nf_reserve(nxs_dyn_handle *h, double **p, size_t *cap, size_t count) {
    if (*p && *cap >= count) return NXS_OK;
    if (*p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));   // (the last ingest may still read it)
        auto it = std::find(h->nf_allocs.begin(), h->nf_allocs.end(), (void *)*p);
        if (it != h->nf_allocs.end()) h->nf_allocs.erase(it);
        (void)hipFree(*p);
        *p = nullptr; *cap = 0;
    }
    if (int rc = dev_alloc(h, h->nf_allocs, p, count)) return rc;
    *cap = count;
    return NXS_OK;
}

int nxs_mapx_constants(double *out, int32_t count) try {   // contrib/mapx/include/mapx.h:47, 55
    if (!out || count < 0) return NXS_ERR_INVALID;
    const double c[NXS_MAPX_CONST_COUNT] = {NXS_MAPX_RE_KM, NXS_MAPX_PI};
    for (int i = 0; i < count && i < NXS_MAPX_CONST_COUNT; ++i) out[i] = c[i];
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_mapx_constants"); }

int nxs_mapx_polar_north(double lat0, double lon0, double lat1, double rotation, double scale, double center_lat, double center_lon, double equatorial_radius,
                         double eccentricity, nxs_mapx_polar *out) try {
    if (!out) return NXS_ERR_INVALID;
    const double PI = NXS_MAPX_PI;
    if (lat1 == 999) lat1 = lat0;                                   // polar_stereographic.c:93
    if (lat0 != 90.00) return fail(nullptr, NXS_ERR_INVALID, "mapx_polar_north: lat0 = %7.2f (the north aspect only)", lat0);
    nxs_mapx_polar m{};
    m.lon0 = lon0; m.lat1 = lat1; m.scale = scale; m.eccentricity = eccentricity;
    m.false_easting = 0.0; m.false_northing = 0.0;                  // mapx.c:795-796
    const double e2 = (eccentricity) * (eccentricity);              // mapx.c:1011
    m.Rg = equatorial_radius / scale;                               // mapx.c:1029, polar_stereographic.c:99
    const double c1 = cos(lat1 * PI / 180);                   // :103-105
    const double s1 = sin(lat1 * PI / 180);
    m.m1 = ((c1) / sqrt(1 - (e2 * s1 * s1)));     // :115-116
    const double num = (1 - eccentricity * s1);         // :118-119
    const double den = (1 + eccentricity * s1);
    m.t1 = tan(PI / 4 - (lat1 * PI / 180) / 2) / pow(num / den, eccentricity / 2);   // :123-124
    const double theta = rotation * PI / 180;                       // mapx.c:1039-1044
    m.T00 = cos(theta);
    m.T01 = sin(theta);
    m.T10 = -sin(theta);
    m.T11 = cos(theta);
    double x0, y0;                                                  // mapx.c:1046-1054 (x0 is never given in an .mpp file of this form)
    nxs_mapx_polar_xy(m, center_lat, center_lon, &x0, &y0);
    m.u0 = m.T00 * x0 + m.T01 * y0;                                 // mapx.c:1061-1062
    m.v0 = m.T10 * x0 + m.T11 * y0;
    *out = m;
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_mapx_polar_north"); }

int nxs_mapx_forward(const nxs_mapx_polar *map, int64_t n, const double *lat, const double *lon, double *x, double *y, int32_t device) try {
    if (!map || !lat || !lon || !x || !y || n < 0) return NXS_ERR_INVALID;
    if (n == 0) return NXS_OK;
    if (device < 0) {
        for (int64_t i = 0; i < n; ++i) nxs_mapx_forward_point(*map, lat[i], lon[i], &x[i], &y[i]);
        return NXS_OK;
    }
    if (n > (int64_t)BLOCK * 0x7fffffffLL) return fail(nullptr, NXS_ERR_INVALID, "mapx_forward: n = %lld", (long long)n);
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, NXS_ERR_HIP, "mapx_forward: no device %d", (int)device); }
    const size_t bytes = (size_t)n * sizeof(double);
    double *d = nullptr;   // lat | lon | x | y
    if (hipMalloc((void **)&d, 4 * bytes) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, NXS_ERR_HIP, "mapx_forward: hipMalloc of %zu bytes", 4 * bytes); }
    hipError_t e = hipMemcpy(d, lat, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, lon, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_mapx_forward, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0, *map, (long long)n, (const double *)d, (const double *)(d + n), d + 2 * n, d + 3 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(x, d + 2 * n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(y, d + 3 * n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(nullptr, NXS_ERR_HIP, "mapx_forward: %s", hipGetErrorString(e));
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_mapx_forward"); }

int nxs_dyn_forcing_targets(nxs_dyn_handle *h, int32_t set, const double *RX, const double *RY) try {
    if (!h || !RX || !RY) return NXS_ERR_INVALID;
    if (set < 0 || set >= NF_SETS) return fail(h, NXS_ERR_INVALID, "forcing_targets: set = %d (0 .. %d)", set, NF_SETS - 1);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "forcing_targets before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Nn = h->dm.Nn;
    if (!h->nf_rx[set]) {
        if (int rc = dev_alloc(h, h->nf_allocs, &h->nf_rx[set], Nn)) return rc;
        if (int rc = dev_alloc(h, h->nf_allocs, &h->nf_ry[set], Nn)) return rc;
    }
    h->nf_targets_have &= ~(1u << set);
    const RowCopy rows[2] = {{h->nf_rx[set], RX, Nn * sizeof(double), "RX"}, {h->nf_ry[set], RY, Nn * sizeof(double), "RY"}};
    if (int rc = copy_rows(h, rows, 2, hipMemcpyHostToDevice)) return rc;
    h->nf_targets_have |= 1u << set;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_forcing_targets"); }

int nxs_dyn_forcing_ingest(nxs_dyn_handle *h, int32_t set, const nxs_dyn_forcing_grid *g, int32_t cyclic_x, int32_t cyclic_y, const double *data, int32_t N_data,
                           const int32_t *row, const int32_t *snapshot, const nxs_dyn_forcing_vectors *vec) try {   // loadDataset, externaldata.cpp:461-940
    if (!h || !g || !data || !row || !snapshot || !g->x_in || !g->y_in) return NXS_ERR_INVALID;
    if (set < 0 || set >= NF_SETS) return fail(h, NXS_ERR_INVALID, "forcing_ingest: set = %d (0 .. %d)", set, NF_SETS - 1);
    const int M = g->M, N = g->N;
    if (M < 2 || N < 2) return fail(h, NXS_ERR_INVALID, "forcing_ingest: a %d x %d grid: nothing to be done", M, N);
    if ((int64_t)(M + 1) * (N + 1) > 0x7fffffffLL) return fail(h, NXS_ERR_INVALID, "forcing_ingest: a %d x %d grid has more points than a launch indexes", M, N);
    if (N_data < 1 || N_data > NF_MAX_COLUMNS) return fail(h, NXS_ERR_INVALID, "forcing_ingest: N_data = %d (1 .. %d)", N_data, NF_MAX_COLUMNS);
    if (g->interp != NXS_INTERP_TRIANGLE && g->interp != NXS_INTERP_BILINEAR && g->interp != NXS_INTERP_NEAREST)
        return fail(h, NXS_ERR_INVALID, "forcing_ingest: Interpolation %d not supported yet", g->interp);
    unsigned seen = 0;
    for (int j = 0; j < N_data; ++j) {
        if (row[j] == -1) continue;
        if (row[j] < 0 || row[j] >= NF_ROWS) return fail(h, NXS_ERR_INVALID, "forcing_ingest: column %d goes to row %d (-1 .. %d)", j, row[j], NF_ROWS - 1);
        if (snapshot[j] != 0 && snapshot[j] != 1) return fail(h, NXS_ERR_INVALID, "forcing_ingest: column %d goes to snapshot %d (0 or 1)", j, snapshot[j]);
        if (seen & nf_bit(snapshot[j], row[j])) return fail(h, NXS_ERR_INVALID, "forcing_ingest: two columns go to snapshot %d of row %s", snapshot[j], nf_name[row[j]]);
        seen |= nf_bit(snapshot[j], row[j]);
    }
    const bool cx = cyclic_x != 0, cy = cyclic_y != 0;
    const int cN = N + (cx ? 1 : 0), cM = M + (cy ? 1 : 0);
    if ((cx || cy) && !(N == g->x_rows && M == g->y_rows)) return fail(h, NXS_ERR_INVALID, "forcing_ingest: with a cyclic axis only pixel centres are accepted");
    if ((cx || cy) && g->row_major) return fail(h, NXS_ERR_INVALID, "forcing_ingest: a cyclic axis needs data [M][N][N_data] (row_major == 0)");
    std::vector<double> x(cN), y(cM);
    if (!g2m_centres(g->x_in, g->x_rows, g->y_in, g->y_rows, M, N, x.data(), y.data()))
        return fail(h, NXS_ERR_INVALID, "forcing_ingest: x and y vectors length should be 1 or 0 more than data number of rows.");
    if (cx) x[N] = x[N - 1] + (x[N - 1] - x[N - 2]);   // externaldata.cpp:1322-1326
    if (cy) y[M] = y[M - 1] + (y[M - 1] - y[M - 2]);   // :1315-1319
    bool any_east_west = false;
    if (vec) {
        if (vec->n_pairs < 0 || vec->n_pairs > NF_MAX_VECTORS) return fail(h, NXS_ERR_INVALID, "forcing_ingest: %d vector pairs (0 .. %d)", vec->n_pairs, NF_MAX_VECTORS);
        if (vec->n_pairs > 0 && g->row_major) return fail(h, NXS_ERR_INVALID, "forcing_ingest: vectors need data [M][N][N_data] (row_major == 0)");
        unsigned long long named = 0;
        for (int k = 0; k < vec->n_pairs; ++k) {
            if (vec->is_wav_dir[k]) return fail(h, NXS_ERR_INVALID, "forcing_ingest: pair %d is a wave direction (wavDirOptions.isWavDir): that branch of transformData is not built", k);
            const int c[2] = {vec->component0[k], vec->component1[k]};
            for (int q = 0; q < 2; ++q) {
                if (c[q] < 0 || c[q] >= N_data) return fail(h, NXS_ERR_INVALID, "forcing_ingest: pair %d names column %d (0 .. %d)", k, c[q], N_data - 1);
                if (row[c[q]] < 0) return fail(h, NXS_ERR_INVALID, "forcing_ingest: pair %d names column %d, which is skipped", k, c[q]);
                if (named & (1ull << c[q])) return fail(h, NXS_ERR_INVALID, "forcing_ingest: column %d is named twice by the vector pairs", c[q]);
                named |= 1ull << c[q];
            }
            any_east_west = any_east_west || vec->east_west_oriented[k] != 0;
        }
        if (vec->n_pairs > 0 && !vec->rotate && vec->gridded_rotation_angle)
            return fail(h, NXS_ERR_INVALID, "forcing_ingest: grid.gridded_rotation_angle (the coupled build's gridTheta rotation) is not built");
        if (any_east_west && (!vec->lat || !vec->lon)) return fail(h, NXS_ERR_INVALID, "forcing_ingest: an east/north pair needs the grid's latitudes and longitudes");
    }
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "forcing_ingest before set_mesh");
    if (!(h->nf_targets_have & (1u << set))) return fail(h, NXS_ERR_STATE, "forcing_ingest: set %d has no targets on this mesh (nxs_dyn_forcing_targets after set_mesh / regrid)", set);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Nn = h->dm.Nn, cells = (size_t)cM * cN * N_data;
    if (int rc = nf_ensure_snapshots(h)) return rc;
    if (int rc = nf_reserve(h, &h->nf_gx, &h->nf_gx_cap, cN)) return rc;
    if (int rc = nf_reserve(h, &h->nf_gy, &h->nf_gy_cap, cM)) return rc;
    if (int rc = nf_reserve(h, &h->nf_data, &h->nf_data_cap, cells)) return rc;
    const size_t nlat = any_east_west ? (vec->latlon_per_point ? (size_t)M * N : (size_t)M) : 0, nlon = any_east_west ? (vec->latlon_per_point ? (size_t)M * N : (size_t)N) : 0;
    if (any_east_west) {
        if (int rc = nf_reserve(h, &h->nf_lat, &h->nf_lat_cap, nlat)) return rc;
        if (int rc = nf_reserve(h, &h->nf_lon, &h->nf_lon_cap, nlon)) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (an earlier ingest may still read the grid buffers)
    h->nf_grid_cells = 0;
    HIPCHK(h, hipMemcpyAsync(h->nf_gx, x.data(), (size_t)cN * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->nf_gy, y.data(), (size_t)cM * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (any_east_west) {
        HIPCHK(h, hipMemcpyAsync(h->nf_lat, vec->lat, nlat * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->nf_lon, vec->lon, nlon * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    const size_t row_bytes = (size_t)N * N_data * sizeof(double);
    pin_host_buffer(h, data, (size_t)M * row_bytes);
    if (cN == N) HIPCHK(h, hipMemcpyAsync(h->nf_data, data, (size_t)M * row_bytes, hipMemcpyHostToDevice, h->stream));   // (row_major too: the same bytes)
    else HIPCHK(h, hipMemcpy2DAsync(h->nf_data, (size_t)cN * N_data * sizeof(double), data, row_bytes, row_bytes, (size_t)M, hipMemcpyHostToDevice, h->stream));   // the wrap column stays free
    HIPCHK(h, hipStreamSynchronize(h->stream));   // x, y are this call's; data, lat, lon are free on return
    const NfGrid grid{h->nf_data, M, N, cM, cN, N_data};
    if (vec && vec->n_pairs > 0 && (any_east_west || vec->rotate)) {
        NfVectors a{};
        a.g = grid;
        a.npairs = vec->n_pairs;
        for (int k = 0; k < vec->n_pairs; ++k) { a.j0[k] = vec->component0[k]; a.j1[k] = vec->component1[k]; a.east_west[k] = vec->east_west_oriented[k] != 0; }
        a.lat = h->nf_lat; a.lon = h->nf_lon; a.per_point = vec->latlon_per_point != 0;
        a.pole_row = a.pole_next = -1;
        if (y[0] == 90.) { a.pole_row = 0; a.pole_next = 1; }             // externaldata.cpp:1210-1221: the last wins
        if (y[M - 1] == 90.) { a.pole_row = M - 1; a.pole_next = M - 2; }
        a.map = vec->map;
        a.R = NXS_MAPX_RE_KM * 1000.;                                     // externaldata.cpp:955
        a.c = vec->cos_m_diff_angle; a.s = vec->sin_m_diff_angle;
        const dim3 pts(nblocks(M * N), a.npairs);
        if (any_east_west) {
            hipLaunchKernelGGL(k_nf_east_north, pts, dim3(BLOCK), 0, h->stream, a);
            if (a.pole_row >= 0) hipLaunchKernelGGL(k_nf_pole, dim3(1), dim3(BLOCK), 0, h->stream, a);
        }
        if (vec->rotate) hipLaunchKernelGGL(k_nf_rotate, pts, dim3(BLOCK), 0, h->stream, a);
        HIPCHK(h, hipGetLastError());
    }
    if (cx || cy) {
        hipLaunchKernelGGL(k_nf_wrap, dim3(nblocks((cx ? M : 0) + (cy ? N : 0) + 1)), dim3(BLOCK), 0, h->stream, grid);
        HIPCHK(h, hipGetLastError());
    }
    NfIngest a{};
    a.g = G2M{h->nf_gx, h->nf_gy, cN, cM, cM, cN, N_data, (int)Nn, g->interp, g->row_major != 0, g2m_monotone(x.data(), cN), g2m_monotone(y.data(), cM), g->default_value};
    a.rx = h->nf_rx[set]; a.ry = h->nf_ry[set];
    for (int j = 0; j < N_data; ++j) if (row[j] >= 0) a.dst[j] = nf_half_row(h, snapshot[j], row[j]);
    hipLaunchKernelGGL(k_nf_ingest, dim3(nblocks((int)Nn)), dim3(BLOCK), 0, h->stream, a, (const double *)h->nf_data);
    HIPCHK(h, hipGetLastError());
    h->nf_grid_cells = cells;
    h->f_have |= seen;
    if (h->f_have == NF_ALL_HALF_ROWS) h->have_pair = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_forcing_ingest"); }

int nxs_dyn_set_forcing_time_rows(nxs_dyn_handle *h, const struct nxs_dyn_forcing_time_rows *t) try {   // ExternalData::get, externaldata.cpp:324-439
    if (!h || !t) return NXS_ERR_INVALID;
    for (int k = 0; k < NF_GROUPS; ++k)
        if (t->mode[k] != NXS_TF_OFF && t->mode[k] != NXS_TF_LINEAR && t->mode[k] != NXS_TF_STEP)
            return fail(h, NXS_ERR_INVALID, "set_forcing_time_rows: unknown mode %d of group %s", t->mode[k], nf_group_name[k]);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "set_forcing_time_rows before set_mesh");
    for (int k = 0; k < NF_GROUPS; ++k) {
        unsigned need0 = nf_bit(0, 2 * k), need1 = nf_bit(1, 2 * k);
        if (k < 2) { need0 |= nf_bit(0, 2 * k + 1); need1 |= nf_bit(1, 2 * k + 1); }
        if (t->mode[k] == NXS_TF_LINEAR && (h->f_have & (need0 | need1)) != (need0 | need1))
            return fail(h, NXS_ERR_STATE, "set_forcing_time_rows: group %s is LINEAR and a snapshot of it is missing on this mesh (present: 0x%x; nxs_dyn_set_forcing_pair / "
                                          "nxs_dyn_forcing_ingest after set_mesh / regrid)", nf_group_name[k], h->f_have);
        if (t->mode[k] == NXS_TF_STEP && (h->f_have & need0) != need0)
            return fail(h, NXS_ERR_STATE, "set_forcing_time_rows: group %s is STEP and its snapshot 0 is missing on this mesh (present: 0x%x)", nf_group_name[k], h->f_have);
    }
    HIPCHK(h, hipSetDevice(h->device));
    NfBlend b{};
    b.Nn = h->dm.Nn;
    double *const live[NF_GROUPS] = {h->ds.wind, h->ds.ocean, h->ds.ssh};
    for (int k = 0; k < NF_GROUPS; ++k) {
        if (t->mode[k] == NXS_TF_OFF) continue;
        b.grp[b.ngroups++] = NfGroup{h->f_snap[2 * k], t->mode[k] == NXS_TF_LINEAR ? h->f_snap[2 * k + 1] : nullptr, live[k], k < 2 ? 2 : 1, t->fcoeff0[k], t->fcoeff1[k], t->factor[k],
                                     t->bias[k], t->mode[k]};
    }
    if (b.ngroups == 0) return NXS_OK;
    hipLaunchKernelGGL(k_nf_blend, dim3(nblocks((b.Nn + 1) / 2), b.ngroups), dim3(BLOCK), 0, h->stream, b);
    HIPCHK(h, hipGetLastError());
    for (int k = 0; k < NF_GROUPS; ++k) if (t->mode[k] != NXS_TF_OFF) h->live_forcing |= 1u << k;
    nf_forcing_given(h);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_set_forcing_time_rows"); }

int nxs_dyn_set_element_depth(nxs_dyn_handle *h, const double *depth) try {
    if (!h || !depth) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "set_element_depth before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const RowCopy rows[1] = {{h->ds.depth, depth, (size_t)h->dm.Ne * sizeof(double), "element_depth"}};
    if (int rc = copy_rows(h, rows, 1, hipMemcpyHostToDevice)) return rc;
    h->have_depth = true;
    nf_forcing_given(h);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_set_element_depth"); }

int nxs_dyn_forcing_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_forcing_rows *out) try {
    if (!h || !out) return NXS_ERR_INVALID;
    if (which < 0 || which > 1) return fail(h, NXS_ERR_INVALID, "forcing_get: which = %d (0, 1: the snapshots)", which);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "forcing_get before set_mesh");
    RowCopy rows[NF_ROWS];
    int n = 0;
    for (int k = 0; k < NF_ROWS; ++k) {
        if (!out->row[k]) continue;
        if (!(h->f_have & nf_bit(which, k))) return fail(h, NXS_ERR_STATE, "forcing_get: row %s of snapshot %d is missing on this mesh", nf_name[k], which);
        rows[n++] = RowCopy{out->row[k], nf_half_row(h, which, k), (size_t)h->dm.Nn * sizeof(double), nf_name[k]};
    }
    HIPCHK(h, hipSetDevice(h->device));
    return copy_rows(h, rows, n, hipMemcpyDeviceToHost);
} catch (...) { return dyn_caught(h, "nxs_dyn_forcing_get"); }
