// nxs_means_regular.inl -- host side of nxs_dyn_means_regular_* (include/nxs_dyn.h): the Moorings means on the REGULAR grid -- GridOutput::updateGridMean() through
// the M_is_regular_grid branch of updateGridMeanWorker, setProcMask, setLSM / applyLSM, rotateVectors, resetGridMean (model/gridoutput.cpp:360-415, 486-538,
// 558-651) and the arithmetic of contrib/bamg/src/InterpFromMeshToGridx.cpp.  Textually included by nxs_dyn.hip inside its extern "C" block, behind
// nxs_means_points.inl.  The kernels are nxs_means_regular_kernels.inl, the arithmetic nxs_means_regular_body.inl.
// The MeansRegular group (grid axes, cos / sin, mask, winners, grid accumulators) is NOT the mesh's: release_mesh leaves it, so it survives nxs_dyn_set_mesh and
// nxs_dyn_regrid; release_means_regular (a new grid, ncols or nrows == 0, nxs_dyn_destroy) lets go of it.

// the grid accumulators at the sizes of the lists configured now, zeroed when made (nxs_dyn_means_configure with other sizes dropped them)
static int mr_ensure_grids(nxs_dyn_handle *h) {
    for (int k = 0; k < 2; ++k) {
        const int n = (int)h->means_ids[k].size();
        if (h->mr_grid_n[k] == n && (n == 0 || h->mr_grid[k])) continue;
        pool_free_one(h->mr_allocs, h->mr_grid[k]);
        h->mr_grid[k] = nullptr; h->mr_grid_n[k] = 0;
        if (!n) continue;
        const size_t count = (size_t)n * h->mr_G;
        if (int rc = dev_alloc(h, h->mr_allocs, &h->mr_grid[k], count)) return rc;
        HIPCHK(h, hipMemsetAsync(h->mr_grid[k], 0, count * sizeof(double), h->stream));
        h->mr_grid_n[k] = n;
    }
    return NXS_OK;
}

// what both launches receive; UM == NULL: the mesh at rest
static nxs_mr::Args mr_args(const nxs_dyn_handle *h, const double *UM) {
    nxs_mr::Args a{};
    const int n_el = (int)h->means_ids[0].size(), n_nod = (int)h->means_ids[1].size();
    a.m.G = h->mr_G; a.m.n_el = n_el; a.m.n_nod = n_nod; a.m.n_pairs = h->mr_n_pairs;
    a.m.ice_col = h->means_ice_mask_col; a.m.Neo = h->dm.Neo;
    for (int nv = 0; nv < n_el; ++nv) if (h->means_mask[0][nv]) a.m.mask_el |= 1u << nv;
    for (int nv = 0; nv < n_nod; ++nv) if (h->means_mask[1][nv]) a.m.mask_nod |= 1u << nv;
    for (int k = 0; k < h->mr_n_pairs; ++k) { a.m.first[k] = (unsigned char)h->mr_first[k]; a.m.second[k] = (unsigned char)h->mr_second[k]; }
    a.m.miss_val = h->mr_miss_val;
    a.m.cosang = h->mr_cos; a.m.sinang = h->mr_sin;
    a.m.el = h->d_means[0]; a.m.nod = h->d_means[1];
    a.m.grid_el = h->mr_grid[0]; a.m.grid_nod = h->mr_grid[1];
    a.ncols = h->mr_ncols; a.nrows = h->mr_nrows; a.Ne = h->dm.Ne; a.Nn = h->dm.Nn; a.spacing = h->mr_spacing;
    a.xg = h->mr_xg; a.yg = h->mr_yg;
    a.t0 = h->dm.t0; a.t1 = h->dm.t1; a.t2 = h->dm.t2; a.x0 = h->dm.x0; a.y0 = h->dm.y0; a.UM = UM;
    a.hit = h->mr_hit;
    return a;
}

// the winner of every grid point into mr_hit, on the stream
static int mr_find_hits(nxs_dyn_handle *h, const nxs_mr::Args &a) {
    HIPCHK(h, hipMemsetAsync(h->mr_hit, 0xFF, (size_t)h->mr_G * sizeof(int), h->stream));   // -1
    hipLaunchKernelGGL(k_means_regular_hits, dim3((a.Ne + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
}

int nxs_dyn_means_regular_set(nxs_dyn_handle *h, const nxs_dyn_means_regular *p) try {
    if (!h) return NXS_ERR_INVALID;
    const bool remove = !p || p->ncols == 0 || p->nrows == 0;
    if (p && (p->ncols < 0 || p->nrows < 0)) return fail(h, NXS_ERR_INVALID, "means_regular_set: ncols = %d, nrows = %d", p->ncols, p->nrows);
    if (!remove) {
        const int n_nod = (int)h->means_ids[1].size();
        if ((long long)p->ncols * p->nrows > 0x7fffffffll) return fail(h, NXS_ERR_INVALID, "means_regular_set: %d x %d grid points do not fit an int", p->ncols, p->nrows);
        if (!(p->mooring_spacing > 0.) || !std::isfinite(p->mooring_spacing)) return fail(h, NXS_ERR_INVALID, "means_regular_set: mooring_spacing must be positive (gridoutput.cpp:488)");
        if (!std::isfinite(p->xmin) || !std::isfinite(p->ymax)) return fail(h, NXS_ERR_INVALID, "means_regular_set: xmin or ymax is not finite");
        if (p->rotation == NXS_MEANS_ROTATE_GRID_THETA) return fail(h, NXS_ERR_INVALID, "means_regular_set: NXS_MEANS_ROTATE_GRID_THETA: the regular grid has no theta (M_grid = Grid())");
        if (p->rotation != NXS_MEANS_ROTATE_NONE && p->rotation != NXS_MEANS_ROTATE_NORTH_EAST)
            return fail(h, NXS_ERR_INVALID, "means_regular_set: rotation = %d is not an nxs_means_rotation mode", p->rotation);
        if (p->rotation == NXS_MEANS_ROTATE_NORTH_EAST && !p->gridLON) return fail(h, NXS_ERR_INVALID, "means_regular_set: NXS_MEANS_ROTATE_NORTH_EAST needs gridLON");
        if (p->n_pairs < 0 || p->n_pairs > NXS_MEANS_MAX_PAIRS) return fail(h, NXS_ERR_INVALID, "means_regular_set: n_pairs = %d (0..%d)", p->n_pairs, NXS_MEANS_MAX_PAIRS);
        for (int k = 0; k < p->n_pairs; ++k)
            if (p->pair_first[k] < 0 || p->pair_first[k] >= n_nod || p->pair_second[k] < 0 || p->pair_second[k] >= n_nod)
                return fail(h, NXS_ERR_INVALID, "means_regular_set: pair %d names the columns %d and %d, the configured nodal list has %d", k, p->pair_first[k], p->pair_second[k], n_nod);
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));   // (a launch may still use the previous grid)
    if (remove) { release_means_regular(h); return NXS_OK; }
    const size_t G = (size_t)p->ncols * p->nrows;
    // x_grid, y_grid exactly as InterpFromMeshToGridx.cpp:78, 88 builds them: the second is not ymin + spacing * j in its last bit
    std::vector<double> xg(p->ncols), yg(p->nrows);
    for (int i = 0; i < p->ncols; ++i) xg[i] = p->xmin + p->mooring_spacing * i;
    for (int i = 0; i < p->nrows; ++i) yg[p->nrows - 1 - i] = p->ymax - p->mooring_spacing * i;
    if (!std::isfinite(xg[p->ncols - 1]) || !std::isfinite(yg[0])) return fail(h, NXS_ERR_INVALID, "means_regular_set: a grid coordinate is not finite");
    // cosang / sinang: gridoutput.cpp:608-609, on the host, once, with the reference's own expression -- entry k is what the loop of :595 uses at i == k
    std::vector<double> cs, sn;
    if (p->rotation == NXS_MEANS_ROTATE_NORTH_EAST) {
        const double PI = NXS_MAPX_PI;   // contrib/mapx/include/mapx.h:47, the PI gridoutput.cpp sees
        const double rotation_angle = p->rotation_angle;
        cs.resize(G); sn.resize(G);
        for (size_t i = 0; i < G; ++i) {
            nxs_cos_sin_of_difference(rotation_angle, p->gridLON[i]*PI/180, &cs[i], &sn[i]);
            if (!std::isfinite(cs[i]) || !std::isfinite(sn[i])) return fail(h, NXS_ERR_INVALID, "means_regular_set: the angle of grid point %d is not finite", (int)i);
        }
    }
    release_means_regular(h);
    int rc;
    if ((rc = dev_alloc(h, h->mr_allocs, &h->mr_xg, (size_t)p->ncols)) || (rc = dev_alloc(h, h->mr_allocs, &h->mr_yg, (size_t)p->nrows)) || (rc = dev_alloc(h, h->mr_allocs, &h->mr_hit, G))) {
        release_means_regular(h);
        return rc;
    }
    if (!cs.empty() && ((rc = dev_alloc(h, h->mr_allocs, &h->mr_cos, G)) || (rc = dev_alloc(h, h->mr_allocs, &h->mr_sin, G)))) { release_means_regular(h); return rc; }
    HIPCHK(h, hipMemcpyAsync(h->mr_xg, xg.data(), xg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->mr_yg, yg.data(), yg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (!cs.empty()) {
        HIPCHK(h, hipMemcpyAsync(h->mr_cos, cs.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->mr_sin, sn.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // xg, yg, cs, sn go away
    h->mr_ncols = p->ncols; h->mr_nrows = p->nrows; h->mr_G = (int)G; h->mr_spacing = p->mooring_spacing; h->mr_miss_val = p->miss_val; h->mr_n_pairs = p->n_pairs;
    for (int k = 0; k < p->n_pairs; ++k) { h->mr_first[k] = p->pair_first[k]; h->mr_second[k] = p->pair_second[k]; }
    h->mr_set = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_set"); }

int nxs_dyn_means_regular_lsm(nxs_dyn_handle *h, const int32_t *lsm_in, int32_t *lsm_out) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_lsm: no grid (nxs_dyn_means_regular_set)");
    const size_t G = (size_t)h->mr_G;
    std::vector<int32_t> lsm(G);
    if (lsm_in) std::copy(lsm_in, lsm_in + G, lsm.begin());
    else {
        if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "means_regular_lsm: computing the mask needs set_mesh");
        HIPCHK(h, hipSetDevice(h->device));
        int *d_lsm = nullptr;
        if (int rc = dev_alloc(h, h->mr_allocs, &d_lsm, G)) return rc;
        int rc = mr_find_hits(h, mr_args(h, nullptr));   // a column of ones on every triangle, ghosts included, in the mesh at rest (gridoutput.cpp:563-573)
        hipError_t e = hipSuccess;
        if (!rc) {
            hipLaunchKernelGGL(k_means_regular_lsm, dim3((h->mr_G + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, h->stream, h->mr_G, (const int *)h->mr_hit, d_lsm);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(lsm.data(), d_lsm, G * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        }
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        pool_free_one(h->mr_allocs, d_lsm);
        if (rc) return rc;
        HIPCHK(h, e);
        HIPCHK(h, e2);
    }
    h->mr_lsm.swap(lsm);
    h->mr_have_lsm = true;
    if (lsm_out) std::copy(h->mr_lsm.begin(), h->mr_lsm.end(), lsm_out);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_lsm"); }

int nxs_dyn_means_regular_update(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "means_regular_update needs set_mesh and put_state");
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_update: no grid (nxs_dyn_means_regular_set)");
    const int n_el = (int)h->means_ids[0].size(), n_nod = (int)h->means_ids[1].size();
    if (!n_el && !n_nod) return fail(h, NXS_ERR_STATE, "means_regular_update: no variable is configured (nxs_dyn_means_configure)");
    for (int k = 0; k < h->mr_n_pairs; ++k)
        if (h->mr_first[k] >= n_nod || h->mr_second[k] >= n_nod)
            return fail(h, NXS_ERR_STATE, "means_regular_update: pair %d names the columns %d and %d, the nodal list configured now has %d", k, h->mr_first[k], h->mr_second[k], n_nod);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;   // (as nxs_dyn_means_update: never a mean of a half-made step without an error)
    if (int rc = mr_ensure_grids(h)) return rc;
    const nxs_mr::Args a = mr_args(h, h->ds.UM);
    const bool timed = h->means_timing != 0;
    if (timed) HIPCHK(h, hipEventRecord(h->mr_ev[0], h->stream));
    if (int rc = mr_find_hits(h, a)) return rc;
    if (timed) HIPCHK(h, hipEventRecord(h->mr_ev[1], h->stream));
    hipLaunchKernelGGL(k_means_regular_gather, dim3((a.m.G + BLOCK - 1) / BLOCK), dim3(BLOCK), (size_t)BLOCK * n_nod * sizeof(double), h->stream, a);
    HIPCHK(h, hipGetLastError());
    if (timed) { HIPCHK(h, hipEventRecord(h->mr_ev[2], h->stream)); h->mr_timed = true; }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_update"); }

int nxs_dyn_means_regular_get(nxs_dyn_handle *h, int32_t apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev, const double **nodal_dev) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_get: no grid (nxs_dyn_means_regular_set)");
    if (h->means_ids[0].empty() && h->means_ids[1].empty()) return fail(h, NXS_ERR_STATE, "means_regular_get: no variable is configured (nxs_dyn_means_configure)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = mr_ensure_grids(h)) return rc;
    double *dst[2] = {grid_elemental, grid_nodal};
    const size_t G = (size_t)h->mr_G;
    for (int k = 0; k < 2; ++k) {
        const size_t bytes = G * h->mr_grid_n[k] * sizeof(double);
        if (dst[k] && bytes) { pin_host_buffer(h, dst[k], bytes); HIPCHK(h, hipMemcpyAsync(dst[k], h->mr_grid[k], bytes, hipMemcpyDeviceToHost, h->stream)); }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->res_ready || h->flow_ready) { int rc = resident_error(h); if (rc) return rc; }   // (synchronised above)
    if (apply_lsm && h->mr_have_lsm)   // applyLSM (gridoutput.cpp:639-651) on the copy: the resident rows go on accumulating
        for (int k = 0; k < 2; ++k)
            if (dst[k])
                for (int nv = 0; nv < h->mr_grid_n[k]; ++nv) {
                    double *row = dst[k] + (size_t)nv * G;
                    for (size_t i = 0; i < G; ++i) if (h->mr_lsm[i] == 0) row[i] = h->mr_miss_val;
                }
    if (elemental_dev) *elemental_dev = h->mr_grid[0];
    if (nodal_dev) *nodal_dev = h->mr_grid[1];
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_get"); }

int nxs_dyn_means_regular_reset(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_reset: no grid (nxs_dyn_means_regular_set)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = mr_ensure_grids(h)) return rc;
    for (int k = 0; k < 2; ++k)
        if (h->mr_grid[k]) HIPCHK(h, hipMemsetAsync(h->mr_grid[k], 0, (size_t)h->mr_grid_n[k] * h->mr_G * sizeof(double), h->stream));
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_reset"); }
