// nxs_means_regular.inl -- host side of nxs_dyn_means_regular_* (include/nxs_dyn.h): the Moorings means on the REGULAR grid -- GridOutput::updateGridMean() through
// the M_is_regular_grid branch of updateGridMeanWorker, setProcMask, setLSM / applyLSM, rotateVectors, resetGridMean (model/gridoutput.cpp:360-415, 486-538,
// 558-651) and the arithmetic of contrib/bamg/src/InterpFromMeshToGridx.cpp.  Textually included by nxs_dyn.hip inside its extern "C" block, behind
// nxs_means_points.inl.  The kernels are nxs_means_regular_kernels.inl, the arithmetic nxs_means_regular_body.inl.
// The MeansRegular group is one OutputGrid (cos / sin, mask, grid accumulators: h->mr, served by nxs_output_grid.inl) plus the grid axes and the winners.  It is NOT
// the mesh's: release_mesh leaves it, so it survives nxs_dyn_set_mesh and nxs_dyn_regrid; release_means_regular (a new grid, ncols or nrows == 0, nxs_dyn_destroy)
// lets go of it.

// what both launches receive; UM == NULL: the mesh at rest
static nxs_mr::Args mr_args(const nxs_dyn_handle *h, const double *UM) {
    nxs_mr::Args a{};
    a.m = og_args(h, h->mr, (int)h->means_ids[0].size(), (int)h->means_ids[1].size(), h->means_mask, h->means_ice_mask_col, h->d_means[0], h->d_means[1]);
    a.ncols = h->mr_ncols; a.nrows = h->mr_nrows; a.Ne = h->dm.Ne; a.Nn = h->dm.Nn; a.spacing = h->mr_spacing;
    a.xg = h->mr_xg; a.yg = h->mr_yg;
    a.t0 = h->dm.t0; a.t1 = h->dm.t1; a.t2 = h->dm.t2; a.x0 = h->dm.x0; a.y0 = h->dm.y0; a.UM = UM;
    a.hit = h->mr_hit;
    return a;
}

// the winner of every grid point into mr_hit, on the stream
static int mr_find_hits(nxs_dyn_handle *h, const nxs_mr::Args &a) {
    HIPCHK(h, hipMemsetAsync(h->mr_hit, 0xFF, (size_t)h->mr.G * sizeof(int), h->stream));   // -1
    hipLaunchKernelGGL(k_means_regular_hits, dim3((a.Ne + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
}

int nxs_dyn_means_regular_set(nxs_dyn_handle *h, const nxs_dyn_means_regular *p) try {
    if (!h) return NXS_ERR_INVALID;
    const bool remove = !p || p->ncols == 0 || p->nrows == 0;
    if (p && (p->ncols < 0 || p->nrows < 0)) return fail(h, NXS_ERR_INVALID, "means_regular_set: ncols = %d, nrows = %d", p->ncols, p->nrows);
    if (!remove) {
        if ((long long)p->ncols * p->nrows > 0x7fffffffll) return fail(h, NXS_ERR_INVALID, "means_regular_set: %d x %d grid points do not fit an int", p->ncols, p->nrows);
        if (!(p->mooring_spacing > 0.) || !std::isfinite(p->mooring_spacing)) return fail(h, NXS_ERR_INVALID, "means_regular_set: mooring_spacing must be positive (gridoutput.cpp:488)");
        if (!std::isfinite(p->xmin) || !std::isfinite(p->ymax)) return fail(h, NXS_ERR_INVALID, "means_regular_set: xmin or ymax is not finite");
        if (p->rotation == NXS_MEANS_ROTATE_GRID_THETA) return fail(h, NXS_ERR_INVALID, "means_regular_set: NXS_MEANS_ROTATE_GRID_THETA: the regular grid has no theta (M_grid = Grid())");
        if (p->rotation != NXS_MEANS_ROTATE_NONE && p->rotation != NXS_MEANS_ROTATE_NORTH_EAST)
            return fail(h, NXS_ERR_INVALID, "means_regular_set: rotation = %d is not an nxs_means_rotation mode", p->rotation);
        if (p->rotation == NXS_MEANS_ROTATE_NORTH_EAST && !p->gridLON) return fail(h, NXS_ERR_INVALID, "means_regular_set: NXS_MEANS_ROTATE_NORTH_EAST needs gridLON");
        if (int rc = og_check_pairs(h, "means_regular_set", p->n_pairs, p->pair_first, p->pair_second, (int)h->means_ids[1].size())) return rc;
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
    std::vector<double> cs, sn;   // entry k is what the loop of gridoutput.cpp:595 uses at i == k: by BAMG index, gridLON in the order given
    if (int rc = mp_angles(h, "means_regular_set", G, p->rotation, p->rotation_angle, p->gridLON, nullptr, cs, sn)) return rc;
    release_means_regular(h);
    h->mr.G = (int)G;
    int rc;
    if ((rc = dev_alloc(h, h->mr.allocs, &h->mr_xg, (size_t)p->ncols)) || (rc = dev_alloc(h, h->mr.allocs, &h->mr_yg, (size_t)p->nrows)) || (rc = dev_alloc(h, h->mr.allocs, &h->mr_hit, G))) {
        release_means_regular(h);
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->mr_xg, xg.data(), xg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->mr_yg, yg.data(), yg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = og_upload(h, h->mr, nullptr, nullptr, cs, sn, p->miss_val, p->n_pairs, p->pair_first, p->pair_second))) { release_means_regular(h); return rc; }   // (synchronises: xg, yg go away)
    h->mr_ncols = p->ncols; h->mr_nrows = p->nrows; h->mr_spacing = p->mooring_spacing;
    h->mr_set = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_set"); }

int nxs_dyn_means_regular_lsm(nxs_dyn_handle *h, const int32_t *lsm_in, int32_t *lsm_out) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_lsm: no grid (nxs_dyn_means_regular_set)");
    return og_lsm(h, "means_regular_lsm", h->mr, lsm_in, lsm_out, [h](int *d_lsm) {
        if (int rc = mr_find_hits(h, mr_args(h, nullptr))) return rc;   // a column of ones on every triangle, ghosts included, in the mesh at rest (gridoutput.cpp:563-573)
        hipLaunchKernelGGL(k_means_regular_lsm, dim3((h->mr.G + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, h->stream, h->mr.G, (const int *)h->mr_hit, d_lsm);
        HIPCHK(h, hipGetLastError());
        return (int)NXS_OK;
    });
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_lsm"); }

int nxs_dyn_means_regular_update(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "means_regular_update needs set_mesh and put_state");
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_update: no grid (nxs_dyn_means_regular_set)");
    const int n_el = (int)h->means_ids[0].size(), n_nod = (int)h->means_ids[1].size();
    if (!n_el && !n_nod) return fail(h, NXS_ERR_STATE, "means_regular_update: no variable is configured (nxs_dyn_means_configure)");
    if (int rc = og_check_stored_pairs(h, "means_regular_update", h->mr, n_nod)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;   // (as nxs_dyn_means_update: never a mean of a half-made step without an error)
    if (int rc = og_ensure(h, h->mr, h->means_ids)) return rc;
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
    return means_grid_get(h, "means_regular_get", h->mr, apply_lsm, grid_elemental, grid_nodal, elemental_dev, nodal_dev);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_get"); }

int nxs_dyn_means_regular_reset(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mr_set) return fail(h, NXS_ERR_STATE, "means_regular_reset: no grid (nxs_dyn_means_regular_set)");
    return og_reset(h, h->mr, h->means_ids);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_regular_reset"); }
