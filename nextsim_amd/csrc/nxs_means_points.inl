// nxs_means_points.inl -- host side of nxs_dyn_means_points_* (include/nxs_dyn.h): the Moorings means on a LOADED grid -- GridOutput::updateGridMean() through the
// M_grid.loaded, non-conservative branch of updateGridMeanWorker, setLSM / applyLSM, rotateVectors, resetGridMean (model/gridoutput.cpp:387-415, 470-485, 511-545,
// 558-651).  Textually included by nxs_dyn.hip inside its extern "C" block, behind nxs_nodal_forcing.inl.  The kernels live next to the exact point locator
// (nxs_means_points_kernels.inl, nxs_interp.hip) and use the drifters' two locators; the per-point arithmetic is nxs_means_points_body.inl.
// The MeansPoints group (points, cos / sin, mask, grid accumulators) is NOT the mesh's: release_mesh leaves it, so it survives nxs_dyn_set_mesh and
// nxs_dyn_regrid; release_means_points (a new grid, G == 0, nxs_dyn_destroy) lets go of it.

// the grid accumulators at the sizes of the lists configured now, zeroed when made (nxs_dyn_means_configure with other sizes dropped them)
static int mp_ensure_grids(nxs_dyn_handle *h) {
    for (int k = 0; k < 2; ++k) {
        const int n = (int)h->means_ids[k].size();
        if (h->mp_grid_n[k] == n && (n == 0 || h->mp_grid[k])) continue;
        pool_free_one(h->mp_allocs, h->mp_grid[k]);
        h->mp_grid[k] = nullptr; h->mp_grid_n[k] = 0;
        if (!n) continue;
        const size_t count = (size_t)n * h->mp_G;
        if (int rc = dev_alloc(h, h->mp_allocs, &h->mp_grid[k], count)) return rc;
        HIPCHK(h, hipMemsetAsync(h->mp_grid[k], 0, count * sizeof(double), h->stream));
        h->mp_grid_n[k] = n;
    }
    return NXS_OK;
}

// what nxs_dyn_means_points_set and nxs_dyn_cpl_out_attach_grid refuse in a set of points (G > 0); `who` names the entry, n_nod is the nodal list the pairs index
static int mp_check_points(nxs_dyn_handle *h, const char *who, const nxs_dyn_means_points *p, int n_nod) {
    if (!p->gridX || !p->gridY) return fail(h, NXS_ERR_INVALID, "%s: gridX or gridY is NULL", who);
    if (p->rotation != NXS_MEANS_ROTATE_NONE && p->rotation != NXS_MEANS_ROTATE_NORTH_EAST && p->rotation != NXS_MEANS_ROTATE_GRID_THETA)
        return fail(h, NXS_ERR_INVALID, "%s: rotation = %d is not an nxs_means_rotation mode", who, p->rotation);
    if (p->rotation == NXS_MEANS_ROTATE_NORTH_EAST && !p->gridLON) return fail(h, NXS_ERR_INVALID, "%s: NXS_MEANS_ROTATE_NORTH_EAST needs gridLON", who);
    if (p->rotation == NXS_MEANS_ROTATE_GRID_THETA && !p->gridTheta) return fail(h, NXS_ERR_INVALID, "%s: NXS_MEANS_ROTATE_GRID_THETA needs gridTheta", who);
    if (p->n_pairs < 0 || p->n_pairs > NXS_MEANS_MAX_PAIRS) return fail(h, NXS_ERR_INVALID, "%s: n_pairs = %d (0..%d)", who, p->n_pairs, NXS_MEANS_MAX_PAIRS);
    for (int k = 0; k < p->n_pairs; ++k)
        if (p->pair_first[k] < 0 || p->pair_first[k] >= n_nod || p->pair_second[k] < 0 || p->pair_second[k] >= n_nod)
            return fail(h, NXS_ERR_INVALID, "%s: pair %d names the columns %d and %d, the configured nodal list has %d", who, k, p->pair_first[k], p->pair_second[k], n_nod);
    for (int i = 0; i < p->G; ++i)
        if (!std::isfinite(p->gridX[i]) || !std::isfinite(p->gridY[i])) return fail(h, NXS_ERR_INVALID, "%s: the coordinate of grid point %d is not finite", who, i);
    return NXS_OK;
}
// cosang / sinang: gridoutput.cpp:602-614, evaluated on the host, once, with the reference's own expressions (both left empty under NXS_MEANS_ROTATE_NONE)
static int mp_angles(nxs_dyn_handle *h, const char *who, const nxs_dyn_means_points *p, std::vector<double> &cs, std::vector<double> &sn) {
    if (p->rotation == NXS_MEANS_ROTATE_NONE) return NXS_OK;
    const size_t G = (size_t)p->G;
    const double PI = NXS_MAPX_PI;   // contrib/mapx/include/mapx.h:47, the PI gridoutput.cpp sees
    const double rotation_angle = p->rotation_angle;
    cs.resize(G); sn.resize(G);
    for (size_t i = 0; i < G; ++i) {
        nxs_cos_sin_of_difference(rotation_angle, p->rotation == NXS_MEANS_ROTATE_NORTH_EAST ? p->gridLON[i]*PI/180 : p->gridTheta[i], &cs[i], &sn[i]);
        if (!std::isfinite(cs[i]) || !std::isfinite(sn[i])) return fail(h, NXS_ERR_INVALID, "%s: the angle of grid point %d is not finite", who, (int)i);
    }
    return NXS_OK;
}

int nxs_dyn_means_points_set(nxs_dyn_handle *h, const nxs_dyn_means_points *p) try {
    if (!h) return NXS_ERR_INVALID;
    if (p && p->G < 0) return fail(h, NXS_ERR_INVALID, "means_points_set: G = %d < 0", p->G);
    if (p && p->G > 0)
        if (int rc = mp_check_points(h, "means_points_set", p, (int)h->means_ids[1].size())) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));   // (a launch may still use the previous grid)
    if (!p || p->G == 0) { release_means_points(h); return NXS_OK; }
    const size_t G = (size_t)p->G;
    std::vector<double> cs, sn;
    if (int rc = mp_angles(h, "means_points_set", p, cs, sn)) return rc;
    release_means_points(h);
    int rc;
    if ((rc = dev_alloc(h, h->mp_allocs, &h->mp_gx, G)) || (rc = dev_alloc(h, h->mp_allocs, &h->mp_gy, G))) { release_means_points(h); return rc; }
    if (!cs.empty() && ((rc = dev_alloc(h, h->mp_allocs, &h->mp_cos, G)) || (rc = dev_alloc(h, h->mp_allocs, &h->mp_sin, G)))) { release_means_points(h); return rc; }
    HIPCHK(h, hipMemcpyAsync(h->mp_gx, p->gridX, G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->mp_gy, p->gridY, G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (!cs.empty()) {
        HIPCHK(h, hipMemcpyAsync(h->mp_cos, cs.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->mp_sin, sn.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the caller's arrays, and cs / sn, may go away
    h->mp_G = p->G; h->mp_miss_val = p->miss_val; h->mp_n_pairs = p->n_pairs;
    for (int k = 0; k < p->n_pairs; ++k) { h->mp_first[k] = p->pair_first[k]; h->mp_second[k] = p->pair_second[k]; }
    h->mp_set = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_set"); }

int nxs_dyn_means_points_lsm(nxs_dyn_handle *h, const int32_t *lsm_in, int32_t *lsm_out) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_lsm: no grid points (nxs_dyn_means_points_set)");
    const size_t G = (size_t)h->mp_G;
    std::vector<int32_t> lsm(G);
    if (lsm_in) std::copy(lsm_in, lsm_in + G, lsm.begin());
    else {
        if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "means_points_lsm: computing the mask needs set_mesh");
        HIPCHK(h, hipSetDevice(h->device));
        if (!h->drift) h->drift = nxs_drifters::create();
        int *d_lsm = nullptr;
        if (int rc = dev_alloc(h, h->mp_allocs, &d_lsm, G)) return rc;
        std::string err;
        int rc = nxs_drifters::means_points_lsm(h->drift, h->stream, drift_view(h), h->mp_G, h->mp_gx, h->mp_gy, d_lsm, err);
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(lsm.data(), d_lsm, G * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        pool_free_one(h->mp_allocs, d_lsm);
        if (rc) return drift_rc(h, rc, "means_points_lsm", err);
        HIPCHK(h, e);
        HIPCHK(h, e2);
    }
    h->mp_lsm.swap(lsm);
    h->mp_have_lsm = true;
    if (lsm_out) std::copy(h->mp_lsm.begin(), h->mp_lsm.end(), lsm_out);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_lsm"); }

int nxs_dyn_means_points_update(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "means_points_update needs set_mesh and put_state");
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_update: no grid points (nxs_dyn_means_points_set)");
    const int n_el = (int)h->means_ids[0].size(), n_nod = (int)h->means_ids[1].size();
    if (!n_el && !n_nod) return fail(h, NXS_ERR_STATE, "means_points_update: no variable is configured (nxs_dyn_means_configure)");
    for (int k = 0; k < h->mp_n_pairs; ++k)
        if (h->mp_first[k] >= n_nod || h->mp_second[k] >= n_nod)
            return fail(h, NXS_ERR_STATE, "means_points_update: pair %d names the columns %d and %d, the nodal list configured now has %d", k, h->mp_first[k], h->mp_second[k], n_nod);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;   // (as nxs_dyn_means_update: never a mean of a half-made step without an error)
    if (int rc = mp_ensure_grids(h)) return rc;
    if (!h->drift) h->drift = nxs_drifters::create();
    nxs_mp::Args a{};
    a.G = h->mp_G; a.n_el = n_el; a.n_nod = n_nod; a.n_pairs = h->mp_n_pairs;
    a.ice_col = h->means_ice_mask_col; a.Neo = h->dm.Neo;
    for (int nv = 0; nv < n_el; ++nv) if (h->means_mask[0][nv]) a.mask_el |= 1u << nv;
    for (int nv = 0; nv < n_nod; ++nv) if (h->means_mask[1][nv]) a.mask_nod |= 1u << nv;
    for (int k = 0; k < h->mp_n_pairs; ++k) { a.first[k] = (unsigned char)h->mp_first[k]; a.second[k] = (unsigned char)h->mp_second[k]; }
    a.miss_val = h->mp_miss_val;
    a.gx = h->mp_gx; a.gy = h->mp_gy; a.cosang = h->mp_cos; a.sinang = h->mp_sin;
    a.el = h->d_means[0]; a.nod = h->d_means[1];
    a.grid_el = h->mp_grid[0]; a.grid_nod = h->mp_grid[1];
    std::string err;
    return drift_rc(h, nxs_drifters::means_points_update(h->drift, h->stream, drift_view(h), h->ds.UM, a, err), "means_points_update", err);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_update"); }

int nxs_dyn_means_points_get(nxs_dyn_handle *h, int32_t apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev, const double **nodal_dev) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_get: no grid points (nxs_dyn_means_points_set)");
    if (h->means_ids[0].empty() && h->means_ids[1].empty()) return fail(h, NXS_ERR_STATE, "means_points_get: no variable is configured (nxs_dyn_means_configure)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = mp_ensure_grids(h)) return rc;
    double *dst[2] = {grid_elemental, grid_nodal};
    const size_t G = (size_t)h->mp_G;
    for (int k = 0; k < 2; ++k) {
        const size_t bytes = G * h->mp_grid_n[k] * sizeof(double);
        if (dst[k] && bytes) { pin_host_buffer(h, dst[k], bytes); HIPCHK(h, hipMemcpyAsync(dst[k], h->mp_grid[k], bytes, hipMemcpyDeviceToHost, h->stream)); }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->res_ready || h->flow_ready) { int rc = resident_error(h); if (rc) return rc; }   // (synchronised above)
    if (apply_lsm && h->mp_have_lsm)   // applyLSM (gridoutput.cpp:639-651) on the copy: the resident rows go on accumulating
        for (int k = 0; k < 2; ++k)
            if (dst[k])
                for (int nv = 0; nv < h->mp_grid_n[k]; ++nv) {
                    double *row = dst[k] + (size_t)nv * G;
                    for (size_t i = 0; i < G; ++i) if (h->mp_lsm[i] == 0) row[i] = h->mp_miss_val;
                }
    if (elemental_dev) *elemental_dev = h->mp_grid[0];
    if (nodal_dev) *nodal_dev = h->mp_grid[1];
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_get"); }

int nxs_dyn_means_points_reset(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_reset: no grid points (nxs_dyn_means_points_set)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = mp_ensure_grids(h)) return rc;
    for (int k = 0; k < 2; ++k)
        if (h->mp_grid[k]) HIPCHK(h, hipMemsetAsync(h->mp_grid[k], 0, (size_t)h->mp_grid_n[k] * h->mp_G * sizeof(double), h->stream));
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_reset"); }
