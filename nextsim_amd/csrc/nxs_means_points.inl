// nxs_means_points.inl -- host side of nxs_dyn_means_points_* (include/nxs_dyn.h): the Moorings means on a LOADED grid -- GridOutput::updateGridMean() through the
// M_grid.loaded, non-conservative branch of updateGridMeanWorker, setLSM / applyLSM, rotateVectors, resetGridMean (model/gridoutput.cpp:387-415, 470-485, 511-545,
// 558-651).  Textually included by nxs_dyn.hip inside its extern "C" block, behind nxs_nodal_forcing.inl.  The kernels live next to the exact point locator
// (nxs_means_points_kernels.inl, nxs_interp.hip) and use the drifters' two locators; the per-point arithmetic is nxs_means_points_body.inl.
// The MeansPoints group is one OutputGrid (points, cos / sin, mask, grid accumulators: h->mp, served by nxs_output_grid.inl) and a flag.  It is NOT the mesh's:
// release_mesh leaves it, so it survives nxs_dyn_set_mesh and nxs_dyn_regrid; release_means_points (a new grid, G == 0, nxs_dyn_destroy) lets go of it.

// what nxs_dyn_means_points_set and nxs_dyn_cpl_out_attach_grid refuse in a set of points (G > 0); `who` names the entry, n_nod is the nodal list the pairs index
static int mp_check_points(nxs_dyn_handle *h, const char *who, const nxs_dyn_means_points *p, int n_nod) {
    if (!p->gridX || !p->gridY) return fail(h, NXS_ERR_INVALID, "%s: gridX or gridY is NULL", who);
    if (p->rotation != NXS_MEANS_ROTATE_NONE && p->rotation != NXS_MEANS_ROTATE_NORTH_EAST && p->rotation != NXS_MEANS_ROTATE_GRID_THETA)
        return fail(h, NXS_ERR_INVALID, "%s: rotation = %d is not an nxs_means_rotation mode", who, p->rotation);
    if (p->rotation == NXS_MEANS_ROTATE_NORTH_EAST && !p->gridLON) return fail(h, NXS_ERR_INVALID, "%s: NXS_MEANS_ROTATE_NORTH_EAST needs gridLON", who);
    if (p->rotation == NXS_MEANS_ROTATE_GRID_THETA && !p->gridTheta) return fail(h, NXS_ERR_INVALID, "%s: NXS_MEANS_ROTATE_GRID_THETA needs gridTheta", who);
    if (int rc = og_check_pairs(h, who, p->n_pairs, p->pair_first, p->pair_second, n_nod)) return rc;
    for (int i = 0; i < p->G; ++i)
        if (!std::isfinite(p->gridX[i]) || !std::isfinite(p->gridY[i])) return fail(h, NXS_ERR_INVALID, "%s: the coordinate of grid point %d is not finite", who, i);
    return NXS_OK;
}
// cosang / sinang: gridoutput.cpp:602-614, evaluated on the host, once, with the reference's own expressions (both left empty under NXS_MEANS_ROTATE_NONE).  Entry i
// is what the loop of :595 uses at i: on the regular grid that is the BAMG index, and gridLON is read in the order it was given (nxs_means_regular_body.inl)
static int mp_angles(nxs_dyn_handle *h, const char *who, size_t G, int rotation, double rotation_angle, const double *gridLON, const double *gridTheta, std::vector<double> &cs,
                     std::vector<double> &sn) {
    if (rotation == NXS_MEANS_ROTATE_NONE) return NXS_OK;
    const double PI = NXS_MAPX_PI;   // contrib/mapx/include/mapx.h:47, the PI gridoutput.cpp sees
    cs.resize(G); sn.resize(G);
    for (size_t i = 0; i < G; ++i) {
        nxs_cos_sin_of_difference(rotation_angle, rotation == NXS_MEANS_ROTATE_NORTH_EAST ? gridLON[i]*PI/180 : gridTheta[i], &cs[i], &sn[i]);
        if (!std::isfinite(cs[i]) || !std::isfinite(sn[i])) return fail(h, NXS_ERR_INVALID, "%s: the angle of grid point %d is not finite", who, (int)i);
    }
    return NXS_OK;
}

// the tail of nxs_dyn_means_points_get and nxs_dyn_means_regular_get: both always synchronise
static int means_grid_get(nxs_dyn_handle *h, const char *who, OutputGrid &g, int32_t apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev, const double **nodal_dev) {
    if (h->means_ids[0].empty() && h->means_ids[1].empty()) return fail(h, NXS_ERR_STATE, "%s: no variable is configured (nxs_dyn_means_configure)", who);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = og_ensure(h, g, h->means_ids)) return rc;
    double *const dst[2] = {grid_elemental, grid_nodal};
    return og_copy_out(h, g, apply_lsm != 0, dst, elemental_dev, nodal_dev, true, nullptr);
}

int nxs_dyn_means_points_set(nxs_dyn_handle *h, const nxs_dyn_means_points *p) try {
    if (!h) return NXS_ERR_INVALID;
    if (p && p->G < 0) return fail(h, NXS_ERR_INVALID, "means_points_set: G = %d < 0", p->G);
    if (p && p->G > 0)
        if (int rc = mp_check_points(h, "means_points_set", p, (int)h->means_ids[1].size())) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));   // (a launch may still use the previous grid)
    if (!p || p->G == 0) { release_means_points(h); return NXS_OK; }
    std::vector<double> cs, sn;
    if (int rc = mp_angles(h, "means_points_set", (size_t)p->G, p->rotation, p->rotation_angle, p->gridLON, p->gridTheta, cs, sn)) return rc;
    release_means_points(h);
    h->mp.G = p->G;
    if (int rc = og_upload(h, h->mp, p->gridX, p->gridY, cs, sn, p->miss_val, p->n_pairs, p->pair_first, p->pair_second)) { release_means_points(h); return rc; }
    h->mp_set = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_set"); }

int nxs_dyn_means_points_lsm(nxs_dyn_handle *h, const int32_t *lsm_in, int32_t *lsm_out) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_lsm: no grid points (nxs_dyn_means_points_set)");
    return og_lsm(h, "means_points_lsm", h->mp, lsm_in, lsm_out, [h](int *d_lsm) {
        if (!h->drift) h->drift = nxs_drifters::create();
        std::string err;
        return drift_rc(h, nxs_drifters::means_points_lsm(h->drift, h->stream, drift_view(h), h->mp.G, h->mp.gx, h->mp.gy, d_lsm, err), "means_points_lsm", err);
    });
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_lsm"); }

int nxs_dyn_means_points_update(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "means_points_update needs set_mesh and put_state");
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_update: no grid points (nxs_dyn_means_points_set)");
    const int n_el = (int)h->means_ids[0].size(), n_nod = (int)h->means_ids[1].size();
    if (!n_el && !n_nod) return fail(h, NXS_ERR_STATE, "means_points_update: no variable is configured (nxs_dyn_means_configure)");
    if (int rc = og_check_stored_pairs(h, "means_points_update", h->mp, n_nod)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;   // (as nxs_dyn_means_update: never a mean of a half-made step without an error)
    if (int rc = og_ensure(h, h->mp, h->means_ids)) return rc;
    if (!h->drift) h->drift = nxs_drifters::create();
    const nxs_mp::Args a = og_args(h, h->mp, n_el, n_nod, h->means_mask, h->means_ice_mask_col, h->d_means[0], h->d_means[1]);
    std::string err;
    return drift_rc(h, nxs_drifters::means_points_update(h->drift, h->stream, drift_view(h), h->ds.UM, a, err), "means_points_update", err);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_update"); }

int nxs_dyn_means_points_get(nxs_dyn_handle *h, int32_t apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev, const double **nodal_dev) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_get: no grid points (nxs_dyn_means_points_set)");
    return means_grid_get(h, "means_points_get", h->mp, apply_lsm, grid_elemental, grid_nodal, elemental_dev, nodal_dev);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_get"); }

int nxs_dyn_means_points_reset(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->mp_set) return fail(h, NXS_ERR_STATE, "means_points_reset: no grid points (nxs_dyn_means_points_set)");
    return og_reset(h, h->mp, h->means_ids);
} catch (...) { return dyn_caught(h, "nxs_dyn_means_points_reset"); }
