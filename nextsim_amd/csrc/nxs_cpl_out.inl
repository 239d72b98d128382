// nxs_cpl_out.inl -- host side of nxs_dyn_cpl_out_* and nxs_dyn_fsd_diag_configure (include/nxs_dyn.h): the coupler's outgoing fields, M_cpl_out -- the "coupler put"
// of FiniteElement::step() (FE.cpp:8226-8266) and the put in front of a regrid (FE.cpp:8012-8052).  Textually included by nxs_dyn.hip inside its extern "C" block,
// behind nxs_means_points.inl, whose checks of a set of points and whose cos / sin it shares.
// A second accumulator set beside the Moorings': its own id lists and tables on the handle, its mesh accumulators in the CplOut group (gone with the mesh, made
// again zeroed by set_mesh / regrid), the exchange grid's points and data_grid in the CplOutGrid group (NOT the mesh's): one OutputGrid, h->cplg, served by
// nxs_output_grid.inl like the two grids of the Moorings, and a flag.  The accumulation is means_update_set --
// the kernels of nxs_dyn_means_update --, the elemental leg of the put nxs_gridmap_send_rows (k_gridmap_send, nxs_gridmap_kernels.inl), the nodal leg
// nxs_drifters::means_points_update on this set's rows with n_el = 0 and no ice mask: no second locator, no copy of the per-point body.

static bool cpl_out_configured(const nxs_dyn_handle *h) { return !h->cpl_ids[0].empty() || !h->cpl_ids[1].empty(); }

int nxs_dyn_cpl_out_configure(nxs_dyn_handle *h, const nxs_dyn_means_config *c) try {
    if (!h || !c) return NXS_ERR_INVALID;
    std::vector<int> ids[2];
    std::vector<unsigned char> mask[2];
    int ice_col = -1;
    bool any_mask = false;
    if (int rc = means_parse_config(h, "cpl_out_configure", c, ids, mask, &ice_col, &any_mask)) return rc;
    if (any_mask) return fail(h, NXS_ERR_INVALID, "cpl_out_configure: a variable has `mask` set: initOASIS sets none (FE.cpp:7596-7684) and the ice-mask rule is not built for this set");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    for (double *&q : h->d_cpl) { pool_free_one(h->cpl_allocs, q); q = nullptr; }
    for (int k = 0; k < 2; ++k) h->cpl_ids[k] = ids[k];
    if (!cpl_out_configured(h)) { release_cpl_out(h); release_cpl_out_grid(h); return NXS_OK; }
    og_drop_resized(h->cplg, ids);   // data_grid is made again by the next put / reset_grid when a list changes its size
    if (h->have_mesh) { int rc = cpl_out_make_buffers(h); if (rc) return rc; }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_configure"); }

int nxs_dyn_cpl_out_update(nxs_dyn_handle *h, double time_factor) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "cpl_out_update needs set_mesh and put_state");
    if (!cpl_out_configured(h)) return fail(h, NXS_ERR_STATE, "cpl_out_update: no variable is configured (nxs_dyn_cpl_out_configure)");
    return means_update_set(h, "cpl_out_update", h->cpl_ids, h->cpl_tab, h->d_cpl, time_factor, false);
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_update"); }

int nxs_dyn_cpl_out_get(nxs_dyn_handle *h, double *elemental, double *nodal, const double **elemental_dev, const double **nodal_dev) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "cpl_out_get before set_mesh");
    if (!cpl_out_configured(h)) return fail(h, NXS_ERR_STATE, "cpl_out_get: no variable is configured (nxs_dyn_cpl_out_configure)");
    HIPCHK(h, hipSetDevice(h->device));
    double *dst[2] = {elemental, nodal};
    const size_t len[2] = {(size_t)h->dm.Ne, (size_t)h->dm.Nn};
    for (int k = 0; k < 2; ++k) {
        const size_t bytes = len[k] * h->cpl_ids[k].size() * sizeof(double);
        if (dst[k] && bytes) { pin_host_buffer(h, dst[k], bytes); HIPCHK(h, hipMemcpyAsync(dst[k], h->d_cpl[k], bytes, hipMemcpyDeviceToHost, h->stream)); }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (elemental_dev) *elemental_dev = h->d_cpl[0];
    if (nodal_dev) *nodal_dev = h->d_cpl[1];
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_get"); }

// resetMeshMean(bamgmesh) of this set, queued on the stream
static int cpl_out_zero_mesh(nxs_dyn_handle *h) {
    const size_t len[2] = {(size_t)h->dm.Ne, (size_t)h->dm.Nn};
    for (int k = 0; k < 2; ++k)
        if (h->d_cpl[k]) HIPCHK(h, hipMemsetAsync(h->d_cpl[k], 0, len[k] * h->cpl_ids[k].size() * sizeof(double), h->stream));
    return NXS_OK;
}
// ... and resetGridMean() behind it: NXS_CPL_OUT_RESET (FE.cpp:8262-8263)
static int cpl_out_zero_both(nxs_dyn_handle *h) {
    if (int rc = cpl_out_zero_mesh(h)) return rc;
    return og_zero(h, h->cplg);
}

int nxs_dyn_cpl_out_reset(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "cpl_out_reset before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    return cpl_out_zero_mesh(h);
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_reset"); }

int nxs_dyn_cpl_out_attach_grid(nxs_dyn_handle *h, struct nxs_gridmap *map, const nxs_dyn_means_points *p) try {
    if (!h || !map) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "cpl_out_attach_grid before set_mesh");
    if (!cpl_out_configured(h)) return fail(h, NXS_ERR_STATE, "cpl_out_attach_grid: no variable is configured (nxs_dyn_cpl_out_configure)");
    int32_t map_nels = 0, G = 0;
    if (int rc = nxs_gridmap_info(map, nullptr, nullptr, nullptr, nullptr, &map_nels, &G)) return fail(h, rc, "cpl_out_attach_grid: %s", nxs_interp_last_error());
    const int n_nod = (int)h->cpl_ids[1].size();
    if (p && p->G <= 0) p = nullptr;
    if (p && p->G != G) return fail(h, NXS_ERR_INVALID, "cpl_out_attach_grid: the map is on a grid of %d cells, the points are %d", G, p->G);
    if (p)
        if (int rc = mp_check_points(h, "cpl_out_attach_grid", p, n_nod)) return rc;
    if (map_nels != h->dm.Ne) return fail(h, NXS_ERR_STATE, "cpl_out_attach_grid: the map is on a mesh of %d elements, the handle's has %d", map_nels, h->dm.Ne);
    if (n_nod > 0 && !p) return fail(h, NXS_ERR_STATE, "cpl_out_attach_grid: %d nodal variables are configured but no points were given (the nodal leg locates the P-points)", n_nod);
    std::vector<double> cs, sn;
    if (p)
        if (int rc = mp_angles(h, "cpl_out_attach_grid", (size_t)p->G, p->rotation, p->rotation_angle, p->gridLON, p->gridTheta, cs, sn)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (a launch may still use the previous points)
    if (h->cplg.G != G) release_cpl_out_grid(h);   // another grid: its accumulators go too
    OutputGrid &g = h->cplg;
    for (double **q : {&g.gx, &g.gy, &g.cos, &g.sin}) { pool_free_one(g.allocs, *q); *q = nullptr; }
    h->cpl_points = false; g.n_pairs = 0;
    g.G = G;
    if (p) {
        if (int rc = og_upload(h, g, p->gridX, p->gridY, cs, sn, p->miss_val, p->n_pairs, p->pair_first, p->pair_second)) return rc;
        h->cpl_points = true;
    }
    h->cpl_map = map;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_attach_grid"); }

int nxs_dyn_cpl_out_put(nxs_dyn_handle *h, double *grid_elemental, double *grid_nodal, const double **elemental_dev, const double **nodal_dev, int32_t flags) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "cpl_out_put needs set_mesh and put_state");
    const int n_el = (int)h->cpl_ids[0].size(), n_nod = (int)h->cpl_ids[1].size();
    if (!n_el && !n_nod) return fail(h, NXS_ERR_STATE, "cpl_out_put: no variable is configured (nxs_dyn_cpl_out_configure)");
    if (!h->cpl_map) return fail(h, NXS_ERR_STATE, "cpl_out_put: no exchange grid is attached on this mesh (nxs_dyn_cpl_out_attach_grid; again after nxs_dyn_set_mesh / nxs_dyn_regrid)");
    if (n_nod > 0 && !h->cpl_points) return fail(h, NXS_ERR_STATE, "cpl_out_put: %d nodal variables are configured but the attached grid has no points", n_nod);
    if (int rc = og_check_stored_pairs(h, "cpl_out_put", h->cplg, n_nod)) return rc;
    if (flags & ~NXS_CPL_OUT_RESET) return fail(h, NXS_ERR_INVALID, "cpl_out_put: unknown flags %d", flags);
    if ((flags & NXS_CPL_OUT_RESET) && ((n_el && !grid_elemental) || (n_nod && !grid_nodal)))
        return fail(h, NXS_ERR_INVALID, "cpl_out_put: NXS_CPL_OUT_RESET without a host array for every configured list: the values would be gone");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;   // (as nxs_dyn_means_update: never a mean of a half-made step without an error)
    if (int rc = og_ensure(h, h->cplg, h->cpl_ids)) return rc;
    if (n_el > 0)   // the elemental leg: interpMethod::conservative (gridoutput.cpp:473, 545)
        if (int rc = nxs_gridmap_send_rows(h->cpl_map, n_el, h->d_cpl[0], h->cplg.grid[0], NXS_REGRID_IN_DEVICE | NXS_REGRID_OUT_DEVICE, (void *)h->stream))
            return fail(h, rc, "cpl_out_put: %s", nxs_interp_last_error());
    if (n_nod > 0) {   // the nodal leg: the exact locator in the mesh displaced by M_UM, the P1 gather, rotateVectors, the proc mask (gridoutput.cpp:478-485, 511-543)
        if (!h->drift) h->drift = nxs_drifters::create();
        const nxs_mp::Args a = og_args(h, h->cplg, 0, n_nod, nullptr, -1, nullptr, h->d_cpl[1]);   // this set's rows, n_el = 0 and no ice mask
        std::string err;
        if (int rc = drift_rc(h, nxs_drifters::means_points_update(h->drift, h->stream, drift_view(h), h->ds.UM, a, err), "cpl_out_put", err)) return rc;
    }
    double *const dst[2] = {grid_elemental, grid_nodal};   // synchronises only when something was copied; the reset is queued behind the copies on the same stream
    return og_copy_out(h, h->cplg, false, dst, elemental_dev, nodal_dev, false, (flags & NXS_CPL_OUT_RESET) ? cpl_out_zero_both : nullptr);
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_put"); }

int nxs_dyn_cpl_out_reset_grid(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!cpl_out_configured(h)) return fail(h, NXS_ERR_STATE, "cpl_out_reset_grid: no variable is configured (nxs_dyn_cpl_out_configure)");
    if (h->cplg.G <= 0) return fail(h, NXS_ERR_STATE, "cpl_out_reset_grid: no exchange grid was attached (nxs_dyn_cpl_out_attach_grid)");
    return og_reset(h, h->cplg, h->cpl_ids);
} catch (...) { return dyn_caught(h, "nxs_dyn_cpl_out_reset_grid"); }

// wave_coupling.dmax_c_threshold, fsd_unbroken_floe_size, fsd_min_floe_size (FE.cpp:1387, 1410-1411): what D_dmax / D_dmean read beside nxs_dyn_fsd_configure's tables
int nxs_dyn_fsd_diag_configure(nxs_dyn_handle *h, double dmax_c_threshold, double fsd_unbroken_floe_size, double fsd_min_floe_size) try {
    if (!h) return NXS_ERR_INVALID;
    if (!std::isfinite(dmax_c_threshold) || !std::isfinite(fsd_unbroken_floe_size) || !std::isfinite(fsd_min_floe_size))
        return fail(h, NXS_ERR_INVALID, "fsd_diag_configure: dmax_c_threshold = %g, fsd_unbroken_floe_size = %g, fsd_min_floe_size = %g must be finite", dmax_c_threshold,
                    fsd_unbroken_floe_size, fsd_min_floe_size);
    h->fsd_diag[0] = dmax_c_threshold; h->fsd_diag[1] = fsd_unbroken_floe_size; h->fsd_diag[2] = fsd_min_floe_size;
    h->fsd_diag_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_diag_configure"); }
