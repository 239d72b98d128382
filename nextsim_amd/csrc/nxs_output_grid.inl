// nxs_output_grid.inl -- what the handle's three output grids share on the host: the loaded-grid Moorings (nxs_means_points.inl), the regular-grid Moorings
// (nxs_means_regular.inl) and the coupler's exchange grid (nxs_cpl_out.inl) each wrap ONE OutputGrid (nxs_dyn.hip) and call these routines with it and, where a
// routine needs them, with the id lists it serves (means_ids for the Moorings, cpl_ids for the coupler).  Textually included by nxs_dyn.hip in front of the means'
// host code.  `who` is the entry's name in front of every text.  What the three entries do differently -- their checks of coordinates and rotation, what a new
// grid releases, when they synchronise, their locators and launches -- stays in their own files.

// the accumulators at the sizes of the lists configured now, zeroed when made (a *_configure with other sizes dropped them: og_drop_resized)
static int og_ensure(nxs_dyn_handle *h, OutputGrid &g, const std::vector<int> *ids /* [2] */) {
    for (int k = 0; k < 2; ++k) {
        const int n = (int)ids[k].size();
        if (g.grid_n[k] == n && (n == 0 || g.grid[k])) continue;
        pool_free_one(g.allocs, g.grid[k]);
        g.grid[k] = nullptr; g.grid_n[k] = 0;
        if (!n) continue;
        const size_t count = (size_t)n * g.G;
        if (int rc = dev_alloc(h, g.allocs, &g.grid[k], count)) return rc;
        HIPCHK(h, hipMemsetAsync(g.grid[k], 0, count * sizeof(double), h->stream));
        g.grid_n[k] = n;
    }
    return NXS_OK;
}
// a list changes its size to that of new_ids: its accumulator goes, and is made again by the next call that needs it (the stream is synchronised)
static void og_drop_resized(OutputGrid &g, const std::vector<int> *new_ids /* [2] */) {
    for (int k = 0; k < 2; ++k)
        if (g.grid_n[k] != (int)new_ids[k].size()) { pool_free_one(g.allocs, g.grid[k]); g.grid[k] = nullptr; g.grid_n[k] = 0; }
}
// resetGridMean(), queued on the stream
static int og_zero(nxs_dyn_handle *h, const OutputGrid &g) {
    for (int k = 0; k < 2; ++k)
        if (g.grid[k]) HIPCHK(h, hipMemsetAsync(g.grid[k], 0, (size_t)g.grid_n[k] * g.G * sizeof(double), h->stream));
    return NXS_OK;
}
// a *_reset entry: the accumulators of these lists, made if need be, to zero
static int og_reset(nxs_dyn_handle *h, OutputGrid &g, const std::vector<int> *ids /* [2] */) {
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = og_ensure(h, g, ids)) return rc;
    return og_zero(h, g);
}

// the pairs of a descriptor against the nodal list they index ...
static int og_check_pairs(nxs_dyn_handle *h, const char *who, int n_pairs, const int32_t *first, const int32_t *second, int n_nod) {
    if (n_pairs < 0 || n_pairs > NXS_MEANS_MAX_PAIRS) return fail(h, NXS_ERR_INVALID, "%s: n_pairs = %d (0..%d)", who, n_pairs, NXS_MEANS_MAX_PAIRS);
    for (int k = 0; k < n_pairs; ++k)
        if (first[k] < 0 || first[k] >= n_nod || second[k] < 0 || second[k] >= n_nod)
            return fail(h, NXS_ERR_INVALID, "%s: pair %d names the columns %d and %d, the configured nodal list has %d", who, k, first[k], second[k], n_nod);
    return NXS_OK;
}
// ... and the stored ones against the list configured now
static int og_check_stored_pairs(nxs_dyn_handle *h, const char *who, const OutputGrid &g, int n_nod) {
    for (int k = 0; k < g.n_pairs; ++k)
        if (g.first[k] >= n_nod || g.second[k] >= n_nod)
            return fail(h, NXS_ERR_STATE, "%s: pair %d names the columns %d and %d, the nodal list configured now has %d", who, k, g.first[k], g.second[k], n_nod);
    return NXS_OK;
}

// the points (none on the regular grid: gridX == NULL), cos / sin (none: both empty) of a grid of g.G points onto the device, then the pairs and miss_val; synchronised:
// the caller's arrays, and cs / sn, may go away
static int og_upload(nxs_dyn_handle *h, OutputGrid &g, const double *gridX, const double *gridY, const std::vector<double> &cs, const std::vector<double> &sn, double miss_val, int n_pairs,
                     const int32_t *first, const int32_t *second) {
    const size_t G = (size_t)g.G;
    int rc;
    if (gridX && ((rc = dev_alloc(h, g.allocs, &g.gx, G)) || (rc = dev_alloc(h, g.allocs, &g.gy, G)))) return rc;
    if (!cs.empty() && ((rc = dev_alloc(h, g.allocs, &g.cos, G)) || (rc = dev_alloc(h, g.allocs, &g.sin, G)))) return rc;
    if (gridX) {
        HIPCHK(h, hipMemcpyAsync(g.gx, gridX, G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(g.gy, gridY, G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (!cs.empty()) {
        HIPCHK(h, hipMemcpyAsync(g.cos, cs.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(g.sin, sn.data(), G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    g.miss_val = miss_val; g.n_pairs = n_pairs;
    for (int k = 0; k < n_pairs; ++k) { g.first[k] = first[k]; g.second[k] = second[k]; }
    return NXS_OK;
}

// what the per-point arithmetic (nxs_means_points_body.inl) receives of a grid: n_el / n_nod columns of the mesh accumulators el / nod into the grid's, mask [2]
// (NULL: none) the Variable::mask flags of the two lists, ice_col the elemental column of the ice mask (-1: no rule)
static nxs_mp::Args og_args(const nxs_dyn_handle *h, const OutputGrid &g, int n_el, int n_nod, const std::vector<unsigned char> *mask, int ice_col, const double *el, const double *nod) {
    nxs_mp::Args a{};
    a.G = g.G; a.n_el = n_el; a.n_nod = n_nod; a.n_pairs = g.n_pairs;
    a.ice_col = ice_col; a.Neo = h->dm.Neo;
    if (mask) {
        for (int nv = 0; nv < n_el; ++nv) if (mask[0][nv]) a.mask_el |= 1u << nv;
        for (int nv = 0; nv < n_nod; ++nv) if (mask[1][nv]) a.mask_nod |= 1u << nv;
    }
    for (int k = 0; k < g.n_pairs; ++k) { a.first[k] = (unsigned char)g.first[k]; a.second[k] = (unsigned char)g.second[k]; }
    a.miss_val = g.miss_val;
    a.gx = g.gx; a.gy = g.gy; a.cosang = g.cos; a.sinang = g.sin;
    a.el = el; a.nod = nod;
    a.grid_el = n_el ? g.grid[0] : nullptr; a.grid_nod = g.grid[1];
    return a;
}

// The accumulators to the host arrays that were given (dst [2], either may be NULL) and the device pointers.  `behind` (may be NULL) is queued on the stream behind
// the copies; the stream is synchronised, and the launches' verdict read, when something was copied or always_sync.  apply_lsm: applyLSM (gridoutput.cpp:639-651) on
// the copy where a mask was set -- the resident rows go on accumulating
static int og_copy_out(nxs_dyn_handle *h, const OutputGrid &g, bool apply_lsm, double *const *dst, const double **elemental_dev, const double **nodal_dev, bool always_sync,
                       int (*behind)(nxs_dyn_handle *)) {
    const size_t G = (size_t)g.G;
    bool copied = false;
    for (int k = 0; k < 2; ++k) {
        const size_t bytes = G * g.grid_n[k] * sizeof(double);
        if (dst[k] && bytes) { pin_host_buffer(h, dst[k], bytes); HIPCHK(h, hipMemcpyAsync(dst[k], g.grid[k], bytes, hipMemcpyDeviceToHost, h->stream)); copied = true; }
    }
    if (behind)
        if (int rc = behind(h)) return rc;
    if (copied || always_sync) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->res_ready || h->flow_ready) { int rc = resident_error(h); if (rc) return rc; }   // (synchronised above)
    }
    if (apply_lsm && g.have_lsm)
        for (int k = 0; k < 2; ++k)
            if (dst[k])
                for (int nv = 0; nv < g.grid_n[k]; ++nv) {
                    double *row = dst[k] + (size_t)nv * G;
                    for (size_t i = 0; i < G; ++i) if (g.lsm[i] == 0) row[i] = g.miss_val;
                }
    if (elemental_dev) *elemental_dev = g.grid[0];
    if (nodal_dev) *nodal_dev = g.grid[1];
    return NXS_OK;
}

// setLSM: the mask of a grid taken over (lsm_in) or computed -- compute(d_lsm) queues on the stream what writes it into d_lsm [G] and returns the entry's status --,
// kept on the handle for applyLSM and copied out
template <class Compute>
static int og_lsm(nxs_dyn_handle *h, const char *who, OutputGrid &g, const int32_t *lsm_in, int32_t *lsm_out, Compute compute) {
    const size_t G = (size_t)g.G;
    std::vector<int32_t> lsm(G);
    if (lsm_in) std::copy(lsm_in, lsm_in + G, lsm.begin());
    else {
        if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "%s: computing the mask needs set_mesh", who);
        HIPCHK(h, hipSetDevice(h->device));
        int *d_lsm = nullptr;
        if (int rc = dev_alloc(h, g.allocs, &d_lsm, G)) return rc;
        const int rc = compute(d_lsm);
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(lsm.data(), d_lsm, G * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        pool_free_one(g.allocs, d_lsm);
        if (rc) return rc;
        HIPCHK(h, e);
        HIPCHK(h, e2);
    }
    g.lsm.swap(lsm);
    g.have_lsm = true;
    if (lsm_out) std::copy(g.lsm.begin(), g.lsm.end(), lsm_out);
    return NXS_OK;
}
