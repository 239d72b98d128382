// nxs_ocean_coupled.inl -- host side of nxs_ocean_coupled_* / nxs_dyn_ocean_coupled_* (include/nxs_dyn.h): the attachment of a coupled ocean (the reference's
// OceanType::COUPLED, #ifdef OASIS) and the way of its received element fields onto the rows thermo() reads.  Textually included by nxs_dyn.hip inside its
// extern "C" block.  The receive is ONE launch of nxs_gridmap_receive_rows (nxs_gridmap_kernels.inl) on the handle's stream; the three guarded statements are in
// k_fluxes (FE.cpp:5150-5157), k_column (5348-5358) and slab_element (5826-5841), switched by ocean_coupled_on(h).  FE.cpp = model/finiteelement.cpp.

static const char *const oc_row_name[NXS_OC_ROWS] = {"ocean_temp", "ocean_salt", "qsrml", "mld", "wlbk"};

int nxs_ocean_coupled_default_config(nxs_dyn_ocean_coupled_config *c) try {   // dataset.cpp:2828-3031 with coupler.rcv_first_layer_depth off, and no wave model
    if (!c) return NXS_ERR_INVALID;
    *c = nxs_dyn_ocean_coupled_config{};
    c->n_fields = 3;
    c->row[0] = NXS_OC_OCEAN_TEMP; c->row[1] = NXS_OC_OCEAN_SALT; c->row[2] = NXS_OC_QSRML;   // I_SST, I_SSS, I_FrcQsr
    for (int k = 0; k < NXS_OC_ROWS; ++k) { c->a[k] = 1.; c->b[k] = 0.; c->factor[k] = 1.; c->bias[k] = 0.; }
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_ocean_coupled_default_config"); }

// what nxs_dyn_ocean_coupled_attach refuses in a configuration; *rows (may be NULL) = the mask of the rows it names
static int oc_config_check(nxs_dyn_handle *h, const nxs_dyn_ocean_coupled_config *c, unsigned *rows) {
    if (!c) return fail(h, NXS_ERR_INVALID, "ocean_coupled: no configuration");
    if (c->n_fields < 1 || c->n_fields > NXS_OC_ROWS) return fail(h, NXS_ERR_INVALID, "ocean_coupled: n_fields = %d (1 .. %d)", c->n_fields, (int)NXS_OC_ROWS);
    unsigned mask = 0;
    for (int k = 0; k < c->n_fields; ++k) {
        if (c->row[k] < 0 || c->row[k] >= NXS_OC_ROWS) return fail(h, NXS_ERR_INVALID, "ocean_coupled: field %d goes to the unknown row %d", k, c->row[k]);
        if (mask & (1u << c->row[k])) return fail(h, NXS_ERR_INVALID, "ocean_coupled: field %d goes to %s, which an earlier field fills already", k, oc_row_name[c->row[k]]);
        mask |= 1u << c->row[k];
    }
    if (rows) *rows = mask;
    return NXS_OK;
}

int nxs_ocean_coupled_config_check(const nxs_dyn_ocean_coupled_config *c) try {
    return oc_config_check(nullptr, c, nullptr);
} catch (...) { return dyn_caught(nullptr, "nxs_ocean_coupled_config_check"); }

int nxs_dyn_ocean_coupled_attach(nxs_dyn_handle *h, struct nxs_gridmap *map, const nxs_dyn_ocean_coupled_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (!c) {   // detach: the handle is again the library without this section
        if (h->oc_attached || !h->oc_allocs.empty()) {
            HIPCHK(h, hipSetDevice(h->device));
            if (h->stream && !h->oc_allocs.empty()) HIPCHK(h, hipStreamSynchronize(h->stream));   // (a launch may still be reading the two rows)
            release_ocean_coupled(h);
        }
        return NXS_OK;
    }
    unsigned rows = 0;
    if (int rc = oc_config_check(h, c, &rows)) return rc;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "ocean_coupled_attach before set_mesh (the attachment goes with the mesh)");
    if (map) {
        int32_t map_nels = 0;
        if (int rc = nxs_gridmap_info(map, nullptr, nullptr, nullptr, nullptr, &map_nels, nullptr)) return fail(h, rc, "ocean_coupled_attach: %s", nxs_interp_last_error());
        if (map_nels != h->dm.Ne)
            return fail(h, NXS_ERR_INVALID, "ocean_coupled_attach: the map is of a mesh of %d elements, the handle's has %d (a partitioned run passes the nxs_gridmap_restrict-ed map)",
                        map_nels, h->dm.Ne);
    }
    h->oc_attached = true; h->oc_map = map; h->oc_cfg = *c; h->oc_rows = rows;   // (rows given under an earlier attachment on this mesh stay present)
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_ocean_coupled_attach"); }

// the device row NXS_OC_* k, made when first wanted: ocean_temp, ocean_salt and mld are the column's forcing rows (state pool), qsrml and wlbk the attachment's own
static int oc_row(nxs_dyn_handle *h, int k, double **out) {
    double **slot = k == NXS_OC_QSRML ? &h->d_oc_qsrml : k == NXS_OC_WLBK ? &h->d_oc_wlbk : &h->d_col_forcing[k == NXS_OC_MLD ? 4 : 2 + k];
    if (!*slot) { if (int rc = dev_alloc(h, (k == NXS_OC_QSRML || k == NXS_OC_WLBK) ? h->oc_allocs : h->state_allocs, slot, (size_t)h->dm.Ne)) return rc; }
    *out = *slot;
    return NXS_OK;
}
static void oc_mark(nxs_dyn_handle *h, int k) {
    if (k == NXS_OC_QSRML || k == NXS_OC_WLBK) h->oc_have |= 1u << k;
    else h->col_forcing_have |= 1u << (k == NXS_OC_MLD ? 4 : 2 + k);   // as after nxs_dyn_column_set_forcing
}
static bool oc_present(const nxs_dyn_handle *h, int k) {
    if (k == NXS_OC_QSRML || k == NXS_OC_WLBK) return (h->oc_have >> k) & 1u;
    return (h->col_forcing_have >> (k == NXS_OC_MLD ? 4 : 2 + k)) & 1u;
}

int nxs_dyn_ocean_coupled_receive(nxs_dyn_handle *h, const double *const *fields, int32_t flags) try {
    if (!h || !fields) return NXS_ERR_INVALID;
    if (!h->oc_attached) return fail(h, NXS_ERR_STATE, "ocean_coupled_receive: no coupled ocean is attached on this mesh (nxs_dyn_ocean_coupled_attach after set_mesh / regrid)");
    if (!h->oc_map) return fail(h, NXS_ERR_STATE, "ocean_coupled_receive: the coupled ocean was attached without a map (nxs_dyn_ocean_coupled_put_rows is its way in)");
    if (flags & ~NXS_REGRID_IN_DEVICE) return fail(h, NXS_ERR_INVALID, "ocean_coupled_receive: flags = 0x%x (0 or NXS_REGRID_IN_DEVICE)", flags);
    const nxs_dyn_ocean_coupled_config &c = h->oc_cfg;
    for (int k = 0; k < c.n_fields; ++k)
        if (!fields[k]) return fail(h, NXS_ERR_INVALID, "ocean_coupled_receive: field %d (%s) is NULL", k, oc_row_name[c.row[k]]);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    double *out[NXS_OC_ROWS] = {};
    for (int k = 0; k < c.n_fields; ++k) { if (int rc = oc_row(h, c.row[k], &out[k])) return rc; }
    if (int rc = nxs_gridmap_receive_rows(h->oc_map, c.n_fields, fields, c.a, c.b, c.factor, c.bias, out, (flags & NXS_REGRID_IN_DEVICE) | NXS_REGRID_OUT_DEVICE, (void *)h->stream))
        return fail(h, rc, "ocean_coupled_receive: %s", nxs_interp_last_error());
    for (int k = 0; k < c.n_fields; ++k) oc_mark(h, c.row[k]);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_ocean_coupled_receive"); }

int nxs_dyn_ocean_coupled_put_rows(nxs_dyn_handle *h, const nxs_dyn_ocean_coupled_rows *r) try {
    if (!h || !r) return NXS_ERR_INVALID;
    if (!h->oc_attached) return fail(h, NXS_ERR_STATE, "ocean_coupled_put_rows: no coupled ocean is attached on this mesh (nxs_dyn_ocean_coupled_attach after set_mesh / regrid)");
    for (int k = 0; k < NXS_OC_ROWS; ++k)
        if (r->row[k] && !(h->oc_rows & (1u << k))) return fail(h, NXS_ERR_INVALID, "ocean_coupled_put_rows: %s is not a row of the attached configuration", oc_row_name[k]);
    HIPCHK(h, hipSetDevice(h->device));
    RowCopy rows[NXS_OC_ROWS];
    for (int k = 0; k < NXS_OC_ROWS; ++k) {
        double *dev = nullptr;
        if (r->row[k]) { if (int rc = oc_row(h, k, &dev)) return rc; }
        rows[k] = RowCopy{dev, r->row[k], (size_t)h->dm.Ne * sizeof(double), oc_row_name[k]};
    }
    if (int rc = copy_rows(h, rows, NXS_OC_ROWS, hipMemcpyHostToDevice)) return rc;
    for (int k = 0; k < NXS_OC_ROWS; ++k) if (r->row[k]) oc_mark(h, k);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_ocean_coupled_put_rows"); }

int nxs_dyn_ocean_coupled_get(nxs_dyn_handle *h, const nxs_dyn_ocean_coupled_rows *out, const double **device_rows) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->oc_attached) return fail(h, NXS_ERR_STATE, "ocean_coupled_get: no coupled ocean is attached on this mesh");
    const double *row[NXS_OC_ROWS];
    for (int k = 0; k < NXS_OC_ROWS; ++k) {
        const bool here = oc_present(h, k);
        if (out && out->row[k] && !here) return fail(h, NXS_ERR_STATE, "ocean_coupled_get: %s was never received or put on this mesh", oc_row_name[k]);
        row[k] = !here ? nullptr : k == NXS_OC_QSRML ? h->d_oc_qsrml : k == NXS_OC_WLBK ? h->d_oc_wlbk : h->d_col_forcing[k == NXS_OC_MLD ? 4 : 2 + k];
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (device_rows) std::copy(row, row + NXS_OC_ROWS, device_rows);
    std::vector<RowCopy> rows(NXS_OC_ROWS);
    for (int k = 0; k < NXS_OC_ROWS; ++k) rows[k] = RowCopy{out ? out->row[k] : nullptr, row[k], (size_t)h->dm.Ne * sizeof(double), oc_row_name[k]};
    return copy_rows(h, rows.data(), NXS_OC_ROWS, hipMemcpyDeviceToHost);   // synchronised: what a launch on the handle's stream wrote is in the rows
} catch (...) { return dyn_caught(h, "nxs_dyn_ocean_coupled_get"); }
