// nxs_nodes_coupled.inl -- host side of nxs_dyn_nodes_coupled_* (include/nxs_dyn.h): the nodal half of a coupled run's receive -- I_Uocn, I_Vocn, I_SSH of
// ocean_cpl_nodes and I_tauwix, I_tauwiy of wave_cpl_nodes -- through a node map (nxs_nodemap_*, include/nxs_interp.h) on the handle's stream.  Textually included
// by nxs_dyn.hip inside its extern "C" block, behind nxs_ocean_coupled.inl.  The ocean's three rows ARE snapshot 0 of the half-rows nxs_dyn_set_forcing_pair owns
// (nxs_nodal_forcing.inl), stored raw: nxs_dyn_set_forcing_time_rows with NXS_TF_STEP is then ExternalData::get (externaldata.cpp:434, 438).  The wave stress is
// the handle's M_tau_wi, attached as nxs_dyn_set_wave_stress attaches it (wave_stress_buffer / wave_stress_attach).  No kernel of its own.

static const char *const nc_name[NXS_NC_DATASETS] = {"ocean_cpl_nodes", "wave_cpl_nodes"};
static const int nc_fields[NXS_NC_DATASETS] = {3, 2};   // I_Uocn, I_Vocn, I_SSH; I_tauwix, I_tauwiy
static const char *const nc_field_name[NXS_NC_DATASETS][3] = {{"I_Uocn", "I_Vocn", "I_SSH"}, {"I_tauwix", "I_tauwiy", ""}};

int nxs_nodes_coupled_default_config(nxs_dyn_nodes_coupled_config *c) try {
    if (!c) return NXS_ERR_INVALID;
    *c = nxs_dyn_nodes_coupled_config{};
    for (int k = 0; k < NXS_NC_MAX_FIELDS; ++k) { c->a[k] = 1.; c->b[k] = 0.; c->factor[k] = 1.; c->bias[k] = 0.; }
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_nodes_coupled_default_config"); }

int nxs_dyn_nodes_coupled_attach(nxs_dyn_handle *h, int32_t which, struct nxs_nodemap *map, const nxs_dyn_nodes_coupled_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (which != NXS_NC_OCEAN && which != NXS_NC_WAVE) return fail(h, NXS_ERR_INVALID, "nodes_coupled_attach: which = %d (NXS_NC_OCEAN, NXS_NC_WAVE)", which);
    if (!c) {   // detach: the rows that were received stay what they are (snapshots of the forcing pair, M_tau_wi)
        h->nc_attached[which] = false; h->nc_map[which] = nullptr;
        return NXS_OK;
    }
    if (!map) return fail(h, NXS_ERR_INVALID, "nodes_coupled_attach: %s needs a node map", nc_name[which]);
    for (int k = 0; k < nc_fields[which]; ++k)
        if (!std::isfinite(c->a[k]) || !std::isfinite(c->b[k]) || !std::isfinite(c->factor[k]) || !std::isfinite(c->bias[k]))
            return fail(h, NXS_ERR_INVALID, "nodes_coupled_attach: a, b, factor or bias of %s is not finite", nc_field_name[which][k]);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "nodes_coupled_attach before set_mesh (the attachment goes with the mesh)");
    int32_t N = 0;
    if (int rc = nxs_nodemap_info(map, &N, nullptr, nullptr)) return fail(h, rc, "nodes_coupled_attach: %s", nxs_interp_last_error());
    int32_t map_device = -1;
    if (int rc = nxs_nodemap_device(map, &map_device)) return fail(h, rc, "nodes_coupled_attach: %s", nxs_interp_last_error());
    if (map_device != h->device)
        return fail(h, NXS_ERR_INVALID, "nodes_coupled_attach: the map of %s is on device %d, the handle on device %d", nc_name[which], map_device, h->device);
    if (N != h->dm.Nn)
        return fail(h, NXS_ERR_INVALID, "nodes_coupled_attach: the map of %s has %d targets, the handle's mesh has %d nodes (ghosts included)", nc_name[which], N, h->dm.Nn);
    h->nc_attached[which] = true; h->nc_map[which] = map; h->nc_cfg[which] = *c;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nodes_coupled_attach"); }

int nxs_dyn_nodes_coupled_receive(nxs_dyn_handle *h, int32_t which, const double *const *fields, int32_t n_fields, int32_t flags) try {
    if (!h || !fields) return NXS_ERR_INVALID;
    if (which != NXS_NC_OCEAN && which != NXS_NC_WAVE) return fail(h, NXS_ERR_INVALID, "nodes_coupled_receive: which = %d (NXS_NC_OCEAN, NXS_NC_WAVE)", which);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "nodes_coupled_receive before set_mesh");
    if (!h->nc_attached[which])
        return fail(h, NXS_ERR_STATE, "nodes_coupled_receive: no %s is attached on this mesh (nxs_dyn_nodes_coupled_attach after set_mesh / regrid)", nc_name[which]);
    if (n_fields != nc_fields[which]) return fail(h, NXS_ERR_INVALID, "nodes_coupled_receive: %s has %d fields, %d were given", nc_name[which], nc_fields[which], n_fields);
    if (flags & ~NXS_REGRID_IN_DEVICE) return fail(h, NXS_ERR_INVALID, "nodes_coupled_receive: flags = 0x%x (0 or NXS_REGRID_IN_DEVICE)", flags);
    for (int k = 0; k < n_fields; ++k)
        if (!fields[k]) return fail(h, NXS_ERR_INVALID, "nodes_coupled_receive: field %d (%s) is NULL", k, nc_field_name[which][k]);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    const nxs_dyn_nodes_coupled_config &c = h->nc_cfg[which];
    const int32_t pairs[NXS_NC_MAX_FIELDS] = {1, -1, -1};   // (I_Uocn, I_Vocn) and (I_tauwix, I_tauwiy)
    double *out[NXS_NC_MAX_FIELDS] = {};
    int get = 0;
    const bool was = wave_attached(h);
    if (which == NXS_NC_OCEAN) {
        if (int rc = nf_ensure_snapshots(h)) return rc;
        out[0] = nf_half_row(h, 0, NXS_NF_OCEAN_U); out[1] = nf_half_row(h, 0, NXS_NF_OCEAN_V); out[2] = nf_half_row(h, 0, NXS_NF_SSH);
    } else {
        if (int rc = wave_stress_buffer(h)) return rc;
        out[0] = h->d_tau_wi; out[1] = h->d_tau_wi + h->dm.Nn;
        get = NXS_NODEMAP_GET;
    }
    if (int rc = nxs_nodemap_receive_rows(h->nc_map[which], n_fields, fields, c.a, c.b, pairs, c.factor, c.bias, out, (flags & NXS_REGRID_IN_DEVICE) | NXS_REGRID_OUT_DEVICE | get,
                                          (void *)h->stream))
        return fail(h, rc, "nodes_coupled_receive: %s", nxs_interp_last_error());
    if (which == NXS_NC_OCEAN) {
        h->f_have |= nf_bit(0, NXS_NF_OCEAN_U) | nf_bit(0, NXS_NF_OCEAN_V) | nf_bit(0, NXS_NF_SSH);   // as nxs_dyn_forcing_ingest marks them
        if (h->f_have == NF_ALL_HALF_ROWS) h->have_pair = true;
    } else {
        if (!was) HIPCHK(h, hipStreamSynchronize(h->stream));   // (the first attachment drops the step's graphs, as nxs_dyn_set_wave_stress does behind its own synchronisation)
        wave_stress_attach(h, was);
    }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nodes_coupled_receive"); }

int nxs_dyn_nodes_coupled_get(nxs_dyn_handle *h, int32_t which, double *const *out, const double **device_rows) try {
    if (!h) return NXS_ERR_INVALID;
    if (which != NXS_NC_OCEAN && which != NXS_NC_WAVE) return fail(h, NXS_ERR_INVALID, "nodes_coupled_get: which = %d (NXS_NC_OCEAN, NXS_NC_WAVE)", which);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "nodes_coupled_get before set_mesh");
    if (!h->nc_attached[which]) return fail(h, NXS_ERR_STATE, "nodes_coupled_get: no %s is attached on this mesh", nc_name[which]);
    const double *row[NXS_NC_MAX_FIELDS] = {};
    if (which == NXS_NC_OCEAN) {
        const int r[3] = {NXS_NF_OCEAN_U, NXS_NF_OCEAN_V, NXS_NF_SSH};
        for (int k = 0; k < 3; ++k) {
            if (!(h->f_have & nf_bit(0, r[k]))) return fail(h, NXS_ERR_STATE, "nodes_coupled_get: %s was never received on this mesh", nc_field_name[which][k]);
            row[k] = nf_half_row(h, 0, r[k]);
        }
    } else {
        if (!wave_attached(h) || !h->d_tau_wi) return fail(h, NXS_ERR_STATE, "nodes_coupled_get: no wave stress was received on this mesh");
        row[0] = h->d_tau_wi; row[1] = h->d_tau_wi + h->dm.Nn;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (device_rows) std::copy(row, row + nc_fields[which], device_rows);
    RowCopy rows[NXS_NC_MAX_FIELDS];
    for (int k = 0; k < nc_fields[which]; ++k) rows[k] = RowCopy{out ? out[k] : nullptr, row[k], (size_t)h->dm.Nn * sizeof(double), nc_field_name[which][k]};
    return copy_rows(h, rows, nc_fields[which], hipMemcpyDeviceToHost);   // synchronised: what the receive on the handle's stream wrote is in the rows
} catch (...) { return dyn_caught(h, "nxs_dyn_nodes_coupled_get"); }
