// nxs_mesh_forcing.inl -- host side of nxs_dyn_forcing_attach_mesh / _ingest_mesh and nxs_dyn_thermo_forcing_attach_mesh / _ingest_mesh (include/nxs_dyn.h): forcing
// given on a TRIANGULATED source (topaz4r_nodes, topaz4r_elements and their kin: InterpFromMeshToMesh2dx, externaldata.cpp:886-931, 944-1288, 1334-1383, 1442-1448)
// through a node map (nxs_nodemap_load_rows, include/nxs_interp.h) on the handle's stream.  Textually included by nxs_dyn.hip inside its extern "C" block, behind
// nxs_nodes_coupled.inl.  The rows ARE the snapshots nxs_dyn_set_forcing_pair owns at the nodes (nf_half_row, nxs_nodal_forcing.inl) and the snapshot rows
// nxs_dyn_thermo_forcing_pair owns at the elements (tf_snap, nxs_thermo_forcing.inl), marked as their grid counterparts mark them: the time blends are
// nxs_dyn_set_forcing_time_rows and nxs_dyn_thermo_forcing_time.  The maps are borrowed; the attachments are the MeshForcing group (release_mesh_forcing, called by
// release_mesh).  No kernel of its own.

// the checks both attachments share: the map's device and target count against the handle's
static int mf_check_map(nxs_dyn_handle *h, const char *who, int32_t set, struct nxs_nodemap *map, int want, const char *what) {
    int32_t N = 0, map_device = -1;
    if (int rc = nxs_nodemap_info(map, &N, nullptr, nullptr)) return fail(h, rc, "%s: %s", who, nxs_interp_last_error());
    if (int rc = nxs_nodemap_device(map, &map_device)) return fail(h, rc, "%s: %s", who, nxs_interp_last_error());
    if (map_device != h->device) return fail(h, NXS_ERR_INVALID, "%s: the map of set %d is on device %d, the handle on device %d", who, set, map_device, h->device);
    if (N != want) return fail(h, NXS_ERR_INVALID, "%s: the map of set %d has %d targets, the handle's mesh has %d %s (ghosts included)", who, set, N, want, what);
    return NXS_OK;
}

int nxs_dyn_forcing_attach_mesh(nxs_dyn_handle *h, int32_t set, struct nxs_nodemap *map) try {
    if (!h) return NXS_ERR_INVALID;
    if (set < 0 || set >= NF_SETS) return fail(h, NXS_ERR_INVALID, "forcing_attach_mesh: set = %d (0 .. %d)", set, NF_SETS - 1);
    if (!map) { h->mf_node_map[set] = nullptr; return NXS_OK; }   // detach: the rows that were ingested stay what they are
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "forcing_attach_mesh before set_mesh (the attachment goes with the mesh)");
    if (int rc = mf_check_map(h, "forcing_attach_mesh", set, map, h->dm.Nn, "nodes")) return rc;
    h->mf_node_map[set] = map;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_forcing_attach_mesh"); }

int nxs_dyn_thermo_forcing_attach_mesh(nxs_dyn_handle *h, int32_t set, struct nxs_nodemap *map) try {
    if (!h) return NXS_ERR_INVALID;
    if (set < 0 || set >= TF_SETS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_attach_mesh: set = %d (0 .. %d)", set, TF_SETS - 1);
    if (!map) { h->mf_elem_map[set] = nullptr; return NXS_OK; }
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_attach_mesh before set_mesh (the attachment goes with the mesh)");
    if (int rc = mf_check_map(h, "thermo_forcing_attach_mesh", set, map, h->dm.Ne, "elements")) return rc;
    h->mf_elem_map[set] = map;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_attach_mesh"); }

// the checks both ingests share, before any device work: the load's shape (its values are nxs_nodemap_load_rows's to judge), the rows, the flags
static int mf_check_ingest(nxs_dyn_handle *h, const char *who, const nxs_nodemap_load *l, const int32_t *row, int32_t flags, int nrows, const char *const *name) {
    if (l->n_var < 1 || l->n_var > NXS_NODEMAP_MAX_LOAD / 2) return fail(h, NXS_ERR_INVALID, "%s: n_var = %d (1 .. %d)", who, l->n_var, NXS_NODEMAP_MAX_LOAD / 2);
    if (l->n_step < 1 || l->n_step > 2) return fail(h, NXS_ERR_INVALID, "%s: n_step = %d (1 or 2)", who, l->n_step);
    unsigned seen = 0;
    bool any = false;
    for (int j = 0; j < l->n_var; ++j) {
        if (row[j] == -1) continue;
        if (row[j] < 0 || row[j] >= nrows) return fail(h, NXS_ERR_INVALID, "%s: variable %d goes to row %d (-1 .. %d)", who, j, row[j], nrows - 1);
        if (seen & (1u << row[j])) return fail(h, NXS_ERR_INVALID, "%s: two variables go to row %s", who, name[row[j]]);
        seen |= 1u << row[j];
        any = true;
    }
    if (!any) return fail(h, NXS_ERR_INVALID, "%s: every variable is skipped", who);
    if (flags & ~NXS_REGRID_IN_DEVICE) return fail(h, NXS_ERR_INVALID, "%s: flags = 0x%x (0 or NXS_REGRID_IN_DEVICE)", who, flags);
    return NXS_OK;
}

int nxs_dyn_forcing_ingest_mesh(nxs_dyn_handle *h, int32_t set, const nxs_nodemap_load *l, const int32_t *row, int32_t flags) try {
    if (!h || !l || !row) return NXS_ERR_INVALID;
    if (set < 0 || set >= NF_SETS) return fail(h, NXS_ERR_INVALID, "forcing_ingest_mesh: set = %d (0 .. %d)", set, NF_SETS - 1);
    if (int rc = mf_check_ingest(h, "forcing_ingest_mesh", l, row, flags, NF_ROWS, nf_name)) return rc;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "forcing_ingest_mesh before set_mesh");
    if (!h->mf_node_map[set])
        return fail(h, NXS_ERR_STATE, "forcing_ingest_mesh: set %d has no node map on this mesh (nxs_dyn_forcing_attach_mesh after set_mesh / regrid)", set);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    if (int rc = nf_ensure_snapshots(h)) return rc;
    double *out[NXS_NODEMAP_MAX_LOAD] = {};
    unsigned seen = 0;
    for (int s = 0; s < l->n_step; ++s)
        for (int j = 0; j < l->n_var; ++j)
            if (row[j] >= 0) { out[s * l->n_var + j] = nf_half_row(h, s, row[j]); seen |= nf_bit(s, row[j]); }
    if (int rc = nxs_nodemap_load_rows(h->mf_node_map[set], l, out, (flags & NXS_REGRID_IN_DEVICE) | NXS_REGRID_OUT_DEVICE, (void *)h->stream))
        return fail(h, rc, "forcing_ingest_mesh: %s", nxs_interp_last_error());
    h->f_have |= seen;   // as nxs_dyn_forcing_ingest marks them
    if (h->f_have == NF_ALL_HALF_ROWS) h->have_pair = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_forcing_ingest_mesh"); }

int nxs_dyn_thermo_forcing_ingest_mesh(nxs_dyn_handle *h, int32_t set, const nxs_nodemap_load *l, const int32_t *row, int32_t flags) try {
    if (!h || !l || !row) return NXS_ERR_INVALID;
    if (set < 0 || set >= TF_SETS) return fail(h, NXS_ERR_INVALID, "thermo_forcing_ingest_mesh: set = %d (0 .. %d)", set, TF_SETS - 1);
    if (int rc = mf_check_ingest(h, "thermo_forcing_ingest_mesh", l, row, flags, TF_ROWS, tf_name)) return rc;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "thermo_forcing_ingest_mesh before set_mesh");
    if (!h->mf_elem_map[set])
        return fail(h, NXS_ERR_STATE, "thermo_forcing_ingest_mesh: set %d has no node map on this mesh (nxs_dyn_thermo_forcing_attach_mesh after set_mesh / regrid)", set);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    double *out[NXS_NODEMAP_MAX_LOAD] = {};
    unsigned seen[2] = {0, 0};
    for (int s = 0; s < l->n_step; ++s)
        for (int j = 0; j < l->n_var; ++j) {
            if (row[j] < 0) continue;
            double **dst = &h->tf_snap[s][row[j]];   // the rows nxs_dyn_thermo_forcing_pair owns, made here when never given
            if (!*dst) { if (int rc = dev_alloc(h, h->tf_allocs, dst, (size_t)h->dm.Ne)) return rc; }
            out[s * l->n_var + j] = *dst;
            seen[s] |= 1u << row[j];
        }
    if (int rc = nxs_nodemap_load_rows(h->mf_elem_map[set], l, out, (flags & NXS_REGRID_IN_DEVICE) | NXS_REGRID_OUT_DEVICE, (void *)h->stream))
        return fail(h, rc, "thermo_forcing_ingest_mesh: %s", nxs_interp_last_error());
    h->tf_have[0] |= seen[0]; h->tf_have[1] |= seen[1];
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_thermo_forcing_ingest_mesh"); }
