// nxs_nesting.inl -- host side of nxs_dyn_nesting_* and nxs_dyn_diffusion_configure / nxs_dyn_diffuse (include/nxs_dyn.h; the kernels are in
// nxs_nesting_kernels.inl).  Textually included by nxs_dyn.hip inside its extern "C" block, behind nxs_thermo_forcing.inl.  The pools are the Nesting and the
// Diffusion group (release_nesting, release_diffusion, called by release_mesh): after nxs_dyn_set_mesh and nxs_dyn_regrid every snapshot is missing again and the
// element-to-element table is built again by the next nxs_dyn_diffuse.  FE.cpp = model/finiteelement.cpp.

static const char *const nest_el_name[NEST_EL_ROWS] = {"dist", "thick", "conc", "snow_thick", "h_young", "conc_young", "hs_young", "sigma1", "sigma2", "sigma3", "damage", "ridge_ratio"};
static const char *const nest_nd_name[NEST_ND_ROWS] = {"dist_nodes", "VT1", "VT2"};
static const char *const nest_ds_name[NEST_DATASETS] = {"distance_elements", "ice_elements", "dynamics_elements", "distance_nodes", "nodes"};

// what nxs_dyn_nesting_configure refuses; the text goes where nxs_dyn_last_error(h) finds it (h == NULL: the thread's create error)
static int nesting_config_check(nxs_dyn_handle *h, const nxs_dyn_nesting_config *c) {
    if (!c) return fail(h, NXS_ERR_INVALID, "nesting_configure: no configuration");
    if (c->nudge_function != NXS_NUDGE_LINEAR && c->nudge_function != NXS_NUDGE_EXPONENTIAL)
        return fail(h, NXS_ERR_INVALID, "nesting_configure: nudge_function = %d not known: use exponential or linear (FE.cpp:4886-4888)", c->nudge_function);
    if (!std::isfinite(c->nudge_timescale) || !(c->nudge_timescale > 0.)) return fail(h, NXS_ERR_INVALID, "nesting_configure: nudge_timescale = %g must be positive and finite", c->nudge_timescale);
    if (!std::isfinite(c->nudge_scale) || !(c->nudge_scale > 0.)) return fail(h, NXS_ERR_INVALID, "nesting_configure: nudge_scale = %g must be positive and finite", c->nudge_scale);
    if (!std::isfinite(c->dtime_step)) return fail(h, NXS_ERR_INVALID, "nesting_configure: dtime_step = %g must be finite", c->dtime_step);
    return NXS_OK;
}

int nxs_nesting_config_check(const nxs_dyn_nesting_config *c) try {
    return nesting_config_check(nullptr, c);
} catch (...) { return dyn_caught(nullptr, "nxs_nesting_config_check"); }

int nxs_dyn_nesting_configure(nxs_dyn_handle *h, const nxs_dyn_nesting_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (int rc = nesting_config_check(h, c)) return rc;
    h->nest_cfg = *c;
    h->nest_q = c->time_step / c->nudge_timescale;      // (time_step/nudge_time): the int converted to double (FE.cpp:4897)
    h->nest_qvt = c->dtime_step / c->nudge_timescale;   // (dtime_step/nudge_time) (FE.cpp:4954)
    h->nest_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_configure"); }

int nxs_dyn_nesting_pair(nxs_dyn_handle *h, const nxs_dyn_nesting_rows *s0, const nxs_dyn_nesting_rows *s1) try {
    if (!h || !s0) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "nesting_pair before set_mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne, Nn = h->dm.Nn;
    const nxs_dyn_nesting_rows *snap[2] = {s0, s1};
    RowCopy rows[2 * (NEST_EL_ROWS + NEST_ND_ROWS)];
    int n = 0;
    for (int s = 0; s < 2; ++s) {
        if (!snap[s]) continue;
        for (int k = 0; k < NEST_EL_ROWS; ++k) {
            if (!snap[s]->element[k]) continue;
            if (!h->nest_el[s][k]) { if (int rc = dev_alloc(h, h->nest_allocs, &h->nest_el[s][k], Ne)) return rc; }
            rows[n++] = RowCopy{h->nest_el[s][k], snap[s]->element[k], Ne * sizeof(double), nest_el_name[k]};
        }
        for (int k = 0; k < NEST_ND_ROWS; ++k) {
            if (!snap[s]->node[k]) continue;
            if (!h->nest_nd[s][k]) { if (int rc = dev_alloc(h, h->nest_allocs, &h->nest_nd[s][k], Nn)) return rc; }
            rows[n++] = RowCopy{h->nest_nd[s][k], snap[s]->node[k], Nn * sizeof(double), nest_nd_name[k]};
        }
    }
    if (int rc = copy_rows(h, rows, n, hipMemcpyHostToDevice)) return rc;
    for (int s = 0; s < 2; ++s) {
        if (!snap[s]) continue;
        for (int k = 0; k < NEST_EL_ROWS; ++k) if (snap[s]->element[k]) h->nest_el_have[s] |= 1u << k;
        for (int k = 0; k < NEST_ND_ROWS; ++k) if (snap[s]->node[k]) h->nest_nd_have[s] |= 1u << k;
    }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_pair"); }

int nxs_dyn_nesting_time(nxs_dyn_handle *h, const struct nxs_dyn_nesting_time *t) try {   // ExternalData::get, externaldata.cpp:366-438
    if (!h || !t) return NXS_ERR_INVALID;
    for (int k = 0; k < NEST_DATASETS; ++k)
        if (t->mode[k] != NXS_TF_OFF && t->mode[k] != NXS_TF_LINEAR && t->mode[k] != NXS_TF_STEP)
            return fail(h, NXS_ERR_INVALID, "nesting_time: unknown mode %d of dataset %s", t->mode[k], nest_ds_name[k]);
    for (int k = 0; k < NEST_DATASETS; ++k) h->nest_time[k] = NestTime{t->fcoeff0[k], t->fcoeff1[k], t->factor[k], t->bias[k], t->mode[k]};
    h->nest_timed = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_time"); }

// the checks the two launches share
static int nesting_ready(nxs_dyn_handle *h, const char *what) {
    if (!h) return NXS_ERR_INVALID;
    if (!h->nest_configured) return fail(h, NXS_ERR_STATE, "%s before nxs_dyn_nesting_configure", what);
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "%s needs set_mesh and put_state", what);
    if (!h->nest_timed) return fail(h, NXS_ERR_STATE, "%s before nxs_dyn_nesting_time", what);
    return NXS_OK;
}
// one variable of dataset ds as the kernels read it: both snapshots under LINEAR, snapshot 0 under STEP
static int nesting_row(nxs_dyn_handle *h, const char *what, int ds, bool nodal, int k, NestRow *out) {
    const int mode = h->nest_time[ds].mode;
    const char *name = nodal ? nest_nd_name[k] : nest_el_name[k];
    if (mode == NXS_TF_OFF) return fail(h, NXS_ERR_STATE, "%s reads row %s and its dataset %s is OFF (nxs_dyn_nesting_time)", what, name, nest_ds_name[ds]);
    const unsigned bit = 1u << k, have0 = nodal ? h->nest_nd_have[0] : h->nest_el_have[0], have1 = nodal ? h->nest_nd_have[1] : h->nest_el_have[1];
    if (!(have0 & bit)) return fail(h, NXS_ERR_STATE, "%s: snapshot 0 of row %s is missing on this mesh (nxs_dyn_nesting_pair after set_mesh / regrid)", what, name);
    if (mode == NXS_TF_LINEAR && !(have1 & bit))
        return fail(h, NXS_ERR_STATE, "%s: row %s is LINEAR and its snapshot 1 is missing on this mesh (nxs_dyn_nesting_pair after set_mesh / regrid)", what, name);
    double *const *s0 = nodal ? h->nest_nd[0] : h->nest_el[0], *const *s1 = nodal ? h->nest_nd[1] : h->nest_el[1];
    *out = NestRow{s0[k], mode == NXS_TF_LINEAR ? s1[k] : nullptr};
    return NXS_OK;
}

int nxs_dyn_nesting_ice(nxs_dyn_handle *h) try {   // nestingIce(), FE.cpp:4878-4908
    if (int rc = nesting_ready(h, "nesting_ice")) return rc;
    NestIce a{};
    a.Ne = h->dm.Ne; a.fn = h->nest_cfg.nudge_function; a.scale = h->nest_cfg.nudge_scale; a.q = h->nest_q;
    a.nfields = h->dp.young_cat ? 6 : 3;
    a.t_dist = h->nest_time[NXS_NEST_DS_DISTANCE_ELEMENTS]; a.t_ice = h->nest_time[NXS_NEST_DS_ICE_ELEMENTS];
    if (int rc = nesting_row(h, "nesting_ice", NXS_NEST_DS_DISTANCE_ELEMENTS, false, NXS_NEST_DIST, &a.dist)) return rc;
    // in the order of the reference's statements: M_conc, M_thick, M_snow_thick; M_conc_young, M_h_young, M_hs_young
    static const int row[NEST_ICE_FIELDS] = {NXS_NEST_CONC, NXS_NEST_THICK, NXS_NEST_SNOW_THICK, NXS_NEST_CONC_YOUNG, NXS_NEST_H_YOUNG, NXS_NEST_HS_YOUNG};
    double *const x[NEST_ICE_FIELDS] = {h->ds.conc, h->ds.thick, h->ds.snow, h->ds.cyoung, h->ds.hyoung, h->ds.hsyoung};
    for (int f = 0; f < a.nfields; ++f) {
        if (int rc = nesting_row(h, "nesting_ice", NXS_NEST_DS_ICE_ELEMENTS, false, row[f], &a.snap[f])) return rc;
        a.x[f] = x[f];
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    hipLaunchKernelGGL(k_nesting_ice, dim3(nblocks((a.Ne + 1) / 2)), dim3(BLOCK), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_ice"); }

int nxs_dyn_nesting_dynamics(nxs_dyn_handle *h) try {   // nestingDynamics(), FE.cpp:4915-4958
    if (int rc = nesting_ready(h, "nesting_dynamics")) return rc;
    if (!h->nest_cfg.nest_dynamic_vars) return fail(h, NXS_ERR_STATE, "nesting_dynamics: nest_dynamic_vars is 0 in the configuration (nxs_dyn_nesting_configure)");
    NestDyn a{};
    a.Ne = h->dm.Ne; a.Nn = h->dm.Nn; a.fn = h->nest_cfg.nudge_function; a.scale = h->nest_cfg.nudge_scale; a.q = h->nest_q; a.qvt = h->nest_qvt;
    a.t_dist = h->nest_time[NXS_NEST_DS_DISTANCE_ELEMENTS]; a.t_dyn = h->nest_time[NXS_NEST_DS_DYNAMICS_ELEMENTS];
    a.t_dist_n = h->nest_time[NXS_NEST_DS_DISTANCE_NODES]; a.t_nodes = h->nest_time[NXS_NEST_DS_NODES];
    const char *what = "nesting_dynamics";
    if (int rc = nesting_row(h, what, NXS_NEST_DS_DISTANCE_ELEMENTS, false, NXS_NEST_DIST, &a.dist)) return rc;
    for (int k = 0; k < 3; ++k) { if (int rc = nesting_row(h, what, NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_SIGMA1 + k, &a.sig[k])) return rc; }
    if (int rc = nesting_row(h, what, NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_DAMAGE, &a.dmg)) return rc;
    if (int rc = nesting_row(h, what, NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_RIDGE_RATIO, &a.ridge)) return rc;
    if (int rc = nesting_row(h, what, NXS_NEST_DS_DISTANCE_NODES, true, NXS_NEST_DIST_NODES, &a.dist_n)) return rc;
    for (int k = 0; k < 2; ++k) { if (int rc = nesting_row(h, what, NXS_NEST_DS_NODES, true, NXS_NEST_VT1 + k, &a.vt[k])) return rc; }
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    // M_sigma / M_damage where they are current (no ensure_arrays: that would be an unpack now and a pack in the next step); under EVP / mEVP the records' fourth
    // slot is not the damage
    a.rec = h->sig_loc ? 1 : 0;
    a.dmg_rec = (h->sig_loc && h->dp.dynamics_type == NXS_DYN_BBM) ? 1 : 0;
    a.S4 = h->ds.S4a; a.s[0] = h->ds.s0; a.s[1] = h->ds.s1; a.s[2] = h->ds.s2; a.damage = h->ds.damage; a.ridge_x = h->ds.ridge; a.VT = h->ds.VT;
    hipLaunchKernelGGL(k_nesting_dynamics, dim3(nblocks((std::max(a.Ne, a.Nn) + 1) / 2)), dim3(BLOCK), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_dynamics"); }

int nxs_dyn_nesting_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_nesting_rows *out) try {
    if (!h || !out) return NXS_ERR_INVALID;
    if (which < 0 || which > 1) return fail(h, NXS_ERR_INVALID, "nesting_get: which = %d (0, 1: the snapshots)", which);
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "nesting_get before set_mesh");
    RowCopy rows[NEST_EL_ROWS + NEST_ND_ROWS];
    int n = 0;
    for (int k = 0; k < NEST_EL_ROWS; ++k) {
        if (!out->element[k]) continue;
        if (!((h->nest_el_have[which] >> k) & 1u)) return fail(h, NXS_ERR_STATE, "nesting_get: row %s of snapshot %d is missing on this mesh", nest_el_name[k], which);
        rows[n++] = RowCopy{out->element[k], h->nest_el[which][k], (size_t)h->dm.Ne * sizeof(double), nest_el_name[k]};
    }
    for (int k = 0; k < NEST_ND_ROWS; ++k) {
        if (!out->node[k]) continue;
        if (!((h->nest_nd_have[which] >> k) & 1u)) return fail(h, NXS_ERR_STATE, "nesting_get: row %s of snapshot %d is missing on this mesh", nest_nd_name[k], which);
        rows[n++] = RowCopy{out->node[k], h->nest_nd[which][k], (size_t)h->dm.Nn * sizeof(double), nest_nd_name[k]};
    }
    HIPCHK(h, hipSetDevice(h->device));
    return copy_rows(h, rows, n, hipMemcpyDeviceToHost);
} catch (...) { return dyn_caught(h, "nxs_dyn_nesting_get"); }

// ---- diffuse(), FE.cpp:2760-2815
int nxs_dyn_diffusion_configure(nxs_dyn_handle *h, double diffusivity_sst, double diffusivity_sss, double dx, double dtime_step) try {
    if (!h) return NXS_ERR_INVALID;
    if (!std::isfinite(diffusivity_sst)) return fail(h, NXS_ERR_INVALID, "diffusion_configure: diffusivity_sst = %g must be finite", diffusivity_sst);
    if (!std::isfinite(diffusivity_sss)) return fail(h, NXS_ERR_INVALID, "diffusion_configure: diffusivity_sss = %g must be finite", diffusivity_sss);
    if (!std::isfinite(dx) || !(dx > 0.)) return fail(h, NXS_ERR_INVALID, "diffusion_configure: dx = %g must be positive and finite", dx);
    if (!std::isfinite(dtime_step)) return fail(h, NXS_ERR_INVALID, "diffusion_configure: dtime_step = %g must be finite", dtime_step);
    const double k[2] = {diffusivity_sst, diffusivity_sss};
    for (int f = 0; f < 2; ++f) {
        h->diff_on[f] = k[f] > 0.;                                  // FE.cpp:2762
        h->diff_factor[f] = k[f] * dtime_step / std::pow(dx, 2.);   // FE.cpp:2775
    }
    h->diff_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_diffusion_configure"); }

// the element-to-element table and the packed OLD copy of this mesh, made once: bamgmesh->ElementConnectivity as nxs_mesh_element_connectivity computes it
// (Mesh.cpp:777-796), as 0-based ints with -1 on the boundary
static int diffusion_ensure(nxs_dyn_handle *h) {
    if (h->d_diff_ec) return NXS_OK;
    const int Ne = h->dm.Ne, Nn = h->dm.Nn;
    std::vector<int32_t> index(3 * (size_t)Ne);
    for (int e = 0; e < Ne; ++e) for (int k = 0; k < 3; ++k) index[3 * (size_t)e + k] = h->h_t[k][e] + 1;
    std::vector<double> ec(3 * (size_t)Ne);
    if (int rc = nxs_mesh_element_connectivity(index.data(), Nn, Ne, ec.data())) return fail(h, rc, "diffuse: the mesh has an edge shared by three triangles");
    std::vector<int> tab(3 * (size_t)Ne);
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = std::isnan(ec[i]) ? -1 : (int)ec[i] - 1;
    const int *d_ec = nullptr;
    if (int rc = dev_upload(h, h->diff_allocs, &d_ec, tab)) return rc;
    if (int rc = dev_alloc(h, h->diff_allocs, &h->d_diff_old, 2 * (size_t)Ne)) return rc;
    h->d_diff_ec = const_cast<int *>(d_ec);
    return NXS_OK;
}

int nxs_dyn_diffuse(nxs_dyn_handle *h) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->diff_configured) return fail(h, NXS_ERR_STATE, "diffuse before nxs_dyn_diffusion_configure");
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "diffuse before set_mesh");
    if (multi_rank(h) || h->have_halo)
        return fail(h, NXS_ERR_STATE, "diffuse: this handle has halo lists set (rank %d of %d): the reference diffuses on its root rank from gathered fields, and the gather / scatter "
                                      "of a partitioned run is not done here", h->rank, h->nranks);
    if (ocean_coupled_on(h)) return fail(h, NXS_ERR_STATE, "diffuse: a coupled ocean is attached (nxs_dyn_ocean_coupled_attach): the reference does not diffuse M_sst / M_sss when coupled to an ocean (FE.cpp:3934-3940)");
    if (!h->diff_on[0] && !h->diff_on[1]) return NXS_OK;   // "nothing to do" (FE.cpp:2762-2767)
    double *sst = h->d_flux_st[2], *sss = h->d_flux_st[3];
    if (!(h->flux_st_have & (1u << 2))) return fail(h, NXS_ERR_STATE, "diffuse: sst was never put on this mesh (nxs_dyn_flux_put after set_mesh / regrid)");
    if (!(h->flux_st_have & (1u << 3))) return fail(h, NXS_ERR_STATE, "diffuse: sss was never put on this mesh (nxs_dyn_flux_put after set_mesh / regrid)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = diffusion_ensure(h)) return rc;
    const int Ne = h->dm.Ne;
    NestPair *old = reinterpret_cast<NestPair *>(h->d_diff_old);
    LAUNCH(h, k_diffuse_pack, Ne, Ne, (const double *)sst, (const double *)sss, old);
    LAUNCH(h, k_diffuse, Ne, Ne, reinterpret_cast<const DiffTri *>(h->d_diff_ec), (const NestPair *)old, h->diff_factor[0], h->diff_factor[1], h->diff_on[0] ? 1 : 0,
           h->diff_on[1] ? 1 : 0, sst, sss);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_diffuse"); }

int nxs_dyn_flux_device_rows(nxs_dyn_handle *h, const double **device_rows) try {
    if (!h || !device_rows) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "flux_device_rows before set_mesh");
    for (int k = 0; k < FLUX_ST_ROWS; ++k) device_rows[k] = (h->flux_st_have >> k) & 1u ? h->d_flux_st[k] : nullptr;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_flux_device_rows"); }
