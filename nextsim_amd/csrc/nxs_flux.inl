// nxs_flux.inl -- host side of nxs_dyn_flux_* / nxs_dyn_fluxes (include/nxs_dyn.h; the kernel is in nxs_flux_kernels.inl).  Textually included by nxs_dyn.hip inside
// its extern "C" block.  FE.cpp = model/finiteelement.cpp.

int nxs_flux_default_config(nxs_dyn_flux_config *c) try {   // model/options.cpp:388-438
    if (!c) return NXS_ERR_INVALID;
    *c = nxs_dyn_flux_config{};
    c->alb_scheme = 3;                       // options.cpp:389
    c->humidity_source = NXS_FLUX_HUM_DEWPOINT;
    c->longwave_source = NXS_FLUX_LW_QLW_IN; // options.cpp:424: thermo.use_parameterised_long_wave_radiation = false
    c->force_neutral_atmosphere = 0;         // options.cpp:436
    c->alb_ice = 0.538;                      // options.cpp:391
    c->alb_sn = 0.8256;                      // options.cpp:392
    c->alb_ponds = 0.30;                     // options.cpp:393
    c->I_0 = 0.30;                           // options.cpp:394
    c->ocean_albedo = 0.07;                  // options.cpp:388: thermo.albedoW
    c->drag_ocean_t = 0.83e-3;               // options.cpp:409
    c->drag_ocean_q = 1.5e-3;                // options.cpp:410
    c->zref_wind = 10.;                      // options.cpp:432
    c->zref_temp = 2.;                       // options.cpp:434
    c->limiting_lengthscale = 1.;            // options.cpp:438
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_flux_default_config"); }

int nxs_flux_constants(double *out, int32_t count) try {   // model/constants.hpp, in the order of NXS_FLUX_CONST_*
    if (!out || count < 0) return NXS_ERR_INVALID;
    const double c[NXS_FLUX_CONST_COUNT] = {NXS_TFRWK, NXS_RA_DRY, NXS_RA_VAP, NXS_CPA, NXS_CPV, NXS_LV0, NXS_EPS, NXS_SIGMA_SB, NXS_VONKARMAN, NXS_GAMMA_D, NXS_RHOA, NXS_LF, NXS_PHYS_G};
    for (int i = 0; i < count && i < NXS_FLUX_CONST_COUNT; ++i) out[i] = c[i];
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_flux_constants"); }

// what nxs_dyn_flux_configure refuses; the text goes where nxs_dyn_last_error(h) finds it (h == NULL: the thread's create error)
static int flux_config_check(nxs_dyn_handle *h, const nxs_dyn_flux_config *c) {
    if (!c) return fail(h, NXS_ERR_INVALID, "flux_configure: no configuration");
    if (c->alb_scheme < 1 || c->alb_scheme > 4) return fail(h, NXS_ERR_INVALID, "flux_configure: alb_scheme = %d (1 .. 4, FE.cpp:6461-6531)", c->alb_scheme);
    if (!(c->zref_wind > 0.)) return fail(h, NXS_ERR_INVALID, "flux_configure: zref_wind = %g must be positive", c->zref_wind);
    if (!(c->zref_temp > 0.)) return fail(h, NXS_ERR_INVALID, "flux_configure: zref_temp = %g must be positive", c->zref_temp);
    if (!(c->limiting_lengthscale > 0.)) return fail(h, NXS_ERR_INVALID, "flux_configure: limiting_lengthscale = %g must be positive", c->limiting_lengthscale);
    if (c->humidity_source < NXS_FLUX_HUM_DEWPOINT || c->humidity_source > NXS_FLUX_HUM_MIXRAT)
        return fail(h, NXS_ERR_INVALID, "flux_configure: unknown humidity_source %d", c->humidity_source);
    if (c->longwave_source != NXS_FLUX_LW_QLW_IN && c->longwave_source != NXS_FLUX_LW_TCC)
        return fail(h, NXS_ERR_INVALID, "flux_configure: unknown longwave_source %d", c->longwave_source);
    return NXS_OK;
}

int nxs_flux_config_check(const nxs_dyn_flux_config *c) try {
    return flux_config_check(nullptr, c);
} catch (...) { return dyn_caught(nullptr, "nxs_flux_config_check"); }

int nxs_dyn_flux_configure(nxs_dyn_handle *h, const nxs_dyn_flux_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (int rc = flux_config_check(h, c)) return rc;
    h->flux_cfg = *c;
    h->flux_configured = true;
    h->flux_dev_valid = false;   // (derived by the next nxs_dyn_fluxes, once)
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_flux_configure"); }

int nxs_dyn_flux_set_atmosphere(nxs_dyn_handle *h, const nxs_dyn_flux_atmosphere *a) try {
    if (!h || !a) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "flux_set_atmosphere before set_mesh");
    const double *src[FLUX_ATM_ROWS] = {a->tair, a->mslp, a->Qsw_in, a->humidity, a->longwave};
    return upload_rows(h, h->d_flux_atm, src, FLUX_ATM_ROWS, &h->flux_atm_have);
} catch (...) { return dyn_caught(h, "nxs_dyn_flux_set_atmosphere"); }

int nxs_dyn_flux_put(nxs_dyn_handle *h, const nxs_dyn_flux_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "flux_put before set_mesh");
    const double *src[FLUX_ST_ROWS] = {s->tice0, s->tsurf_young, s->sst, s->sss, s->drag_ti, s->drag_ti_young, s->pond_fraction, s->lid_volume};
    return upload_rows(h, h->d_flux_st, src, FLUX_ST_ROWS, &h->flux_st_have);
} catch (...) { return dyn_caught(h, "nxs_dyn_flux_put"); }

int nxs_dyn_flux_get(nxs_dyn_handle *h, nxs_dyn_flux_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "flux_get before set_mesh");
    double *dst[FLUX_ST_ROWS] = {s->tice0, s->tsurf_young, s->sst, s->sss, s->drag_ti, s->drag_ti_young, s->pond_fraction, s->lid_volume};
    static const char *const name[FLUX_ST_ROWS] = {"tice0", "tsurf_young", "sst", "sss", "drag_ti", "drag_ti_young", "pond_fraction", "lid_volume"};
    for (int k = 0; k < FLUX_ST_ROWS; ++k)
        if (dst[k] && !(h->flux_st_have & (1u << k))) return fail(h, NXS_ERR_STATE, "flux_get: %s was never put on this mesh", name[k]);
    HIPCHK(h, hipSetDevice(h->device));
    return download_rows(h, dst, h->d_flux_st, FLUX_ST_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_flux_get"); }

int nxs_dyn_fluxes(nxs_dyn_handle *h) try {   // thermo()'s "fluxes" timer, FE.cpp:5214-5277
    if (!h) return NXS_ERR_INVALID;
    if (!h->flux_configured) return fail(h, NXS_ERR_STATE, "fluxes before nxs_dyn_flux_configure");
    if (!h->have_mesh || !h->have_state || !h->have_forcing) return fail(h, NXS_ERR_STATE, "fluxes needs set_mesh, put_state and a forcing (the wind)");
    if (h->flux_atm_have != (1u << FLUX_ATM_ROWS) - 1)
        return fail(h, NXS_ERR_STATE, "fluxes: an atmosphere row is missing on this mesh (nxs_dyn_flux_set_atmosphere; mask of the rows present 0x%x)", h->flux_atm_have);
    if (h->flux_st_have != (1u << FLUX_ST_ROWS) - 1)
        return fail(h, NXS_ERR_STATE, "fluxes: a flux row is missing on this mesh (nxs_dyn_flux_put after set_mesh / regrid; mask of the rows present 0x%x)", h->flux_st_have);
    if (ocean_coupled_on(h) && !(h->oc_have & (1u << NXS_OC_QSRML)))
        return fail(h, NXS_ERR_STATE, "fluxes: a coupled ocean is attached and qsrml is missing on this mesh (nxs_dyn_ocean_coupled_receive / _put_rows; FE.cpp:5150-5157)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    const size_t Ne = h->dm.Ne;
    if (!h->d_flux_out) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_flux_out, (size_t)FLUX_ROWS * Ne)) return rc; }
    if (!h->d_tau_ow) h->d_tau_ow = h->d_flux_out + (size_t)FLUX_TAU_OW * Ne;   // (else: the row nxs_dyn_means_set_tau_ow made; both are the state pool's)
    if (!h->flux_dev_valid || h->flux_dev_qda != h->params.quad_drag_coef_air) {   // (z0 follows the handle's current quad_drag_coef_air: nxs_dyn_set_params)
        h->flux_dev = flux_derive(h->flux_cfg, h->params.quad_drag_coef_air);
        h->flux_dev_qda = h->params.quad_drag_coef_air;
        h->flux_dev_valid = true;
    }
    const FluxDev &c = h->flux_dev;
    double *const *at = h->d_flux_atm, *const *st = h->d_flux_st;
    const FluxArrays a{h->dm.Ne, h->dm.Nn, h->dp.young_cat, h->dm.t0, h->dm.t1, h->dm.t2, h->ds.wind, at[0], at[1], at[2], at[3], at[4],
                       h->ds.conc, h->ds.snow, h->ds.cyoung, h->ds.hsyoung, st[0], st[1], st[2], st[6], st[7],
                       h->ds.drag_ui, st[4], h->ds.drag_ui_young, st[5], h->d_flux_out, h->d_tau_ow, ocean_coupled_on(h) ? h->d_oc_qsrml : nullptr};
    LAUNCH(h, k_fluxes, h->dm.Ne, a, c);
    HIPCHK(h, hipGetLastError());
    h->tau_ow_attached = true;   // D_tau_ow is the handle's own now: taux / tauy / taumod of nxs_dyn_means_update need no upload
    h->flux_done = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fluxes"); }

int nxs_dyn_fluxes_get(nxs_dyn_handle *h, const nxs_dyn_flux_rows *out, const double **device_rows) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->flux_done) return fail(h, NXS_ERR_STATE, "fluxes_get before nxs_dyn_fluxes on this mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const double *row[FLUX_ROWS];
    for (int k = 0; k < FLUX_ROWS; ++k) row[k] = k == FLUX_TAU_OW ? h->d_tau_ow : h->d_flux_out + (size_t)k * h->dm.Ne;
    if (device_rows) std::copy(row, row + FLUX_ROWS, device_rows);
    return download_rows(h, out ? out->row : nullptr, row, FLUX_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_fluxes_get"); }
