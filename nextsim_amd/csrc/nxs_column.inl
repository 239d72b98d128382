// nxs_column.inl -- host side of nxs_col_* / nxs_dyn_column_* / nxs_dyn_column (include/nxs_dyn.h; the kernel is in nxs_column_kernels.inl).  Textually included by
// nxs_dyn.hip inside its extern "C" block, behind nxs_flux.inl.  FE.cpp = model/finiteelement.cpp.

int nxs_col_default_config(nxs_dyn_column_config *c) try {   // model/options.cpp:112, 291-293, 383-420
    if (!c) return NXS_ERR_INVALID;
    *c = nxs_dyn_column_config{};
    c->thermo_type = NXS_COL_THERMO_WINTON;               // options.cpp:112
    c->qio_type = NXS_COL_QIO_BASIC;                      // options.cpp:383
    c->freezingpoint_type = NXS_COL_FREEZINGPOINT_LINEAR; // options.cpp:384
    c->ocean_type = NXS_COL_OCEAN_CONSTANT;               // options.cpp:101
    c->snowfall_source = NXS_COL_SNOWFALL_PRECIP_SNOWFR;
    c->mld_source = NXS_COL_MLD_CONSTANT;
    c->flooding = 1;                                      // options.cpp:390
    c->freezingpoint_mu = 0.055;                          // options.cpp:386
    c->snow_cond = 0.3096;                                // options.cpp:404
    c->Csens_io = 1.e-3;                                  // options.cpp:411
    c->constant_mld = 9.;                                 // options.cpp:293
    c->nudge_timeT = NXS_DAYS_IN_SEC * 30;                // options.cpp:418, FE.cpp:5179
    c->nudge_timeS = NXS_DAYS_IN_SEC * 30;                // options.cpp:420, FE.cpp:5180
    c->Qdw_const = 0.;                                    // options.cpp:291
    c->Fdw_const = 0.;                                    // options.cpp:292
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_col_default_config"); }

int nxs_col_constants(double *out, int32_t count) try {   // model/constants.hpp, in the order of NXS_COL_CONST_*
    if (!out || count < 0) return NXS_ERR_INVALID;
    const double c[NXS_COL_CONST_COUNT] = {NXS_RHOW, NXS_CPW, NXS_RHOI, NXS_RHOS, NXS_LF, NXS_HEAT_C, NXS_KI, NXS_SI, NXS_HMIN};
    for (int i = 0; i < count && i < NXS_COL_CONST_COUNT; ++i) out[i] = c[i];
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_col_constants"); }

// what nxs_dyn_column_configure refuses; the text goes where nxs_dyn_last_error(h) finds it (h == NULL: the thread's create error)
static int col_config_check(nxs_dyn_handle *h, const nxs_dyn_column_config *c) {
    if (!c) return fail(h, NXS_ERR_INVALID, "column_configure: no configuration");
    if (c->thermo_type != NXS_COL_THERMO_ZERO_LAYER && c->thermo_type != NXS_COL_THERMO_WINTON)
        return fail(h, NXS_ERR_INVALID, "column_configure: unknown thermo_type %d", c->thermo_type);
    if (c->qio_type != NXS_COL_QIO_BASIC && c->qio_type != NXS_COL_QIO_EXCHANGE) return fail(h, NXS_ERR_INVALID, "column_configure: unknown qio_type %d", c->qio_type);
    if (c->freezingpoint_type != NXS_COL_FREEZINGPOINT_LINEAR && c->freezingpoint_type != NXS_COL_FREEZINGPOINT_UNESCO)
        return fail(h, NXS_ERR_INVALID, "column_configure: unknown freezingpoint_type %d", c->freezingpoint_type);
    if (c->ocean_type == NXS_COL_OCEAN_COUPLED)
        return fail(h, NXS_ERR_INVALID, "column_configure: ocean_type = COUPLED is the reference's #ifdef OASIS branch (FE.cpp:5348-5358), which is not built");
    if (c->ocean_type != NXS_COL_OCEAN_CONSTANT && c->ocean_type != NXS_COL_OCEAN_NUDGED) return fail(h, NXS_ERR_INVALID, "column_configure: unknown ocean_type %d", c->ocean_type);
    if (c->snowfall_source < NXS_COL_SNOWFALL_PRECIP_SNOWFR || c->snowfall_source > NXS_COL_SNOWFALL_PRECIP_TAIR)
        return fail(h, NXS_ERR_INVALID, "column_configure: unknown snowfall_source %d", c->snowfall_source);
    if (c->mld_source != NXS_COL_MLD_CONSTANT && c->mld_source != NXS_COL_MLD_ROW) return fail(h, NXS_ERR_INVALID, "column_configure: unknown mld_source %d", c->mld_source);
    if (!(c->snow_cond > 0.)) return fail(h, NXS_ERR_INVALID, "column_configure: snow_cond = %g must be positive", c->snow_cond);
    if (!(c->constant_mld > 0.)) return fail(h, NXS_ERR_INVALID, "column_configure: constant_mld = %g must be positive", c->constant_mld);
    if (!(c->nudge_timeT > 0.)) return fail(h, NXS_ERR_INVALID, "column_configure: nudge_timeT = %g must be positive", c->nudge_timeT);
    if (!(c->nudge_timeS > 0.)) return fail(h, NXS_ERR_INVALID, "column_configure: nudge_timeS = %g must be positive", c->nudge_timeS);
    return NXS_OK;
}

int nxs_col_config_check(const nxs_dyn_column_config *c) try {
    return col_config_check(nullptr, c);
} catch (...) { return dyn_caught(nullptr, "nxs_col_config_check"); }

int nxs_dyn_column_configure(nxs_dyn_handle *h, const nxs_dyn_column_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (int rc = col_config_check(h, c)) return rc;
    h->col_cfg = *c;
    h->col_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_column_configure"); }

int nxs_dyn_column_set_forcing(nxs_dyn_handle *h, const nxs_dyn_column_forcing *f) try {
    if (!h || !f) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "column_set_forcing before set_mesh");
    const double *src[COL_FORCING_ROWS] = {f->precip, f->snow, f->ocean_temp, f->ocean_salt, f->mld};
    return upload_rows(h, h->d_col_forcing, src, COL_FORCING_ROWS, &h->col_forcing_have);
} catch (...) { return dyn_caught(h, "nxs_dyn_column_set_forcing"); }

int nxs_dyn_column_put(nxs_dyn_handle *h, const nxs_dyn_column_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "column_put before set_mesh");
    const double *src[COL_ST_ROWS] = {s->tice1, s->tice2};
    return upload_rows(h, h->d_col_st, src, COL_ST_ROWS, &h->col_st_have);
} catch (...) { return dyn_caught(h, "nxs_dyn_column_put"); }

int nxs_dyn_column_get_state(nxs_dyn_handle *h, nxs_dyn_column_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "column_get_state before set_mesh");
    double *dst[COL_ST_ROWS] = {s->tice1, s->tice2};
    static const char *const name[COL_ST_ROWS] = {"tice1", "tice2"};
    for (int k = 0; k < COL_ST_ROWS; ++k)
        if (dst[k] && !(h->col_st_have & (1u << k))) return fail(h, NXS_ERR_STATE, "column_get_state: %s was never put on this mesh", name[k]);
    HIPCHK(h, hipSetDevice(h->device));
    return download_rows(h, dst, h->d_col_st, COL_ST_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_column_get_state"); }

int nxs_dyn_column(nxs_dyn_handle *h, int32_t dt) try {   // thermo()'s slab loop, sections 3.2 to 5, FE.cpp:5306-5411
    if (!h) return NXS_ERR_INVALID;
    if (dt <= 0) return fail(h, NXS_ERR_INVALID, "column: dt = %d must be positive", dt);
    if (!h->col_configured) return fail(h, NXS_ERR_STATE, "column before nxs_dyn_column_configure");
    if (!h->have_mesh || !h->have_state || !h->flux_done) return fail(h, NXS_ERR_STATE, "column before nxs_dyn_fluxes on this mesh (its rows, and tice0, tsurf_young, sst, sss, are the column's inputs)");
    const nxs_dyn_column_config &g = h->col_cfg;
    const bool coupled = ocean_coupled_on(h);   // the reference's OceanType::COUPLED, FE.cpp:5348-5358: the configuration's ocean_type is not consulted
    if (coupled && g.freezingpoint_type != NXS_COL_FREEZINGPOINT_UNESCO)
        return fail(h, NXS_ERR_STATE, "column: a coupled ocean is attached and freezingpoint_type is not UNESCO (FE.cpp:1246: the reference overrides the option when coupled to an ocean)");
    if (coupled)
        for (int k = 2; k <= 3; ++k)
            if (!(h->col_forcing_have & (1u << k)))
                return fail(h, NXS_ERR_STATE, "column: a coupled ocean is attached and %s is missing on this mesh (nxs_dyn_ocean_coupled_receive / _put_rows)", k == 2 ? "ocean_temp" : "ocean_salt");
    unsigned need = 0;   // bits of nxs_dyn_column_forcing: precip, snow, ocean_temp, ocean_salt, mld
    if (g.snowfall_source != NXS_COL_SNOWFALL_SNOWFALL) need |= 1u << 0;
    if (g.snowfall_source != NXS_COL_SNOWFALL_PRECIP_TAIR) need |= 1u << 1;
    if (g.ocean_type != NXS_COL_OCEAN_CONSTANT || coupled) need |= (1u << 2) | (1u << 3);
    if (g.mld_source == NXS_COL_MLD_ROW) need |= 1u << 4;
    if ((h->col_forcing_have & need) != need)
        return fail(h, NXS_ERR_STATE, "column: a forcing row is missing on this mesh (nxs_dyn_column_set_forcing after set_mesh / regrid; needed 0x%x, present 0x%x)", need, h->col_forcing_have);
    if (h->flux_atm_have != (1u << FLUX_ATM_ROWS) - 1 || h->flux_st_have != (1u << FLUX_ST_ROWS) - 1)
        return fail(h, NXS_ERR_STATE, "column: an atmosphere or flux row is missing on this mesh");
    if (g.thermo_type == NXS_COL_THERMO_WINTON && h->col_st_have != (1u << COL_ST_ROWS) - 1)
        return fail(h, NXS_ERR_STATE, "column: WINTON needs tice1 and tice2 on this mesh (nxs_dyn_column_put; mask of the rows present 0x%x)", h->col_st_have);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    const size_t Ne = h->dm.Ne;
    if (!h->d_col_out) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_col_out, (size_t)COL_ROWS * Ne)) return rc; }
    ColDev c{};
    c.thermo_type = g.thermo_type; c.qio_type = g.qio_type; c.freezingpoint_type = g.freezingpoint_type; c.ocean_type = coupled ? (int)NXS_COL_OCEAN_COUPLED : g.ocean_type;
    c.snowfall_source = g.snowfall_source; c.mld_source = g.mld_source; c.flooding = g.flooding != 0; c.young_cat = h->dp.young_cat ? 1 : 0;
    c.mu = g.freezingpoint_mu; c.ks = g.snow_cond; c.Csens_io = g.Csens_io; c.constant_mld = g.constant_mld; c.timeT = g.nudge_timeT; c.timeS = g.nudge_timeS;
    c.Qdw_const = g.Qdw_const; c.Fdw_const = g.Fdw_const; c.dt = double(dt);
    double *const *st = h->d_flux_st, *const *fo = h->d_col_forcing;
    // (a row the configuration does not need is never read: any valid row stands in for it)
    const double *any = h->d_flux_atm[0];
    const ColArrays a{h->dm.Ne, h->dm.Nn, h->dm.t0, h->dm.t1, h->dm.t2, h->ds.VT, h->ds.ocean, h->d_flux_atm[0], fo[0] ? fo[0] : any, fo[1] ? fo[1] : any, fo[2] ? fo[2] : any,
                       fo[3] ? fo[3] : any, fo[4] ? fo[4] : any, h->d_flux_out, h->ds.conc, h->ds.thick, h->ds.snow, h->ds.cyoung, h->ds.hyoung, h->ds.hsyoung,
                       st[0], h->d_col_st[0], h->d_col_st[1], st[1], st[2], st[3], h->d_col_out, coupled ? st[2] : nullptr, coupled ? st[3] : nullptr};
    LAUNCH(h, k_column, h->dm.Ne, a, c);
    HIPCHK(h, hipGetLastError());
    h->col_done = true;
    h->col_fresh = true;   // (what nxs_dyn_slab spends: nxs_slab.inl)
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_column"); }

int nxs_dyn_column_get(nxs_dyn_handle *h, const nxs_dyn_column_rows *out, const double **device_rows) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->col_done) return fail(h, NXS_ERR_STATE, "column_get before nxs_dyn_column on this mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const double *row[COL_ROWS];
    for (int k = 0; k < COL_ROWS; ++k) row[k] = h->d_col_out + (size_t)k * h->dm.Ne;
    if (device_rows) std::copy(row, row + COL_ROWS, device_rows);
    return download_rows(h, out ? out->row : nullptr, row, COL_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_column_get"); }
