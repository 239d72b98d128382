// nxs_slab.inl -- host side of nxs_slab_* / nxs_dyn_slab_* / nxs_dyn_slab (include/nxs_dyn.h; the kernel is in nxs_slab_kernels.inl).  Textually included by
// nxs_dyn.hip inside its extern "C" block, behind nxs_column.inl.  FE.cpp = model/finiteelement.cpp.

int nxs_slab_default_config(nxs_dyn_slab_config *c) try {   // model/options.cpp:329-331, 397-403, 428-449, 543-548
    if (!c) return NXS_ERR_INVALID;
    *c = nxs_dyn_slab_config{};
    c->newice_type = 4;                                   // options.cpp:397
    c->melt_type = 2;                                     // options.cpp:398
    c->use_assim_flux = 0;                                // options.cpp:428
    c->temp_dep_healing = 0;                              // options.cpp:329
    c->use_meltponds = 0;                                 // options.cpp:445
    c->reset_by_date = 0;                                 // options.cpp:544
    c->include_young_ice = 1;                             // options.cpp:545
    c->equal_melting = 1;                                 // options.cpp:548
    c->hnull = 0.25;                                      // options.cpp:399
    c->PhiF = 4.;                                         // options.cpp:400
    c->PhiM = 0.5;                                        // options.cpp:401
    c->h_young_min = 0.05;                                // options.cpp:403
    c->h_young_max = 0.5;                                 // options.cpp:402
    c->assim_flux_exponent = 1.0;                         // options.cpp:430
    c->reset_freeze_days = 3.;                            // options.cpp:546
    c->meltpond_runoff_fraction = 0.2;                    // options.cpp:447
    c->meltpond_depth_to_fraction = 0.8;                  // options.cpp:449
    c->time_relaxation_damage = NXS_DAYS_IN_SEC * 25.;    // options.cpp:330 [days]
    c->deltaT_relaxation_damage = 20.;                    // options.cpp:331
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_slab_default_config"); }

int nxs_slab_constants(double *out, int32_t count) try {   // model/constants.hpp, in the order of NXS_SLAB_CONST_*
    if (!out || count < 0) return NXS_ERR_INVALID;
    const double c[NXS_SLAB_CONST_COUNT] = {NXS_CMIN, NXS_HMIN, NXS_RHOW, NXS_CPW, NXS_RHOI, NXS_RHOS, NXS_LF, NXS_HEAT_C, NXS_KI, NXS_SI, NXS_DAYS_IN_SEC};
    for (int i = 0; i < count && i < NXS_SLAB_CONST_COUNT; ++i) out[i] = c[i];
    return NXS_OK;
} catch (...) { return dyn_caught(nullptr, "nxs_slab_constants"); }

// what nxs_dyn_slab_configure refuses; the text goes where nxs_dyn_last_error(h) finds it (h == NULL: the thread's create error)
static int slab_config_check(nxs_dyn_handle *h, const nxs_dyn_slab_config *c) {
    if (!c) return fail(h, NXS_ERR_INVALID, "slab_configure: no configuration");
    if (c->newice_type < 1 || c->newice_type > 4) return fail(h, NXS_ERR_INVALID, "slab_configure: newice_type = %d (1 .. 4, FE.cpp:5477-5554)", c->newice_type);
    if (c->melt_type == 3)
        return fail(h, NXS_ERR_INVALID, "slab_configure: melt_type = 3 is the reference's #ifdef OASIS branch (FE.cpp:5591-5641, the FSD-dependent lateral melt), which is not built");
    if (c->melt_type < 1 || c->melt_type > 2) return fail(h, NXS_ERR_INVALID, "slab_configure: melt_type = %d (1 .. 2, FE.cpp:5562-5645)", c->melt_type);
    if (!(c->hnull > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: hnull = %g must be positive", c->hnull);
    if (!(c->PhiF > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: PhiF = %g must be positive", c->PhiF);
    if (!(c->h_young_min > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: h_young_min = %g must be positive", c->h_young_min);
    if (!(c->h_young_max > c->h_young_min)) return fail(h, NXS_ERR_INVALID, "slab_configure: h_young_max = %g must be larger than h_young_min = %g", c->h_young_max, c->h_young_min);
    if (!(c->meltpond_depth_to_fraction > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: meltpond_depth_to_fraction = %g must be positive", c->meltpond_depth_to_fraction);
    if (!(c->time_relaxation_damage > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: time_relaxation_damage = %g must be positive", c->time_relaxation_damage);
    if (!(c->deltaT_relaxation_damage > 0.)) return fail(h, NXS_ERR_INVALID, "slab_configure: deltaT_relaxation_damage = %g must be positive", c->deltaT_relaxation_damage);
    return NXS_OK;
}

int nxs_slab_config_check(const nxs_dyn_slab_config *c) try {
    return slab_config_check(nullptr, c);
} catch (...) { return dyn_caught(nullptr, "nxs_slab_config_check"); }

int nxs_dyn_slab_configure(nxs_dyn_handle *h, const nxs_dyn_slab_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (int rc = slab_config_check(h, c)) return rc;
    h->slab_cfg = *c;
    h->slab_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_configure"); }

static const char *const slab_st_name[SLAB_ST_ROWS] = {"conc_upd", "pond_volume", "del_vi_tend", "freeze_days", "freeze_onset", "conc_summer", "thick_summer", "fyi_fraction",
                                                        "age_det", "age"};

int nxs_dyn_slab_put(nxs_dyn_handle *h, const nxs_dyn_slab_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "slab_put before set_mesh");
    const double *src[SLAB_ST_ROWS] = {s->conc_upd, s->pond_volume, s->del_vi_tend, s->freeze_days, s->freeze_onset, s->conc_summer, s->thick_summer, s->fyi_fraction, s->age_det, s->age};
    if (!h->d_slab_st[0]) {   // one block for the ten rows: the kernel takes its base (a pointer per row would not fit the scalar registers)
        HIPCHK(h, hipSetDevice(h->device));
        double *base = nullptr;
        if (int rc = dev_alloc(h, h->state_allocs, &base, (size_t)SLAB_ST_ROWS * h->dm.Ne)) return rc;
        for (int k = 0; k < SLAB_ST_ROWS; ++k) h->d_slab_st[k] = base + (size_t)k * h->dm.Ne;
    }
    return upload_rows(h, h->d_slab_st, src, SLAB_ST_ROWS, &h->slab_st_have);
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_put"); }

int nxs_dyn_slab_get_state(nxs_dyn_handle *h, nxs_dyn_slab_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "slab_get_state before set_mesh");
    double *dst[SLAB_ST_ROWS + 1] = {s->conc_upd, s->pond_volume, s->del_vi_tend, s->freeze_days, s->freeze_onset, s->conc_summer, s->thick_summer, s->fyi_fraction, s->age_det, s->age,
                                     s->time_relaxation_damage};
    for (int k = 0; k < SLAB_ST_ROWS; ++k)
        if (dst[k] && !(h->slab_st_have & (1u << k))) return fail(h, NXS_ERR_STATE, "slab_get_state: %s was never put on this mesh", slab_st_name[k]);
    if (s->time_relaxation_damage && !h->have_state) return fail(h, NXS_ERR_STATE, "slab_get_state: time_relaxation_damage before put_state");
    HIPCHK(h, hipSetDevice(h->device));
    const double *dev[SLAB_ST_ROWS + 1];
    for (int k = 0; k < SLAB_ST_ROWS; ++k) dev[k] = h->d_slab_st[k];
    dev[SLAB_ST_ROWS] = h->ds.theal;
    return download_rows(h, dst, dev, SLAB_ST_ROWS + 1);
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_get_state"); }

static int slab_coupled_ready(nxs_dyn_handle *h);   // nxs_slab_fsd.inl

// what nxs_dyn_slab and nxs_dyn_slab_coupled (nxs_slab_fsd.inl) share: the refusals -- about the bins each has its own, at the same place --, the output rows, and
// the arguments of slab_element
static int slab_launch_args(nxs_dyn_handle *h, bool coupled, int32_t dt, const nxs_dyn_slab_clock *clock, SlabArrays *pa, SlabDev *pc) {
    const char *const what = coupled ? "slab_coupled" : "slab";
    if (dt <= 0) return fail(h, NXS_ERR_INVALID, "%s: dt = %d must be positive", what, dt);
    if (!clock) return fail(h, NXS_ERR_INVALID, "%s: no clock (nxs_dyn_slab_clock: the five flags the reference derives from M_current_time)", what);
    if (!h->slab_configured) return fail(h, NXS_ERR_STATE, "%s before nxs_dyn_slab_configure", what);
    if (!h->have_mesh || !h->have_state || !h->flux_done || !h->col_done)
        return fail(h, NXS_ERR_STATE, "%s before nxs_dyn_column on this mesh (its rows and those of nxs_dyn_fluxes are the slab's inputs)", what);
    if (!h->col_fresh)
        return fail(h, NXS_ERR_STATE, "%s: a second nxs_dyn_slab without a new nxs_dyn_column in between (the state has moved on: the column's rows are stale)", what);
    const nxs_dyn_slab_config &g = h->slab_cfg;
    const nxs_dyn_column_config &cg = h->col_cfg;
    if (!coupled && h->dw.conc_fsd)
        return fail(h, NXS_ERR_STATE, "slab: floe-size bins are attached (%d; nxs_dyn_put_coupled): the limit block's FSD branches, FE.cpp:5729-5764, are nxs_dyn_slab_coupled's", h->dw.nbins);
    if (coupled) { if (int rc = slab_coupled_ready(h)) return rc; }
    const bool young = h->dp.young_cat != 0;
    if ((g.newice_type == 4) != young)
        return fail(h, NXS_ERR_STATE, "%s: newice_type = %d on a handle of the %s category (newice_type 4 is the young-ice category's, and only its)", what, g.newice_type,
                    young ? "young-ice" : "classic");
    unsigned need = ((1u << SLAB_ST_ROWS) - 1) & ~3u;   // bits of nxs_dyn_slab_state: conc_upd, pond_volume, then the eight rows every launch needs
    if (g.use_assim_flux) need |= 1u << 0;
    if (g.use_meltponds) need |= 1u << 1;
    if ((h->slab_st_have & need) != need) {
        int k = 0;
        while (!((need & ~h->slab_st_have) & (1u << k))) ++k;
        return fail(h, NXS_ERR_STATE, "%s: %s is missing on this mesh (nxs_dyn_slab_put after set_mesh / regrid; needed 0x%x, present 0x%x)", what, slab_st_name[k], need, h->slab_st_have);
    }
    unsigned fneed = 1u << 0;   // bits of nxs_dyn_column_forcing: precip (the rain), mld
    if (cg.mld_source == NXS_COL_MLD_ROW) fneed |= 1u << 4;
    if ((h->col_forcing_have & fneed) != fneed)
        return fail(h, NXS_ERR_STATE, "%s: %s is missing on this mesh (nxs_dyn_column_set_forcing)", what, (h->col_forcing_have & 1u) ? "mld" : "precip");
    if (h->flux_st_have != (1u << FLUX_ST_ROWS) - 1) return fail(h, NXS_ERR_STATE, "%s: a flux row is missing on this mesh", what);
    const bool winton = cg.thermo_type == NXS_COL_THERMO_WINTON;
    if (winton && h->col_st_have != (1u << COL_ST_ROWS) - 1) return fail(h, NXS_ERR_STATE, "%s: WINTON needs tice1 and tice2 on this mesh", what);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    const size_t Ne = h->dm.Ne;
    if (!h->d_slab_out) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_slab_out, (size_t)SLAB_ROWS * Ne)) return rc; }
    if (!h->d_slab_br) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_slab_br, Ne)) return rc; }
    SlabDev c{};
    c.newice_type = g.newice_type; c.melt_type = coupled && h->slab_coupled_melt_type ? h->slab_coupled_melt_type : g.melt_type; c.freezingpoint_type = cg.freezingpoint_type;
    c.flags = (g.use_assim_flux ? SF_ASSIM : 0) | (g.temp_dep_healing ? SF_HEALING : 0) | (g.use_meltponds ? SF_PONDS : 0) | (g.reset_by_date ? SF_RESET_BY_DATE : 0) |
              (g.include_young_ice && g.reset_by_date ? SF_YOUNG_IN_MYI_RESET : 0) /* FE.cpp:5649-5650 */ | (g.equal_melting ? SF_EQUAL_MELTING : 0) |
              (young ? SF_YOUNG_CAT : 0) | (winton ? SF_WINTON : 0) | (cg.mld_source == NXS_COL_MLD_ROW ? SF_MLD_ROW : 0) |
              (clock->first_step_of_day ? SF_FIRST_STEP : 0) | (clock->last_step_of_day ? SF_LAST_STEP : 0) | (clock->fyi_reset_now ? SF_FYI_RESET : 0) |
              (clock->myi_reset_now ? SF_MYI_RESET : 0) | (clock->onset_reset_now ? SF_ONSET_RESET : 0) | (ocean_coupled_on(h) ? SF_OCEAN_COUPLED : 0);
    c.rh0 = 1. / g.hnull; c.rPhiF = 1. / g.PhiF;   // FE.cpp:5184-5185
    c.PhiF = g.PhiF; c.PhiM = g.PhiM; c.h_young_min = g.h_young_min;
    c.h_young_max_sharp = .5 * (g.h_young_min + g.h_young_max);   // FE.cpp:1198
    c.assim_flux_exponent = g.assim_flux_exponent; c.freeze_days_threshold = g.reset_freeze_days; c.meltponds_roff = g.meltpond_runoff_fraction;
    c.meltponds_dep2frac = g.meltpond_depth_to_fraction; c.time_relaxation_damage = g.time_relaxation_damage; c.deltaT_relaxation_damage = g.deltaT_relaxation_damage;
    c.mu = cg.freezingpoint_mu; c.ks = cg.snow_cond; c.constant_mld = cg.constant_mld; c.ocean_albedo = h->flux_cfg.ocean_albedo; c.dt = double(dt);
    double *const *st = h->d_flux_st, *const *fo = h->d_col_forcing;
    // (a row the configuration does not need is never touched: any valid row stands in for it)
    double *const any = h->d_slab_out;
    const SlabArrays a{h->dm.Ne, h->dm.Nn, h->dm.t0, h->dm.t1, h->dm.t2, h->ds.wind, h->d_flux_out, h->d_col_out, fo[0], fo[4] ? fo[4] : any,
                       h->ds.conc, h->ds.thick, h->ds.snow, h->ds.ridge, h->ds.cyoung, h->ds.hyoung, h->ds.hsyoung, h->ds.cmyi, h->ds.tmyi, h->ds.theal,
                       st[2], st[3], st[6], st[7], st[0], winton ? h->d_col_st[0] : any, winton ? h->d_col_st[1] : any, h->d_slab_st[0], h->d_slab_out, h->d_slab_br};
    *pa = a; *pc = c;
    return NXS_OK;
}

int nxs_dyn_slab(nxs_dyn_handle *h, int32_t dt, const nxs_dyn_slab_clock *clock) try {   // thermo()'s slab loop from FE.cpp:5413 to its end, 6133
    if (!h) return NXS_ERR_INVALID;
    SlabArrays a; SlabDev c;
    if (int rc = slab_launch_args(h, false, dt, clock, &a, &c)) return rc;
    LAUNCH(h, k_slab, h->dm.Ne, a, c);
    HIPCHK(h, hipGetLastError());
    h->col_fresh = false;   // the column's rows are spent: the next nxs_dyn_slab wants a new nxs_dyn_column
    h->slab_done = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_slab"); }

int nxs_dyn_slab_get(nxs_dyn_handle *h, const nxs_dyn_slab_rows *out, const double **device_rows) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->slab_done) return fail(h, NXS_ERR_STATE, "slab_get before nxs_dyn_slab on this mesh");
    HIPCHK(h, hipSetDevice(h->device));
    const double *row[SLAB_ROWS];
    for (int k = 0; k < SLAB_ROWS; ++k) row[k] = h->d_slab_out + (size_t)k * h->dm.Ne;
    if (device_rows) std::copy(row, row + SLAB_ROWS, device_rows);
    return download_rows(h, out ? out->row : nullptr, row, SLAB_ROWS);
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_get"); }
