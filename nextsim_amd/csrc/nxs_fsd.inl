// nxs_fsd.inl -- host side of nxs_dyn_fsd_* (include/nxs_dyn.h; the kernels are in nxs_fsd_kernels.inl).  Textually included by nxs_dyn.hip inside its
// extern "C" block.  FE.cpp = model/finiteelement.cpp.

// what nxs_dyn_fsd_configure refuses; the text goes where nxs_dyn_last_error(h) finds it (h == NULL: the thread's create error)
static int fsd_config_check(nxs_dyn_handle *h, const nxs_dyn_fsd_config *c, int attached_bins) {
    if (!c) return fail(h, NXS_ERR_INVALID, "fsd_configure: no configuration");
    const int n = c->num_bins;
    if (n < 1 || n > NXS_FSD_MAX_BINS) return fail(h, NXS_ERR_INVALID, "fsd_configure: num_bins = %d (1 .. NXS_FSD_MAX_BINS = %d)", n, NXS_FSD_MAX_BINS);
    if (n != attached_bins) return fail(h, NXS_ERR_INVALID, "fsd_configure: num_bins = %d, the attached conc_fsd has %d (nxs_dyn_put_coupled)", n, attached_bins);
    if (c->breakup_type < NXS_BREAKUP_NONE || c->breakup_type > NXS_BREAKUP_DUMONT) return fail(h, NXS_ERR_INVALID, "fsd_configure: unknown breakup_type %d", c->breakup_type);
    if (c->welding_type != NXS_WELDING_NONE && c->welding_type != NXS_WELDING_ROACH) return fail(h, NXS_ERR_INVALID, "fsd_configure: unknown welding_type %d", c->welding_type);
    if (c->fsd_damage_type < 0 || c->fsd_damage_type > 2) return fail(h, NXS_ERR_INVALID, "fsd_configure: unknown fsd_damage_type %d", c->fsd_damage_type);
    if (c->breakup_prob_type != 0) return fail(h, NXS_ERR_INVALID, "fsd_configure: unknown breakup_prob_type %d (only 0 exists, FE.cpp:4331-4341)", c->breakup_prob_type);
    const nxs_fsd_tables &t = c->tables;
    if (!t.bin_widths || !t.bin_low_limits || !t.bin_up_limits || !t.bin_centres || !t.area_scaled_up || !t.area_scaled_centered || !t.area_scaled_binwidth || !t.alpha_merge)
        return fail(h, NXS_ERR_INVALID, "fsd_configure: a table is NULL (nxs_fsd_bins makes them)");
    for (int kx = 0; kx < n; ++kx)
        for (int ky = 0; ky <= kx; ++ky) {
            const int a = t.alpha_merge[kx * n + ky];
            if (a < 1 || a > n)
                return fail(h, NXS_ERR_INVALID, "fsd_configure: alpha_merge[%d][%d] = %d is outside [1, %d]: weldingRoach would index tmp_conc_fsd[a - 1] out of bounds (FE.cpp:4780)", kx, ky, a, n);
        }
    return NXS_OK;
}

int nxs_fsd_config_check(const nxs_dyn_fsd_config *c, int32_t attached_bins) try {
    return fsd_config_check(nullptr, c, attached_bins);
} catch (...) { return dyn_caught(nullptr, "nxs_fsd_config_check"); }

int nxs_dyn_fsd_configure(nxs_dyn_handle *h, const nxs_dyn_fsd_config *c) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "fsd_configure before set_mesh");
    if (int rc = fsd_config_check(h, c, h->dw.conc_fsd ? h->dw.nbins : 0)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    FsdDev d{};
    const int n = c->num_bins;
    const nxs_fsd_tables &t = c->tables;
    d.n = n; d.breakup_type = c->breakup_type; d.damage_type = c->fsd_damage_type; d.welding_type = c->welding_type;
    d.distinguish = c->distinguish_mech_fsd != 0; d.debug = c->debug_fsd != 0; d.cell_avg = c->breakup_cell_average_thickness != 0;
    d.coef1 = c->breakup_coef1; d.coef2 = c->breakup_coef2; d.coef3 = c->breakup_coef3; d.prob_cutoff = c->breakup_prob_cutoff;
    {   // FE.cpp:4334-4335: tau_w = breakup_timescale_tuning; P[j] = P[j] * (1. - std::exp(-P[j] * cpl_time_step / tau_w)), P[j] = P_inf = 0 or 1
        const double tau_w = c->breakup_timescale_tuning;
        for (int k = 0; k < 2; ++k) { const double P = k; d.pfac[k] = P * (1. - std::exp(-P * c->cpl_time_step / tau_w)); }
    }
    const double poisson = 0.3;
    d.pi4_young = std::pow(NXS_PI, 4) * c->floes_flex_young;                           // FE.cpp:4312
    d.dflex_den = 48 * NXS_RHOW * NXS_FSD_G * (1 - std::pow(poisson, 2));                // FE.cpp:4313
    d.thick_min = c->breakup_thick_min; d.damage_max = c->fsd_damage_max; d.kappa = c->welding_kappa;
    const int ksi = 2;
    d.log_ksi = std::log(ksi);                                                           // FE.cpp:4398
    for (int k = 0; k < n; ++k) {
        d.centres[k] = t.bin_centres[k]; d.low[k] = t.bin_low_limits[k]; d.up[k] = t.bin_up_limits[k];
        d.asu[k] = t.area_scaled_up[k]; d.asc[k] = t.area_scaled_centered[k]; d.asb[k] = t.area_scaled_binwidth[k];
        d.widths[k] = t.bin_widths[k];
    }
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) {
            d.alpha[j][k] = t.alpha_merge[j * n + k];
            if (k > j) continue;
            if (c->breakup_type == NXS_BREAKUP_ZHANG) d.beta[j][k] = t.bin_widths[k] / (t.bin_up_limits[j] - t.bin_low_limits[0]);   // FE.cpp:4361
            else if (c->breakup_type == NXS_BREAKUP_UNIFORM_SIZE)                                                                   // FE.cpp:4380-4381
                d.beta[j][k] = (std::pow(t.bin_up_limits[k], 3) - std::pow(t.bin_low_limits[k], 3)) / (std::pow(t.bin_up_limits[j], 3) - std::pow(t.bin_low_limits[0], 3));
        }
    if (!h->d_fsd_cfg) {   // the handle's own (not the mesh's): freed by nxs_dyn_destroy
        HIPCHK(h, hipMalloc((void **)&h->d_fsd_cfg, sizeof(FsdDev)));
        HIPCHK(h, hipMalloc((void **)&h->d_fsd_flags, FSD_FLAGS * sizeof(int)));
        HIPCHK(h, hipMemsetAsync(h->d_fsd_flags, 0, FSD_FLAGS * sizeof(int), h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_fsd_cfg, &d, sizeof d, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (d is a local)
    h->fsd_cfg = d;
    h->fsd_configured = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_configure"); }

int nxs_dyn_fsd_put(nxs_dyn_handle *h, const nxs_dyn_fsd_state *s) try {   // M_conc_mech_fsd, M_cum_wave_damage
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "fsd_put before set_mesh");
    if (s->conc_mech_fsd && (!h->dw.conc_fsd || s->num_fsd_bins != h->dw.nbins))
        return fail(h, NXS_ERR_INVALID, "fsd_put: conc_mech_fsd with %d bins, the attached conc_fsd has %d (nxs_dyn_put_coupled first)", s->num_fsd_bins, h->dw.conc_fsd ? h->dw.nbins : 0);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne, nf = (size_t)h->dw.nbins * Ne;
    int rc;
    if (s->conc_mech_fsd) {
        if (nf > h->mech_capacity) {
            if ((rc = dev_alloc(h, h->coupled_allocs, &h->d_mech, nf))) return rc;
            h->mech_capacity = nf;
        }
        pin_host_buffer(h, s->conc_mech_fsd, nf * sizeof(double));
        HIPCHK(h, hipMemcpyAsync(h->d_mech, s->conc_mech_fsd, nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (s->cum_wave_damage) {
        if (!h->d_cumw && (rc = dev_alloc(h, h->coupled_allocs, &h->d_cumw, Ne))) return rc;
        pin_host_buffer(h, s->cum_wave_damage, Ne * sizeof(double));
        HIPCHK(h, hipMemcpyAsync(h->d_cumw, s->cum_wave_damage, Ne * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->fsd_mech = s->conc_mech_fsd ? h->d_mech : nullptr;
    h->fsd_cumw = s->cum_wave_damage ? h->d_cumw : nullptr;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_put"); }

int nxs_dyn_fsd_get(nxs_dyn_handle *h, nxs_dyn_fsd_state *s) try {
    if (!h || !s) return NXS_ERR_INVALID;
    if (!h->have_mesh) return fail(h, NXS_ERR_STATE, "fsd_get before set_mesh");
    if (s->conc_mech_fsd && !h->fsd_mech) return fail(h, NXS_ERR_INVALID, "fsd_get: conc_mech_fsd is not attached");
    if (s->cum_wave_damage && !h->fsd_cumw) return fail(h, NXS_ERR_INVALID, "fsd_get: cum_wave_damage is not attached");
    if (s->conc_mech_fsd && s->num_fsd_bins != h->dw.nbins) return fail(h, NXS_ERR_INVALID, "fsd_get: %d bins asked for, %d attached", s->num_fsd_bins, h->dw.nbins);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Ne = h->dm.Ne, nf = (size_t)h->dw.nbins * Ne;
    int crash = 0;
    if (h->d_fsd_flags) {   // the crash conditions of weldingRoach since the last get: reported once
        HIPCHK(h, hipMemcpyAsync(&crash, h->d_fsd_flags + FSD_FLAG_WELD_CRASH, sizeof crash, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_fsd_flags + FSD_FLAG_WELD_CRASH, 0, sizeof(int), h->stream));
    }
    const RowCopy cp[2] = {{s->conc_mech_fsd, h->fsd_mech, nf * sizeof(double), "conc_mech_fsd"}, {s->cum_wave_damage, h->fsd_cumw, Ne * sizeof(double), "cum_wave_damage"}};
    if (int rc = copy_rows(h, cp, 2, hipMemcpyDeviceToHost)) return rc;
    s->weld_crash = crash;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_get"); }

// the checks the four kernels share, and their arguments
static int fsd_ready(nxs_dyn_handle *h, const char *what, bool need_mech, FsdArrays *a) {
    if (!h) return NXS_ERR_INVALID;
    if (!h->have_mesh || !h->have_state) return fail(h, NXS_ERR_STATE, "%s needs set_mesh and put_state", what);
    if (!h->fsd_configured) return fail(h, NXS_ERR_STATE, "%s before nxs_dyn_fsd_configure", what);
    if (!h->dw.conc_fsd || h->dw.nbins != h->fsd_cfg.n)
        return fail(h, NXS_ERR_STATE, "%s: configured for %d bins, %d attached (nxs_dyn_put_coupled)", what, h->fsd_cfg.n, h->dw.conc_fsd ? h->dw.nbins : 0);
    if ((need_mech || h->fsd_cfg.distinguish) && !h->fsd_mech)
        return fail(h, NXS_ERR_STATE, "%s reads M_conc_mech_fsd (%s): attach it with nxs_dyn_fsd_put", what, h->fsd_cfg.distinguish ? "distinguish_mech_fsd" : "fsd_damage_type 1 / 2");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = launch_gave_up(h)) return rc;
    const bool rec = h->sig_loc && h->dp.dynamics_type == NXS_DYN_BBM;   // M_damage in the records the sub-step loop left behind (k_pack_state)
    *a = FsdArrays{h->dm.Ne, h->dp.young_cat, h->dw.conc_fsd, h->fsd_mech, h->dw.cum_damage, h->fsd_cumw, h->ds.conc, h->ds.cyoung, h->ds.thick, h->ds.hyoung, h->ds.theal,
                   rec ? h->ds.S4a + 3 : h->ds.damage, rec ? 4 : 1, h->d_fsd_flags};
    return NXS_OK;
}

#define FSD_LAUNCH(h, kern, ...)                                                      \
    do {                                                                              \
        const int n_ = (h)->fsd_cfg.n;                                                \
        if (n_ <= 2) LAUNCH(h, kern<2>, (h)->dm.Ne, __VA_ARGS__);                     \
        else if (n_ <= 6) LAUNCH(h, kern<6>, (h)->dm.Ne, __VA_ARGS__);                \
        else if (n_ <= 12) LAUNCH(h, kern<12>, (h)->dm.Ne, __VA_ARGS__);              \
        else LAUNCH(h, kern<16>, (h)->dm.Ne, __VA_ARGS__);                            \
        HIPCHK(h, hipGetLastError());                                                 \
    } while (0)

int nxs_dyn_fsd_init(nxs_dyn_handle *h) try {   // FE.cpp:7562-7576
    FsdArrays a;
    if (int rc = fsd_ready(h, "fsd_init", false, &a)) return rc;
    LAUNCH(h, k_fsd_init, h->dm.Ne, a, (const FsdDev *)h->d_fsd_cfg);
    HIPCHK(h, hipGetLastError());
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_init"); }

int nxs_dyn_fsd_update(nxs_dyn_handle *h) try {   // updateFSD(), FE.cpp:4674-4732
    FsdArrays a;
    if (int rc = fsd_ready(h, "fsd_update", false, &a)) return rc;
    FSD_LAUNCH(h, k_fsd_update, a, (const FsdDev *)h->d_fsd_cfg);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_update"); }

int nxs_dyn_fsd_breakup(nxs_dyn_handle *h, const double *wlbk, int32_t flags, int32_t *breakup_in_dt, int32_t *crash) try {   // redistributeFSD(), FE.cpp:4268-4483
    FsdArrays a;
    if (h && !wlbk) return fail(h, NXS_ERR_INVALID, "fsd_breakup: wlbk is NULL");
    if (h && (flags & ~NXS_FSD_WLBK_ON_DEVICE)) return fail(h, NXS_ERR_INVALID, "fsd_breakup: unknown flags %d", flags);
    if (int rc = fsd_ready(h, "fsd_breakup", h && h->fsd_cfg.damage_type != 0, &a)) return rc;
    const size_t Ne = h->dm.Ne;
    const double *d_wlbk = wlbk;
    if (!(flags & NXS_FSD_WLBK_ON_DEVICE)) {
        if (!h->d_wlbk) { if (int rc = dev_alloc(h, h->coupled_allocs, &h->d_wlbk, Ne)) return rc; }
        pin_host_buffer(h, wlbk, Ne * sizeof(double));
        HIPCHK(h, hipMemcpyAsync(h->d_wlbk, wlbk, Ne * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // (the upload of a host array is waited for, like every put; the kernel is not)
        d_wlbk = h->d_wlbk;
    }
    HIPCHK(h, hipMemsetAsync(h->d_fsd_flags, 0, 2 * sizeof(int), h->stream));   // M_breakup_in_dt = false (FE.cpp:4280), crash = false
    FSD_LAUNCH(h, k_fsd_breakup, a, (const FsdDev *)h->d_fsd_cfg, d_wlbk);
    if (breakup_in_dt || crash) {
        int f[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(f, h->d_fsd_flags, sizeof f, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (breakup_in_dt) *breakup_in_dt = f[FSD_FLAG_BREAKUP];
        if (crash) *crash = f[FSD_FLAG_CRASH];
    }
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_breakup"); }

int nxs_dyn_fsd_weld(nxs_dyn_handle *h, double ddt, const uint8_t *freezing) try {   // weldingRoach() + the mechanical healing, FE.cpp:4737-4870, 5888-5896
    FsdArrays a;
    if (h && !freezing) return fail(h, NXS_ERR_INVALID, "fsd_weld: freezing is NULL");
    if (int rc = fsd_ready(h, "fsd_weld", false, &a)) return rc;
    const size_t Ne = h->dm.Ne;
    if (!h->d_freezing) { if (int rc = dev_alloc(h, h->coupled_allocs, &h->d_freezing, Ne)) return rc; }
    HIPCHK(h, hipMemcpyAsync(h->d_freezing, freezing, Ne, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the upload is waited for, the kernel is not)
    FSD_LAUNCH(h, k_fsd_weld, a, (const FsdDev *)h->d_fsd_cfg, ddt, (const unsigned char *)h->d_freezing);
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_fsd_weld"); }
