// nxs_slab_fsd.inl -- host side of nxs_slab_coupled_config_check / nxs_dyn_slab_coupled* (include/nxs_dyn.h; the kernels are in nxs_slab_fsd_kernels.inl and
// nxs_slab_kernels.inl).  Textually included by nxs_dyn.hip inside its extern "C" block, behind nxs_slab.inl and nxs_fsd.inl.  FE.cpp = model/finiteelement.cpp.

static int slab_coupled_config_check(nxs_dyn_handle *h, const nxs_dyn_slab_config *c, int melt_type, int attached_bins) {
    if (!c) return fail(h, NXS_ERR_INVALID, "slab_coupled_configure: no configuration");
    if (melt_type < 1 || melt_type > 3) return fail(h, NXS_ERR_INVALID, "slab_coupled_configure: melt_type = %d (1 .. 3, FE.cpp:5562-5645)", melt_type);
    if (melt_type == 3 && attached_bins < 1)
        return fail(h, NXS_ERR_INVALID, "slab_coupled_configure: melt_type = 3 and attached_bins = %d < 1 are not compatible (FE.cpp:5594-5595; nxs_dyn_put_coupled)", attached_bins);
    nxs_dyn_slab_config own = *c;
    own.melt_type = melt_type == 3 ? 2 : melt_type;   // everything else is the slab's own check
    return slab_config_check(h, &own);
}

int nxs_slab_coupled_config_check(const nxs_dyn_slab_config *c, int32_t melt_type, int32_t attached_bins) try {
    return slab_coupled_config_check(nullptr, c, melt_type, attached_bins);
} catch (...) { return dyn_caught(nullptr, "nxs_slab_coupled_config_check"); }

int nxs_dyn_slab_coupled_configure(nxs_dyn_handle *h, int32_t melt_type) try {
    if (!h) return NXS_ERR_INVALID;
    if (!h->slab_configured) return fail(h, NXS_ERR_STATE, "slab_coupled_configure before nxs_dyn_slab_configure");
    if (int rc = slab_coupled_config_check(h, &h->slab_cfg, melt_type, 1)) return rc;   // (the bins melt_type 3 needs are asked for by nxs_dyn_slab_coupled: they go with the mesh, this survives it)
    h->slab_coupled_melt_type = melt_type;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_coupled_configure"); }

// what nxs_dyn_slab_coupled refuses about the bins (slab_launch_args calls it where nxs_dyn_slab refuses attached bins)
static int slab_coupled_ready(nxs_dyn_handle *h) {
    if (!h->dw.conc_fsd) return fail(h, NXS_ERR_STATE, "slab_coupled: no floe-size bins are attached (nxs_dyn_put_coupled with num_fsd_bins > 0); nxs_dyn_slab is the loop without them");
    if (!h->fsd_configured) return fail(h, NXS_ERR_STATE, "slab_coupled before nxs_dyn_fsd_configure (distinguish_mech_fsd, welding_type, welding_kappa, debug_fsd and the tables are its)");
    if (h->dw.nbins != h->fsd_cfg.n) return fail(h, NXS_ERR_STATE, "slab_coupled: configured for %d bins, %d attached (nxs_dyn_put_coupled, nxs_dyn_fsd_configure)", h->fsd_cfg.n, h->dw.nbins);
    if (h->fsd_cfg.distinguish && !h->fsd_mech)
        return fail(h, NXS_ERR_STATE, "slab_coupled: distinguish_mech_fsd without M_conc_mech_fsd: attach it with nxs_dyn_fsd_put");
    return NXS_OK;
}

int nxs_dyn_slab_coupled(nxs_dyn_handle *h, int32_t dt, const nxs_dyn_slab_clock *clock) try {   // thermo()'s slab loop of an OASIS build, FE.cpp:5413-6133
    if (!h) return NXS_ERR_INVALID;
    SlabArrays a; SlabDev c;
    if (int rc = slab_launch_args(h, true, dt, clock, &a, &c)) return rc;
    const size_t Ne = h->dm.Ne;
    if (!h->d_slab_scr) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_slab_scr, (size_t)SLAB_SCR_ROWS * Ne)) return rc; }
    if (!h->d_slab_br2) { if (int rc = dev_alloc(h, h->state_allocs, &h->d_slab_br2, Ne)) return rc; }
    if (!h->d_slab_crash) {   // the handle's own (not the mesh's): freed by nxs_dyn_destroy
        HIPCHK(h, hipMalloc((void **)&h->d_slab_crash, sizeof(int)));
        HIPCHK(h, hipMemsetAsync(h->d_slab_crash, 0, sizeof(int), h->stream));
    }
    const FsdDev *const fc = (const FsdDev *)h->d_fsd_cfg;
    const SlabCoupled x{h->dw.conc_fsd, fc->widths, fc->centres, h->dw.nbins, h->d_slab_scr, h->d_slab_br2};   // (addresses inside the device copy: nothing is read here)
    if (h->slab_coupled_timing) HIPCHK(h, hipEventRecord(h->slab_ev[0], h->stream));
    LAUNCH(h, k_coupled_thermo, h->dm.Ne, a, c, x);
    HIPCHK(h, hipGetLastError());
    if (h->slab_coupled_timing) HIPCHK(h, hipEventRecord(h->slab_ev[1], h->stream));
    const bool rec = h->sig_loc && h->dp.dynamics_type == NXS_DYN_BBM;   // as fsd_ready: M_damage is not touched here
    const FsdArrays fa{h->dm.Ne, h->dp.young_cat, h->dw.conc_fsd, h->fsd_mech, h->dw.cum_damage, h->fsd_cumw, h->ds.conc, h->ds.cyoung, h->ds.thick, h->ds.hyoung, h->ds.theal,
                       rec ? h->ds.S4a + 3 : h->ds.damage, rec ? 4 : 1, h->d_fsd_flags};
    const CoupledBins b{c.dt, c.melt_type, h->d_slab_scr, h->d_col_out + (size_t)COL_DEL_HI * Ne, h->d_slab_br, h->d_slab_br2, h->d_slab_crash};
    FSD_LAUNCH(h, k_coupled_bins, fa, fc, b);
    if (h->slab_coupled_timing) { HIPCHK(h, hipEventRecord(h->slab_ev[2], h->stream)); h->slab_coupled_timed = true; }
    h->col_fresh = false;   // the column's rows are spent, as by nxs_dyn_slab
    h->slab_done = true;
    h->slab_coupled_done = true;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_coupled"); }

int nxs_dyn_slab_coupled_info(nxs_dyn_handle *h, struct nxs_dyn_slab_coupled_info *info) try {
    if (!h || !info) return NXS_ERR_INVALID;
    int crash = 0;
    if (h->d_slab_crash) {   // the M_debug_fsd conditions of redistributeThermoFSD since the last call: reported once
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpyAsync(&crash, h->d_slab_crash, sizeof crash, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_slab_crash, 0, sizeof(int), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    info->thermo_fsd_crash = crash;
    return NXS_OK;
} catch (...) { return dyn_caught(h, "nxs_dyn_slab_coupled_info"); }
