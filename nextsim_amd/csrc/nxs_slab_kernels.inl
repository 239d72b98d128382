// nxs_slab_kernels.inl -- the rest of thermo()'s slab loop on the device: FE.cpp:5413-6133 as a default (non-OASIS) build compiles it (textually included by
// nxs_dyn.hip behind nxs_column_kernels.inl; include/nxs_dyn.h, nxs_slab_* / nxs_dyn_slab_* / nxs_dyn_slab).  FE.cpp = model/finiteelement.cpp.
//   k_slab   the assimilation flux (FE.cpp:5415-5425), section 6: new ice and lateral melt (5434-5646, newice_type 1 .. 4 with windSpeedElement, 6359-6370, and
//            melt_type 1, 2), the freeze-days block (5649-5682), the new concentration and thickness with Winton's (38), (39), (26) (5685-5711), the limit block
//            (5714-5728), section 7 (5800-5801), section 8: the slab ocean with meltPonds (5812-5846, 6538-6627), section 9: the temperature-dependent healing
//            (5854-5881), section 10: the diagnostics (5903-5976) and the age and type tracers (5980-6132)
// One thread = one element, ghost elements included, one launch per call.  Every row is [Ne] and a thread touches entry e of it: whole lines per wave; only
// newice_type 3 gathers M_wind at the three nodes.  No LDS, no atomics.  Operand order is the reference's, divisions stay divisions, the build is uncontracted
// (-ffp-contract=off).  The library calls beyond sqrt and round are pow (the assimilation flux) and hypot (newice_type 3).  The configuration switches are uniform
// branches of one body.  Everything of an element is worked on as locals and stored once, as soon as it is final (conditional stores through references cost scratch: see
// nxs_column_kernels.inl; early stores and late loads keep the live registers down).  Qow is the reference's function-local vector: the kernel works on a register copy and the flux rows stay READ-ONLY, like the column rows.
// Where the reference makes a NaN (0 / 0 in f1 of FE.cpp:5706 when there is neither old nor new ice) the kernel makes the same one.
// The body is slab_element<COUPLED>, ONE source of the loop's arithmetic: k_slab is its COUPLED = false instance (a default build's loop), k_coupled_thermo
// (nxs_slab_fsd_kernels.inl, nxs_dyn_slab_coupled) its COUPLED = true instance, which adds what an OASIS build compiles into these lines: melt_type 3
// (FE.cpp:5592-5640), reading the bins as a stream, and the four intermediates the bins' own launch needs (old_conc, old_conc_young, lat_melt_rate,
// young_ice_growth) as rows.  Everything COUPLED adds stands behind `if constexpr`, so k_slab is the kernel it was.
// NOT here: the FSD branches of the limit block (5729-5764), redistributeThermoFSD (5768-5776), the in-loop weldingRoach (5779-5797) and the mechanical FSD healing
// of 9.b (5883-5898) are k_coupled_bins (nxs_slab_fsd_kernels.inl).  In NO kernel, because they need the coupled ocean's received fields: the OceanType::COUPLED
// guards (5826-5841), their counterpart in the column (5348-5358), M_qsrml (5150-5156).  The throw of a wrong newice_type / melt_type is NXS_ERR_INVALID at
// configuration.

// physical::, model/constants.hpp (cpw, ki and hmin are nxs_column_kernels.inl's)
#define NXS_CMIN 1e-12

#include "nxs_wind_speed.inl"   // wind_speed_element: shared with k_fluxes and the Moorings means

enum { SLAB_QA = 0, SLAB_QSW, SLAB_QLW, SLAB_QSH, SLAB_QLH, SLAB_QO, SLAB_QNOSUN, SLAB_QSW_OCEAN, SLAB_QASSIM, SLAB_DELS, SLAB_FWFLUX_ICE, SLAB_FWFLUX, SLAB_BRINE,
       SLAB_EVAP, SLAB_RAIN, SLAB_VICE_MELT, SLAB_DEL_VI_YOUNG, SLAB_DEL_HI, SLAB_DEL_HI_YOUNG, SLAB_NEWICE, SLAB_MLT_TOP, SLAB_MLT_BOT, SLAB_SNOW2ICE, SLAB_ALBEDO,
       SLAB_SIALB, SLAB_DEL_CI_MLT_MYI, SLAB_DEL_VI_MLT_MYI, SLAB_DEL_CI_RPLNT_MYI, SLAB_DEL_VI_RPLNT_MYI, SLAB_ROWS = 29 };
enum { SLAB_ST_ROWS = 10 /* nxs_dyn_slab_state without time_relaxation_damage */ };
static_assert(SLAB_ROWS == NXS_SLAB_ROWS && (int)SLAB_QASSIM == (int)NXS_SLAB_QASSIM && (int)SLAB_RAIN == (int)NXS_SLAB_RAIN && (int)SLAB_SIALB == (int)NXS_SLAB_SIALB &&
              (int)SLAB_DEL_VI_RPLNT_MYI == (int)NXS_SLAB_DEL_VI_RPLNT_MYI, "the rows of nxs_dyn_slab_get");

// the switches of the configuration and the clock: one word, uniform
enum { SF_ASSIM = 1 << 0, SF_HEALING = 1 << 1, SF_PONDS = 1 << 2, SF_RESET_BY_DATE = 1 << 3, SF_YOUNG_IN_MYI_RESET = 1 << 4 /* age.include_young_ice && age.reset_by_date:
       FE.cpp:5649-5650 */, SF_EQUAL_MELTING = 1 << 5, SF_YOUNG_CAT = 1 << 6, SF_WINTON = 1 << 7, SF_MLD_ROW = 1 << 8,
       SF_FIRST_STEP = 1 << 9, SF_LAST_STEP = 1 << 10, SF_FYI_RESET = 1 << 11, SF_MYI_RESET = 1 << 12, SF_ONSET_RESET = 1 << 13 /* nxs_dyn_slab_clock */,
       SF_OCEAN_COUPLED = 1 << 14 /* OceanType::COUPLED: a coupled ocean is attached (nxs_dyn_ocean_coupled_attach), M_sst and M_sss are not advanced */ };

struct SlabDev {
    int newice_type, melt_type;
    unsigned flags;                              // SF_*
    int freezingpoint_type;                      // the column's (section 9's Tbot)
    double rh0, rPhiF, PhiF, PhiM, h_young_min, h_young_max_sharp, assim_flux_exponent, freeze_days_threshold, meltponds_roff, meltponds_dep2frac;
    double time_relaxation_damage, deltaT_relaxation_damage;
    double mu, ks, constant_mld, ocean_albedo;   // the column's and the fluxes' configuration: one copy of each
    double dt;                                   // double(dt) of thermo(int dt): ddt; dtime_step is the same number (FE.cpp:1083-1084, 8140)
};

struct SlabArrays {
    int Ne, Nn;
    const int *t0, *t1, *t2;
    const double *wind;                                         // [2Nn] M_wind (newice_type 3)
    const double *flux;                                         // [FLUX_ROWS][Ne] the rows of nxs_dyn_fluxes, read-only
    const double *col;                                          // [COL_ROWS][Ne] the rows of nxs_dyn_column, read-only
    const double *precip, *mld;
    double *conc, *thick, *snow_thick, *ridge, *cyoung, *hyoung, *hsyoung, *cmyi, *tmyi, *theal;   // rows of nxs_dyn_state, in place
    double *sst, *sss, *pond_fraction, *lid_volume;             // rows of nxs_dyn_flux_state, in place
    double *tice0, *tice1, *tice2;
    double *st;                                                 // [SLAB_ST_ROWS][Ne] nxs_dyn_slab_state, one block: conc_upd is read, the other nine rows in place
    double *out;                                                // [SLAB_ROWS][Ne]
    unsigned *branches;                                         // [Ne] NXS_SLAB_BR_*
};
enum { SLAB_ST_CONC_UPD = 0, SLAB_ST_POND_VOLUME, SLAB_ST_DEL_VI_TEND, SLAB_ST_FREEZE_DAYS, SLAB_ST_FREEZE_ONSET, SLAB_ST_CONC_SUMMER, SLAB_ST_THICK_SUMMER,
       SLAB_ST_FYI_FRACTION, SLAB_ST_AGE_DET, SLAB_ST_AGE };

// what the COUPLED instance adds to the arrays of a launch (nxs_dyn_slab_coupled)
struct SlabCoupled {
    const double *fsd;                  // [nb][Ne] M_conc_fsd, read-only here
    const double *widths, *centres;     // [nb] M_fsd_bin_widths, M_fsd_bin_centres (device copies: the tables of nxs_dyn_fsd_configure)
    int nb;
    double *scr;                        // [SLAB_SCR_ROWS][Ne] what thermo() hands redistributeThermoFSD
    unsigned *br2;                      // [Ne] NXS_SLAB_FSD_BR_*
};
enum { SLAB_SCR_OLD_CONC = 0, SLAB_SCR_OLD_CONC_YOUNG, SLAB_SCR_LAT_MELT_RATE, SLAB_SCR_YOUNG_ICE_GROWTH, SLAB_SCR_ROWS };

template <bool COUPLED>
__device__ __forceinline__ void slab_element(const SlabArrays &a, const SlabDev &c, const SlabCoupled &x, const int e) {
    const size_t n = (size_t)a.Ne;
    const double ddt = c.dt;
    const double dtime_step = c.dt;
    const double qi = NXS_LF * NXS_RHOI;
    const double qs = NXS_LF * NXS_RHOS;
    const bool young = (c.flags & SF_YOUNG_CAT) != 0, winton = (c.flags & SF_WINTON) != 0, young_in_myi_reset = (c.flags & SF_YOUNG_IN_MYI_RESET) != 0;
    unsigned br = 0;
    [[maybe_unused]] unsigned br2 = 0;                  // NXS_SLAB_FSD_BR_* (COUPLED)
    [[maybe_unused]] double lat_melt_rate = 0.;         // FE.cpp:5471 (COUPLED)
    [[maybe_unused]] double young_ice_growth = 0.;      // FE.cpp:5473 (COUPLED)
    const double *const F = a.flux + e, *const K = a.col + e;
    double *const o = a.out + e, *const S = a.st + e;
    // FE.cpp:5306-5319 (the column left M_conc, M_thick, M_snow_thick and M_conc_young as they were)
    double conc = a.conc[e], thick = a.thick[e];
    double cy = 0., hy = 0., hsy = 0.;
    if (young) { cy = a.cyoung[e]; hy = a.hyoung[e]; hsy = a.hsyoung[e]; }
    const double old_vol = thick;
    const double old_conc = conc;
    const double old_conc_young = cy;
    const double old_conc_tot = old_conc + old_conc_young;
    const double old_ow_fraction = 1. - old_conc_tot;
    const double Qio = K[COL_QIO * n], Qio_young = K[COL_YOUNG * n];
    const double Qio_mean = Qio * old_conc + Qio_young * old_conc_young;   // FE.cpp:5821
    const double del_hi = K[COL_DEL_HI * n], del_hi_young = K[(COL_YOUNG + 4) * n];
    const double evap = F[FLUX_EVAP * n];
    {   // the diagnostics that need nothing of sections 6 to 9 (FE.cpp:5906-5924, 5942, 5954-5957, 5972-5976), stored while their operands are at hand
        const double Qlw_ow = F[FLUX_QLW_OW * n], Qsw_ow = F[FLUX_QSW_OW * n], Qlh_ow = F[FLUX_QLH_OW * n], Qsh_ow = F[FLUX_QSH_OW * n];
        const double Qlwi = F[FLUX_QLWI * n], Qswi = F[FLUX_QSWI * n], Qlhi = F[FLUX_QLHI * n], Qshi = F[FLUX_QSHI * n], albedo = F[FLUX_ALBEDO * n];
        double Qlw_young = 0., Qsw_young = 0., Qlh_young = 0., Qsh_young = 0., albedo_young = 0.;   // FE.cpp:5265-5273
        if (young) {
            Qlw_young = F[(FLUX_YOUNG + 1) * n]; Qsw_young = F[(FLUX_YOUNG + 2) * n]; Qlh_young = F[(FLUX_YOUNG + 3) * n]; Qsh_young = F[(FLUX_YOUNG + 4) * n];
            albedo_young = F[(FLUX_YOUNG + 8) * n];
        }
        o[SLAB_QSW * n] = Qswi * old_conc + Qsw_young * old_conc_young + Qsw_ow * old_ow_fraction;
        o[SLAB_QLW * n] = Qlwi * old_conc + Qlw_young * old_conc_young + Qlw_ow * old_ow_fraction;
        o[SLAB_QSH * n] = Qshi * old_conc + Qsh_young * old_conc_young + Qsh_ow * old_ow_fraction;
        o[SLAB_QLH * n] = Qlhi * old_conc + Qlh_young * old_conc_young + Qlh_ow * old_ow_fraction;
        o[SLAB_QNOSUN * n] = Qio_mean + old_ow_fraction * (Qlw_ow + Qlh_ow + Qsh_ow);
        o[SLAB_QSW_OCEAN * n] = old_ow_fraction * Qsw_ow;
        o[SLAB_EVAP * n] = evap * (1. - old_conc - old_conc_young);
        o[SLAB_DEL_HI * n] = del_hi * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_DEL_HI_YOUNG * n] = del_hi_young * NXS_DAYS_IN_SEC / ddt;
        double sialb = old_conc * albedo;
        if (young) sialb += old_conc_young * albedo_young;
        o[SLAB_ALBEDO * n] = sialb + STD_MAX(0., old_ow_fraction) * c.ocean_albedo;
        o[SLAB_SIALB * n] = (old_conc_tot > 0.) ? (sialb / old_conc_tot) : 0.;
    }
    // what sections 2 to 5 hand on
    double Qow = F[FLUX_QOW * n];
    const double Qia = F[FLUX_QIA * n];
    double Qia_young = 0.;   // FE.cpp:5266
    if (young) Qia_young = F[FLUX_YOUNG * n];
    const double tfrw = K[COL_TFRW * n];
    const double hi_old = K[COL_HI_OLD * n], del_hs_mlt = K[COL_DEL_HS_MLT * n], mlt_hi_top = K[COL_MLT_HI_TOP * n];
    double hi = K[COL_HI * n], hs = K[COL_HS * n];
    double mld = c.constant_mld;
    if (c.flags & SF_MLD_ROW) mld = a.mld[e];
    double sst = a.sst[e];
    double tice0 = a.tice0[e], tice1 = 0., tice2 = 0.;
    if (winton) { tice1 = a.tice1[e]; tice2 = a.tice2[e]; }

    // the compensation of the heat flux for a concentration reduced by assimilation, FE.cpp:5413-5425
    double Qassm = 0.;
    if (c.flags & SF_ASSIM) {
        const double conc_upd = S[SLAB_ST_CONC_UPD * n];
        const double conc_pre_assim = old_conc + old_conc_young - conc_upd;
        if (conc_pre_assim > 0 && conc_upd < 0) {
            br |= NXS_SLAB_BR_ASSIM;
            Qassm = (Qow * old_ow_fraction + Qio * old_conc + Qio_young * old_conc_young) * (pow(conc_upd / conc_pre_assim + 1, c.assim_flux_exponent) - 1);
        }
    }

    // 6) the ice growth over open water and the lateral melt, FE.cpp:5434-5646
    const double tw_new = sst - ddt * (Qow + Qassm) / (mld * NXS_RHOW * NXS_CPW);
    double newice = 0;
    if (tw_new < tfrw) {
        br |= NXS_SLAB_BR_SUPERCOOLED;
        newice = old_ow_fraction * (tfrw - tw_new) * mld * NXS_RHOW * NXS_CPW / qi;
        Qow = -(tfrw - sst) * mld * NXS_RHOW * NXS_CPW / ddt;
    }
    const double newice_stored = newice;
    double del_vi = newice + del_hi * old_conc;
    double del_vs_mlt = del_hs_mlt * old_conc;
    {   // FE.cpp:5448-5462, with the rows of FE.cpp:5951, 5963-5969 that nothing else reads
        double mlt_vi_top = mlt_hi_top * old_conc;
        double mlt_vi_bot = K[COL_MLT_HI_BOT * n] * old_conc;
        double snow2ice = K[COL_DEL_HI_S2I * n] * old_conc;
        double del_vi_young = 0.;
        if (young) {
            del_vi_young += del_hi_young * old_conc_young;
            del_vi += del_hi_young * old_conc_young;
            mlt_vi_top += K[(COL_YOUNG + 6) * n] * old_conc_young;
            mlt_vi_bot += K[(COL_YOUNG + 7) * n] * old_conc_young;
            snow2ice += K[(COL_YOUNG + 8) * n] * old_conc_young;
            del_vs_mlt += K[(COL_YOUNG + 5) * n] * old_conc_young;
        }
        o[SLAB_DEL_VI_YOUNG * n] = del_vi_young * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_MLT_TOP * n] = mlt_vi_top * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_MLT_BOT * n] = mlt_vi_bot * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_SNOW2ICE * n] = snow2ice * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_NEWICE * n] = newice_stored * NXS_DAYS_IN_SEC / ddt;
        o[SLAB_VICE_MELT * n] = del_vi * NXS_DAYS_IN_SEC / ddt;
    }
    double del_c = 0.;
    double newsnow = 0.;
    if (c.newice_type == 1) {
        del_c = newice * c.rh0;
    } else if (c.newice_type == 2) {
        if (hi_old > 0.) {
            br |= NXS_SLAB_BR_N2_HI_OLD;
            del_c = newice * c.PhiF / hi_old;
        } else if (newice > 0.) {
            br |= NXS_SLAB_BR_N2_NEWICE;
            del_c = 1.;
        } else
            del_c = 0.;
    } else if (c.newice_type == 3) {
        const double wspeed = wind_speed_element(a.wind, a.Nn, a.t0[e], a.t1[e], a.t2[e]);   // windSpeedElement, FE.cpp:6359-6370
        const double h0 = (1. + 0.1 * wspeed) / 15.;
        const double hp = c.rPhiF * hi_old;
        if (hp < h0) br |= NXS_SLAB_BR_N3_H0;
        del_c = newice / STD_MAX(hp, h0);
    } else {   // 4: the young-ice category
        hy += newice;
        const double room = 1. - conc, grown = cy + newice / c.h_young_min;
        cy = STD_MIN(room, grown);
        newice = 0.;
        newsnow = 0.;
        if (cy > 0.) {
            br |= NXS_SLAB_BR_N4_YOUNG;
            if (hy < c.h_young_min * cy) {
                br |= NXS_SLAB_BR_N4_NOT_FILLED;
                cy = hy / c.h_young_min;
                if constexpr (COUPLED) young_ice_growth = cy - old_conc_young;   // FE.cpp:5518
            } else {
                const double hiy = hy / cy;
                if (hiy > c.h_young_max_sharp) {
                    br |= NXS_SLAB_BR_N4_SHARP;
                    const double hsy0 = hsy / cy;
                    const double hsyc = STD_MAX(0., hsy0);
                    double tmp = cy * (c.h_young_max_sharp - c.h_young_min) / (hiy - c.h_young_min);
                    const double dc = cy - tmp;
                    del_c = STD_MAX(0., dc);
                    cy = tmp;
                    tmp = cy * c.h_young_max_sharp;
                    const double dv = hy - tmp;
                    newice = STD_MAX(0., dv);
                    hy = tmp;
                    tmp = cy * hsyc;
                    const double ds = hsy - tmp;
                    newsnow = STD_MAX(0., ds);
                    hsy = tmp;
                }
            }
        } else {
            br |= NXS_SLAB_BR_N4_NO_ROOM;
            thick += hy;
            newice = hy;
            newsnow = hsy;
            hy = 0.;
            hsy = 0.;
        }
    }
    {
        const double room = 1. - conc;
        del_c = STD_MIN(room, del_c);
    }
    if (del_hi < 0.) {
        br |= NXS_SLAB_BR_MELT;
        if (c.melt_type == 1) {
            if (conc < 1.) {
                br |= NXS_SLAB_BR_MELT_SIDE;
                del_c += del_hi * conc * c.PhiM / hi_old;
            } else
                del_c += 0.;
        } else if (!COUPLED || c.melt_type == 2) {
            if (hi > 0.) {
                br |= NXS_SLAB_BR_MELT_SIDE;
                del_c += c.PhiM * (1. - conc) * STD_MIN(0., Qow) * ddt / (hi * qi + hs * qs);
                Qow *= (1. - c.PhiM);
            } else
                del_c = -conc;
        } else if constexpr (COUPLED) {   // 3: Roach et al. (2018), FE.cpp:5592-5640 (M_num_fsd_bins >= 1: the configuration check)
            if (tw_new > tfrw) {
                br2 |= NXS_SLAB_FSD_BR_MELT3;
                const double m1 = 3.e-6;
                const double m2 = 1.36;
                double del_c_melt = 0.;
                double cat0_del_c = 0.;
                if (hi > 0) {
                    const double ctot = conc + cy;
                    if (ctot < 1e-11)
                        br2 |= NXS_SLAB_FSD_BR_CTOT_BREAK;   // the break of FE.cpp:5611
                    else {
                        double h0 = 0.;
                        if (cy > 0.) h0 = c.h_young_min + 2. * (hy - c.h_young_min * cy) / (cy);
                        if (fabs(x.fsd[(size_t)(x.nb - 1) * n + e] - ctot) < 1e-7) {   // unbroken: melt_type 2's rule on ctot
                            br2 |= NXS_SLAB_FSD_BR_UNBROKEN;
                            del_c_melt += c.PhiM * (1. - ctot) * STD_MIN(0., Qow) * ddt / (hi * qi + hs * qs);
                            const double all = -ctot;
                            del_c_melt = STD_MAX(del_c_melt, all);
                            Qow *= (1. - c.PhiM);
                        } else {
                            lat_melt_rate = -m1 * pow(tw_new - tfrw, m2);
                            lat_melt_rate = lat_melt_rate * 2.;
                            cat0_del_c = lat_melt_rate * x.fsd[e] / x.widths[0] * ddt;
                            del_c_melt += cat0_del_c;
                            for (int j = 0; j < x.nb - 1; ++j) del_c_melt += lat_melt_rate * (x.fsd[(size_t)j * n + e] * 2. / x.centres[j]) * ddt;
                            Qow -= del_c_melt * (hi * qi * conc + h0 * qi * cy) / (ddt * ctot);
                        }
                        del_c += (conc / ctot) * del_c_melt;
                        cy += del_c_melt * (cy / ctot);
                    }
                }
            }
        }
    }
    if constexpr (COUPLED) {   // what redistributeThermoFSD is called with (FE.cpp:5772), stored while at hand
        double *const X = x.scr + e;
        X[SLAB_SCR_OLD_CONC * n] = old_conc; X[SLAB_SCR_OLD_CONC_YOUNG * n] = old_conc_young; X[SLAB_SCR_LAT_MELT_RATE * n] = lat_melt_rate;
        X[SLAB_SCR_YOUNG_ICE_GROWTH * n] = young_ice_growth;
    }

    // the freeze days, FE.cpp:5649-5682
    double del_vi_tend = S[SLAB_ST_DEL_VI_TEND * n], freeze_days = S[SLAB_ST_FREEZE_DAYS * n], conc_summer_row = S[SLAB_ST_CONC_SUMMER * n],
           thick_summer_row = S[SLAB_ST_THICK_SUMMER * n];
    if (c.flags & SF_FIRST_STEP) del_vi_tend = 0.;
    del_vi_tend += del_vi * ddt;
    S[SLAB_ST_DEL_VI_TEND * n] = del_vi_tend;
    if (c.flags & SF_LAST_STEP) {
        if (del_vi_tend > 0.) {
            br |= NXS_SLAB_BR_DAY_FREEZE;
            freeze_days += 1.;
        } else if (del_vi_tend < 0.) {
            br |= NXS_SLAB_BR_DAY_MELT;
            freeze_days = 0.;
            double conc_summer = conc + STD_MIN(0., del_c);
            double thick_summer = thick + STD_MIN(0., del_vi);
            if (young && young_in_myi_reset) {
                conc_summer += cy;
                thick_summer += hy;
            }
            const double cs1 = STD_MIN(1., conc_summer);
            conc_summer_row = STD_MAX(0., cs1);
            thick_summer_row = STD_MAX(0., thick_summer);
        }
    }

    // the new concentration and thickness, FE.cpp:5685-5711
    conc += del_c;
    if (conc >= NXS_CMIN) {
        br |= NXS_SLAB_BR_CONC_GE_CMIN;
        hi = (hi * old_conc + newice) / conc;
        if (del_c < 0.) {
            br |= NXS_SLAB_BR_DEL_C_NEG;
            Qow -= del_c * hs * qs / ddt;
        } else
            hs = (hs * old_conc + newsnow) / conc;
        if (winton) {
            double f1 = thick / (thick + newice);
            double Tbar = f1 * (tice1 - NXS_LF * c.mu * NXS_SI / (NXS_HEAT_C * tice1)) + (1 - f1) * tfrw;   // (39)
            tice1 = (Tbar - sqrt(Tbar * Tbar + 4 * c.mu * NXS_SI * NXS_LF / NXS_HEAT_C)) / 2.;              // (38)
            tice2 = f1 * tice2 + (1 - f1) * tfrw;                                                           // (26)
        }
    }
    // the limits, FE.cpp:5714-5728
    double ridge = a.ridge[e];
    if (conc < NXS_CMIN || hi < NXS_HMIN) {
        br |= NXS_SLAB_BR_LIMIT;
        Qow += conc * hi * qi / ddt + conc * hs * qs / ddt;
        conc = 0.;
        tice0 = -c.mu * NXS_SI;
        if (winton) { tice1 = -c.mu * NXS_SI; tice2 = -c.mu * NXS_SI; }
        hi = 0.;
        hs = 0.;
        ridge = 0.;
    }

    // 7) the effective ice and snow thickness, FE.cpp:5800-5801
    thick = hi * conc;
    const double snow_thick = hs * conc;

    // 8) the slab ocean, FE.cpp:5812-5846
    const double precip = a.precip[e], tmp_snowfall = K[COL_SNOWFALL * n];
    const double rain0 = precip - tmp_snowfall;
    const double rain_on_ice = STD_MAX(0., rain0);
    double rain = (1. - old_conc - old_conc_young) * precip + (old_conc + old_conc_young) * rain_on_ice;
    double emp = evap * (1. - old_conc - old_conc_young) - rain;
    if (c.flags & SF_PONDS) {   // meltPonds(i, ddt, hi, hs, mlt_hi_top, del_hs_mlt, Qia[i], rain_on_ice, roff, dep2frac), FE.cpp:6538-6627
        double pond_volume = S[SLAB_ST_POND_VOLUME * n], lid_volume = a.lid_volume[e], pond_fraction;
        const double hIceMin = 0.1;
        const double concMin = 0.1;
        const double max_lid_thickness = 0.3;
        const double min_lid_thickness = 1e-3;
        const double ice_to_water = NXS_RHOI / NXS_RHOW;
        const double snow_to_water = NXS_RHOS / NXS_RHOW;
        const double water_to_ice = NXS_RHOW / NXS_RHOI;
        const double availableWater = -mlt_hi_top * ice_to_water - del_hs_mlt * snow_to_water + rain_on_ice / NXS_RHOW * ddt;
        pond_volume += (1 - c.meltponds_roff) * availableWater * conc;
        if (pond_volume <= 0. || conc <= concMin || thick / conc <= hIceMin) {
            br |= NXS_SLAB_BR_POND_FLUSHED;
            pond_volume = 0.;
            lid_volume = 0.;
            pond_fraction = 0.;
        } else {
            pond_fraction = sqrt(pond_volume / c.meltponds_dep2frac);
            const double nosnow = 1. - hs / (hs + 0.2);
            pond_fraction = STD_MIN(pond_fraction, nosnow);
            const double d0 = c.meltponds_dep2frac * pond_fraction, d1 = 0.9 * hi;
            double pond_depth = STD_MIN(d0, d1);
            pond_volume = pond_depth * pond_fraction;
            pond_depth = STD_MAX(0.05, pond_depth);
            const double fmax = (lid_volume + pond_volume) / pond_depth;
            pond_fraction = STD_MIN(pond_fraction, fmax);
            double delLidVolume = 0;
            if (lid_volume > 0. && pond_fraction > 1e-11) {
                br |= NXS_SLAB_BR_LID_EXISTS;
                const double TPond = -c.mu * NXS_SI;
                const double lt0 = lid_volume * water_to_ice / pond_fraction;
                const double lt1 = STD_MIN(max_lid_thickness, lt0);
                const double lidThickness = STD_MAX(min_lid_thickness, lt1);
                const double Qic = (TPond - tice0) / lidThickness * NXS_KI;
                const double qd = Qia - Qic;
                const double delLidThickness = (STD_MIN(qd, 0.) + Qic) * ddt / (NXS_RHOI * NXS_LF);
                delLidVolume = delLidThickness * ice_to_water * pond_fraction;
                const double nl = -lid_volume;
                delLidVolume = STD_MAX(delLidVolume, nl);
            } else if (Qia > 0.) {
                br |= NXS_SLAB_BR_LID_FORMS;
                delLidVolume = ddt * Qia / (NXS_RHOI * NXS_LF) * ice_to_water;
            }
            lid_volume += delLidVolume;
            pond_volume -= delLidVolume;
            if (pond_volume <= 0. || lid_volume * water_to_ice / pond_fraction >= max_lid_thickness) {
                br |= NXS_SLAB_BR_LID_REMOVED;
                lid_volume = 0.;
                pond_volume = 0.;
                pond_fraction = 0.;
            }
        }
        S[SLAB_ST_POND_VOLUME * n] = pond_volume; a.lid_volume[e] = lid_volume; a.pond_fraction[e] = pond_fraction;
    }
    const double Qdw = K[COL_QDW * n], Fdw = K[COL_FDW * n];
    double Qow_mean = Qow * old_ow_fraction;
    const bool ocean_coupled = (c.flags & SF_OCEAN_COUPLED) != 0;   // FE.cpp:5826-5828, 5838-5840
    if (!ocean_coupled) sst = sst - ddt * (Qio_mean + Qow_mean - Qdw + Qassm) / (NXS_RHOW * NXS_CPW * mld);
    double denominator = (mld * NXS_RHOW - del_vi * NXS_RHOI - (del_vs_mlt * NXS_RHOS + (emp - Fdw) * ddt));
    if (!(denominator > 1. * NXS_RHOW)) {
        br |= NXS_SLAB_BR_DENOM_CLAMP;
        denominator = 1. * NXS_RHOW;
    }
    double sss = a.sss[e];
    const double si_eff = STD_MIN(sss, NXS_SI);
    if (sss < NXS_SI) br |= NXS_SLAB_BR_SSS_BELOW_SI;
    const double delsss = ((sss - si_eff) * NXS_RHOI * del_vi + sss * (del_vs_mlt * NXS_RHOS + (emp - Fdw) * ddt)) / denominator;
    if (!ocean_coupled) {
        sss += delsss;
        a.sst[e] = sst; a.sss[e] = sss;
    }
    if (thick > old_vol) {
        br |= NXS_SLAB_BR_RIDGE;
        ridge *= old_vol / thick;
    }

    // 9) the temperature-dependent healing, FE.cpp:5854-5881
    if (c.flags & SF_HEALING) {
        double theal;
        if (thick > 0.) {
            br |= NXS_SLAB_BR_HEAL_ICE;
            ColDev cc{};
            cc.freezingpoint_type = c.freezingpoint_type; cc.mu = c.mu;
            const double Tbot = col_freezing_point(cc, sss);
            double C, deltaT;
            if (!winton) {
                C = NXS_KI * snow_thick / (c.ks * thick);
                const double d = Tbot - tice0;
                deltaT = STD_MAX(1e-36, d) / (1. + C);
            } else {
                C = NXS_KI * snow_thick / (c.ks * thick / 4.);
                const double d = Tbot + C * (Tbot - tice1) - tice0;
                deltaT = STD_MAX(1e-36, d) / (1. + C);
            }
            const double t = c.time_relaxation_damage * c.deltaT_relaxation_damage / deltaT;
            theal = STD_MAX(t, ddt);
        } else
            theal = 1e36;
        a.theal[e] = theal;
    }

    // 10) the diagnostics, FE.cpp:5903-5976
    o[SLAB_QA * n] = Qia * old_conc + Qia_young * old_conc_young + Qow * old_ow_fraction;
    o[SLAB_QO * n] = Qio_mean + Qow_mean;
    o[SLAB_QASSIM * n] = Qassm;
    o[SLAB_DELS * n] = delsss * NXS_RHOW * mld * NXS_DAYS_IN_SEC / dtime_step;
    const double fwflux_ice = -1. / ddt * ((1. - 1e-3 * si_eff) * NXS_RHOI * del_vi + NXS_RHOS * del_vs_mlt);
    o[SLAB_FWFLUX_ICE * n] = fwflux_ice;
    o[SLAB_FWFLUX * n] = fwflux_ice - emp;
    o[SLAB_BRINE * n] = -1e-3 * si_eff * NXS_RHOI * del_vi / ddt;
    o[SLAB_RAIN * n] = rain;
    a.snow_thick[e] = snow_thick; a.ridge[e] = ridge;
    a.tice0[e] = tice0;
    if (winton) { a.tice1[e] = tice1; a.tice2[e] = tice2; }

    // 10) the age and type tracers, FE.cpp:5980-6132
    double del_vi_rplnt_myi = 0.;
    double del_ci_rplnt_myi = 0.;
    double del_vi_mlt_myi = 0.;
    double del_ci_mlt_myi = 0.;
    double cmyi = a.cmyi[e], tmyi = a.tmyi[e];
    double freeze_onset = S[SLAB_ST_FREEZE_ONSET * n], fyi_fraction = S[SLAB_ST_FYI_FRACTION * n], age_det = S[SLAB_ST_AGE_DET * n], age = S[SLAB_ST_AGE * n];
    if (conc < NXS_CMIN || thick < conc * NXS_HMIN) {
        br |= NXS_SLAB_BR_NO_ICE_TRACERS;
        fyi_fraction = 0.;
        age_det = 0.;
        age = 0.;
        tmyi = 0.;
        cmyi = 0.;
        freeze_days = 0.;
        freeze_onset = 1.;
    } else {
        if (c.flags & SF_FYI_RESET)
            fyi_fraction = 0.;
        else {
            const double conc_fyi = fyi_fraction + del_c;
            const double f1 = STD_MIN(1., conc_fyi);
            fyi_fraction = STD_MAX(0., f1);
        }
        const double r_age = old_conc / conc;
        double w_age = old_conc <= 0 ? 0. : STD_MIN(r_age, 1.);
        const double y_det = (1 - w_age) * ddt;
        age_det = w_age * (age_det + ddt) + STD_MAX(y_det, 0.);
        const double r_vol = old_vol / thick;
        w_age = old_vol <= 0 ? 0. : STD_MIN(r_vol, 1.);
        const double y_age = (1 - w_age) * ddt;
        age = w_age * (age + ddt) + STD_MAX(y_age, 0.);
        bool reset_myi = false;
        if (c.flags & SF_RESET_BY_DATE) {
            if (c.flags & SF_MYI_RESET) reset_myi = true;
        } else if (freeze_days >= c.freeze_days_threshold) {
            br |= NXS_SLAB_BR_FREEZE_DAYS_GE;
            if (freeze_onset <= 0.5) {
                reset_myi = true;
                freeze_onset = 1.;
            }
        }
        if (c.flags & SF_ONSET_RESET) {
            freeze_onset = 0.;
            double ctot = conc;
            if (young) ctot += cy;
            if (ctot == 0.) freeze_onset = 1.;
            double conc_summer = conc;
            double thick_summer = thick;
            if (young && young_in_myi_reset) {
                conc_summer += cy;
                thick_summer += hy;
            }
            const double cs1 = STD_MIN(1., conc_summer);
            conc_summer_row = STD_MAX(0., cs1);
            thick_summer_row = STD_MAX(0., thick_summer);
        }
        freeze_onset = round(freeze_onset);
        const double old_conc_myi = cmyi;
        const double old_thick_myi = tmyi;
        double c_myi_max = conc;
        double v_myi_max = thick;
        if (young && young_in_myi_reset) {
            c_myi_max += cy;
            v_myi_max += hy;
        }
        if (reset_myi) {
            br |= NXS_SLAB_BR_RESET;
            if (!(c.flags & SF_RESET_BY_DATE)) {
                const double c_myi_reset = STD_MAX(conc_summer_row, cmyi);
                const double v_myi_reset = STD_MAX(thick_summer_row, tmyi);
                cmyi = STD_MIN(c_myi_max, c_myi_reset);
                tmyi = STD_MIN(v_myi_max, v_myi_reset);
            } else {
                cmyi = c_myi_max;
                tmyi = v_myi_max;
            }
            const double c1 = STD_MIN(1., cmyi);
            cmyi = STD_MAX(0., c1);
            tmyi = STD_MAX(0., tmyi);
            del_ci_rplnt_myi = cmyi - old_conc_myi;
            del_vi_rplnt_myi = tmyi - old_thick_myi;
        } else if (thick < old_vol && old_conc > 0 && old_vol > 0) {
            br |= NXS_SLAB_BR_OLD_MELT;
            if (c.flags & SF_EQUAL_MELTING) {
                const double rc = conc / old_conc, rv = thick / old_vol;
                const double del_c_ratio = STD_MIN(rc, 1.);
                const double del_v_ratio = STD_MIN(rv, 1.);
                const double dc = cmyi * (del_c_ratio - 1.), dv = tmyi * (del_v_ratio - 1.);
                del_ci_mlt_myi = STD_MIN(0., dc);
                del_vi_mlt_myi = STD_MIN(0., dv);
            }
            const double cn = cmyi + del_ci_mlt_myi, vn = tmyi + del_vi_mlt_myi;
            const double c1 = STD_MIN(c_myi_max, cn), v1 = STD_MIN(v_myi_max, vn);
            cmyi = STD_MAX(0., c1);
            tmyi = STD_MAX(0., v1);
            del_ci_mlt_myi = cmyi - old_conc_myi;
            del_vi_mlt_myi = tmyi - old_thick_myi;
        }
    }
    o[SLAB_DEL_CI_MLT_MYI * n] = del_ci_mlt_myi * NXS_DAYS_IN_SEC / ddt;
    o[SLAB_DEL_VI_MLT_MYI * n] = del_vi_mlt_myi * NXS_DAYS_IN_SEC / ddt;
    o[SLAB_DEL_CI_RPLNT_MYI * n] = del_ci_rplnt_myi * NXS_DAYS_IN_SEC / ddt;
    o[SLAB_DEL_VI_RPLNT_MYI * n] = del_vi_rplnt_myi * NXS_DAYS_IN_SEC / ddt;

    // the stores of everything updated in place
    a.conc[e] = conc; a.thick[e] = thick; a.cmyi[e] = cmyi; a.tmyi[e] = tmyi;
    if (young) { a.cyoung[e] = cy; a.hyoung[e] = hy; a.hsyoung[e] = hsy; }
    S[SLAB_ST_FREEZE_DAYS * n] = freeze_days; S[SLAB_ST_FREEZE_ONSET * n] = freeze_onset; S[SLAB_ST_CONC_SUMMER * n] = conc_summer_row;
    S[SLAB_ST_THICK_SUMMER * n] = thick_summer_row; S[SLAB_ST_FYI_FRACTION * n] = fyi_fraction; S[SLAB_ST_AGE_DET * n] = age_det; S[SLAB_ST_AGE * n] = age;
    a.branches[e] = br;
    if constexpr (COUPLED) x.br2[e] = br2;
}

__global__ void __launch_bounds__(BLOCK) k_slab(SlabArrays a, SlabDev c) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    slab_element<false>(a, c, SlabCoupled{}, e);
}
