// nxs_column_kernels.inl -- the ice columns of thermo()'s slab loop on the device: its sections 3.2 to 5, FE.cpp:5306-5411 (textually included by nxs_dyn.hip behind
// nxs_flux_kernels.inl; include/nxs_dyn.h, nxs_dyn_column_* / nxs_dyn_column).  FE.cpp = model/finiteelement.cpp.
//   k_column   the snowfall rule (FE.cpp:5321-5332), the nudging flux (5343-5366), iceOceanHeatflux (6396-6428), freezingPoint (6432-6448), thermoWinton (6633-6853)
//              or thermoIce0 (6860-6962) for the old ice and, in the young-ice category, thermoIce0 for the young ice with the stores of FE.cpp:5409-5410
// One thread = one element, ghost elements included, one launch per call; the old-ice and the young-ice column of an element run in the same thread.  Every row is
// [Ne] and a thread touches entry e of it; only the EXCHANGE scheme gathers M_VT and M_ocean at the three nodes.  No LDS, no atomics.  Operand order is the
// reference's, divisions stay divisions, the build is uncontracted (-ffp-contract=off).  The only library calls are sqrt (Winton's (21) and (38), the UNESCO
// freezing point) and hypot (EXCHANGE).  Where the reference makes a transient NaN (0 / 0 in (26) or (39) of a layer that has gone) the kernel makes the same one.
// NOT here: Winton's LOG(WARNING) when everything sublimates and its assert(Msurf >= 0); thermo() from FE.cpp:5413 on.  The OceanType::COUPLED branch (#ifdef OASIS,
// FE.cpp:5348-5358) runs while a coupled ocean is attached (nxs_dyn_ocean_coupled_attach): the host then passes NXS_COL_OCEAN_COUPLED, whatever was configured.

// physical::, model/constants.hpp (rhow, rhoi, rhos, Lf, C and si are nxs_dyn_kernels.inl's)
#define NXS_CPW 4186.84
#define NXS_KI 2.0334
#define NXS_HMIN 0.01

enum { COL_SNOWFALL = 0, COL_QDW, COL_FDW, COL_TFRW, COL_QIO, COL_HI, COL_HS, COL_HI_OLD, COL_DEL_HI, COL_DEL_HS_MLT, COL_MLT_HI_TOP, COL_MLT_HI_BOT, COL_DEL_HI_S2I,
       COL_YOUNG = 13 /* the nine rows from COL_QIO again */, COL_ROWS = 22 };
enum { COL_FORCING_ROWS = 5 /* nxs_dyn_column_forcing */, COL_ST_ROWS = 2 /* nxs_dyn_column_state */ };
static_assert(COL_ROWS == NXS_COL_ROWS && (int)COL_QIO == (int)NXS_COL_QIO && (int)COL_DEL_HI_S2I == (int)NXS_COL_DEL_HI_S2I && (int)COL_YOUNG == (int)NXS_COL_QIO_YOUNG, "the rows of nxs_dyn_column_get");

struct ColDev {
    int thermo_type, qio_type, freezingpoint_type, ocean_type, snowfall_source, mld_source, flooding, young_cat;
    double mu, ks, Csens_io, constant_mld, timeT, timeS, Qdw_const, Fdw_const;
    double dt;   // double(dt) of thermo(int dt): ddt, and what iceOceanHeatflux(..., const double dt) receives
};

struct ColArrays {
    int Ne, Nn;
    const int *t0, *t1, *t2;
    const double *VT, *ocean;                                   // [2Nn] M_VT, M_ocean (EXCHANGE)
    const double *tair, *precip, *snow, *ocean_temp, *ocean_salt, *mld;
    const double *flux;                                         // [FLUX_ROWS][Ne] the rows of nxs_dyn_fluxes
    const double *conc, *thick, *snow_thick, *cyoung;
    double *hyoung, *hsyoung;                                   // M_h_young, M_hs_young: rows of the dynamics state, written (FE.cpp:5409-5410)
    double *tice0, *tice1, *tice2, *tsurf_young;                // in place
    const double *sst, *sss;
    double *out;                                                // [COL_ROWS][Ne]
    double *sst_reset, *sss_reset;                              // the same two rows, writable: OceanType::COUPLED resets them (NULL otherwise)
};

// freezingPoint, FE.cpp:6432-6448
__device__ __forceinline__ double col_freezing_point(const ColDev &c, double sss) {
    if (c.freezingpoint_type == NXS_COL_FREEZINGPOINT_LINEAR) return -c.mu * sss;
    return (-0.0575 + 1.710523e-3 * sqrt(sss) - 2.154996e-4 * sss) * sss;
}

// thermoIce0, FE.cpp:6860-6962.  mlt_hi_bot and del_hi_s2i are the caller's accumulators (+=); Tsurf is read before it is written
__device__ __forceinline__ void col_ice0(const ColDev &c, double dt, double conc, double voli, double vols, double snowfall, double Qia, double dQiadT, double I, double subl,
                                         double Tbot, double &Qio_, double &hi_, double &hs_, double &hi_old_, double &del_hi_, double &del_hs_mlt_, double &mlt_hi_top_,
                                         double &mlt_hi_bot_, double &del_hi_s2i_, double &Tsurf_) {
    // (the in/out arguments are worked on as locals and stored once at the end: every one of them stays in registers)
    double Qio = Qio_, hi, hs, hi_old, del_hi, del_hs_mlt = del_hs_mlt_, mlt_hi_top = mlt_hi_top_, mlt_hi_bot = mlt_hi_bot_, del_hi_s2i = del_hi_s2i_, Tsurf = Tsurf_;
    const double qi = NXS_LF * NXS_RHOI;
    const double qs = NXS_LF * NXS_RHOS;
    const double Tfr_ice = -c.mu * NXS_SI;
    const double beta = 0.4;
    const double gamma = 1.065;
    if (conc <= 0. || voli <= 0.) {
        hi = 0.;
        hi_old = 0.;
        hs = 0.;
        Tsurf = Tfr_ice;
        del_hi = 0.;
    } else {
        hi = voli / conc;
        hi_old = hi;
        hs = vols / conc;
        double Qic, del_hb, del_ht, draft;
        const double Qia_mod = Qia + (1. - beta) * I;
        Qic = c.ks * (Tbot - Tsurf) / (hs + c.ks * hi / NXS_KI) * gamma;
        Tsurf = Tsurf + (Qic - Qia_mod) / (c.ks / (hs + c.ks * hi / NXS_KI) + dQiadT);
        if (hs > 0.) Tsurf = STD_MIN(0., Tsurf);
        else {
            const double tf = -c.mu * NXS_SI;
            Tsurf = STD_MIN(tf, Tsurf);
        }
        const double qm = Qia_mod - Qic;
        del_hs_mlt = STD_MIN(qm, 0.) * dt / qs;
        hs += del_hs_mlt - subl * dt / NXS_RHOS;
        del_ht = STD_MIN(hs, 0.) * qs / qi;
        hs = STD_MAX(0., hs);
        hs += snowfall / NXS_RHOS * dt;
        del_hb = (Qic - Qio) * dt / qi;
        del_hi = del_ht + del_hb;
        hi = hi + del_hi;
        mlt_hi_top = STD_MIN(del_ht, 0.);
        mlt_hi_bot = STD_MIN(del_hb, 0.);
        draft = (hi * NXS_RHOI + hs * NXS_RHOS) / NXS_RHOW;
        if (c.flooding && draft > hi) {
            del_hi_s2i += draft - hi;
            hs = hs - (draft - hi) * NXS_RHOI / NXS_RHOS;
            hi = draft;
        }
        if (hi < NXS_HMIN) {
            if (del_hi < 0.) {
                mlt_hi_top *= -hi_old / del_hi;
                mlt_hi_bot *= -hi_old / del_hi;
            }
            del_hi_s2i = 0.;
            del_hi = -hi_old;
            Qio = Qio + hi * qi / dt + hs * qs / dt;
            hi = 0.;
            hs = 0.;
            Tsurf = Tfr_ice;
        }
    }
    Qio_ = Qio; hi_ = hi; hs_ = hs; hi_old_ = hi_old; del_hi_ = del_hi; del_hs_mlt_ = del_hs_mlt; mlt_hi_top_ = mlt_hi_top; mlt_hi_bot_ = mlt_hi_bot; del_hi_s2i_ = del_hi_s2i;
    Tsurf_ = Tsurf;
}

// thermoWinton, FE.cpp:6633-6853; numbers in parentheses are the equations of Winton (2000), as in the reference
__device__ __forceinline__ void col_winton(const ColDev &c, double dt, double conc, double voli, double vols, double snowfall, double Qia, double dQiadT, double I, double subl,
                                           double Tbot, double &Qio_, double &hi_, double &hs_, double &hi_old_, double &del_hi_, double &del_hs_mlt_, double &mlt_hi_top_,
                                           double &mlt_hi_bot_, double &del_hi_s2i_, double &Tsurf_, double &T1_, double &T2_) {
    double Qio = Qio_, hi, hs, hi_old, del_hi, del_hs_mlt = del_hs_mlt_, mlt_hi_top = mlt_hi_top_, mlt_hi_bot = mlt_hi_bot_, del_hi_s2i = del_hi_s2i_, Tsurf = Tsurf_;
    double T1 = T1_, T2 = T2_;
    const double qi = NXS_LF * NXS_RHOI;
    const double qs = NXS_LF * NXS_RHOS;
    const double Crho = NXS_HEAT_C * NXS_RHOI;
    const double Tfr_ice = -c.mu * NXS_SI;
    if (conc <= 0. || voli <= 0.) {
        hi = 0.;
        hs = 0.;
        hi_old = 0.;
        del_hi = 0.;
        Tsurf = Tfr_ice;
        T1 = Tfr_ice;
        T2 = Tfr_ice;
    } else {
        hi = voli / conc;
        hi_old = hi;
        hs = vols / conc;
        const double Tfr_surf = (hs > 0) ? 0. : Tfr_ice;
        double K12 = 4 * NXS_KI * c.ks / (c.ks * hi + 4 * NXS_KI * hs);   // (5)
        double A = Qia - Tsurf * dQiadT;                                  // (7)
        double B = dQiadT;                                                // (8)
        double K32 = 2 * NXS_KI / hi;                                     // (10)
        double A1 = hi * Crho / (2 * dt) + K32 * (4 * dt * K32 + hi * Crho) / (6 * dt * K32 + hi * Crho) + K12 * B / (K12 + B);   // (16)
        double B1 = -hi / (2 * dt) * (Crho * T1 + qi * Tfr_ice / T1) - I - K32 * (4 * dt * K32 * Tbot + hi * Crho * T2) / (6 * dt * K32 + hi * Crho) + A * K12 / (K12 + B);   // (17)
        double C1 = hi * qi * Tfr_ice / (2 * dt);                         // (18)
        T1 = -(B1 + sqrt(B1 * B1 - 4 * A1 * C1)) / (2 * A1);              // (21)
        Tsurf = (K12 * T1 - A) / (K12 + B);                               // (6)
        double Msurf = 0.;
        if (Tsurf > Tfr_surf) {
            Tsurf = Tfr_surf;
            A1 += K12 - K12 * B / (K12 + B);
            B1 -= K12 * Tsurf + A * K12 / (K12 + B);
            T1 = -(B1 + sqrt(B1 * B1 - 4 * A1 * C1)) / (2 * A1);          // (21)
            Msurf = K12 * (T1 - Tsurf) - (A + B * Tsurf);                 // (22)
        }
        T2 = (2 * dt * K32 * (T1 + 2 * Tbot) + hi * Crho * T2) / (6 * dt * K32 + hi * Crho);   // (15)
        double h1 = hi / 2.;
        double h2 = hi / 2.;
        double E1 = Crho * (T1 - Tfr_ice) - qi * (1 - Tfr_ice / T1);      // (1)
        double E2 = Crho * (T2 - Tfr_ice) - qi;                           // (25)
        hs += snowfall / NXS_RHOS * dt;
        if (subl * dt <= hs * NXS_RHOS) hs -= subl * dt / NXS_RHOS;
        else if (subl * dt - hs * NXS_RHOS <= h1 * NXS_RHOI) {
            h1 -= (subl * dt - hs * NXS_RHOS) / NXS_RHOI;
            hs = 0.;
        } else if (subl * dt - h1 * NXS_RHOI - hs * NXS_RHOS <= h2 * NXS_RHOI) {
            h2 -= (subl * dt - h1 * NXS_RHOI - hs * NXS_RHOS) / NXS_RHOI;
            h1 = 0.;
            hs = 0.;
        } else {
            h2 = 0.;
            h1 = 0.;
            hs = 0.;
        }
        const double top0 = h1 + h2 - hi_old;
        mlt_hi_top = STD_MAX(0., top0);
        double Mbot = Qio - 4 * NXS_KI * (Tbot - T2) / hi;                // (23)
        del_hs_mlt = 0;
        if (Mbot <= 0.) {
            double Ebot = Crho * (Tbot - Tfr_ice) - qi;                   // (25)
            double delh2 = Mbot * dt / Ebot;                              // (24)
            T2 = (delh2 * Tbot + h2 * T2) / (delh2 + h2);                 // (26)
            h2 += delh2;
        } else {
            const double m2 = -Mbot * dt / E2;
            double delh2 = -STD_MIN(m2, h2);                              // (31)
            const double m1 = -(Mbot * dt + E2 * h2) / E1, m1p = STD_MAX(m1, 0.);
            double delh1 = -STD_MIN(m1p, h1);                             // (32)
            const double ms = (Mbot * dt + E2 * h2 + E1 * h1) / qs, msp = STD_MAX(ms, 0.);
            del_hs_mlt = -STD_MIN(msp, hs);                               // (32)
            if (h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.) {
                const double back = Mbot * dt - qs * hs + E1 * h1 + E2 * h2;
                Qio -= STD_MAX(back, 0.) / dt;                            // (34)
            }
            hs += del_hs_mlt;
            h1 += delh1;
            h2 += delh2;
            mlt_hi_bot += delh1 + delh2;
        }
        const double s0 = Msurf * dt / qs;
        del_hs_mlt -= STD_MIN(s0, hs);                                    // (27)
        const double s1 = -(Msurf * dt - qs * hs) / E1, s1p = STD_MAX(s1, 0.);
        double delh1 = -STD_MIN(s1p, h1);                                 // (28)
        const double s2 = -(Msurf * dt - qs * hs + E1 * h1) / E2, s2p = STD_MAX(s2, 0.);
        double delh2 = -STD_MIN(s2p, h2);                                 // (29)
        if (h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.) {
            const double back = Msurf * dt - qs * hs + E1 * h1 + E2 * h2;
            Qio -= STD_MAX(back, 0.) / dt;                                // (30)
        }
        hs += del_hs_mlt;
        h1 += delh1;
        h2 += delh2;
        mlt_hi_top += delh1 + delh2;
        double freeboard = (hi * (NXS_RHOW - NXS_RHOI) - hs * NXS_RHOS) / NXS_RHOW;
        if (c.flooding && freeboard < 0) {
            const double fb = freeboard * NXS_RHOI / NXS_RHOS;
            hs += STD_MIN(fb, 0.);
            const double nf = -freeboard;
            double delh1 = STD_MAX(nf, 0.);
            double f1 = 1 - delh1 / (delh1 + h1);
            double Tbar = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * Tfr_ice;   // (39)
            T1 = (Tbar - sqrt(Tbar * Tbar - 4 * Tfr_ice * qi / Crho)) / 2.;               // (38)
            h1 += delh1;
            del_hi_s2i += delh1;
        }
        hi = h1 + h2;
        if (h2 > h1) {
            double f1 = h1 / hi * 2.;
            double Tbar = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * T2;        // (39)
            T1 = (Tbar - sqrt(Tbar * Tbar - 4 * Tfr_ice * qi / Crho)) / 2.;               // (38)
        } else if (hi > 0.) {
            double f1 = (2. * h1 - hi) / hi;
            T2 = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * T2;                 // (40)
            if (T2 > Tfr_ice) {
                mlt_hi_top -= hi / 4 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1));
                mlt_hi_bot -= hi / 4 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1));
                hi -= hi / 2 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1));
                T2 = Tfr_ice;
            }
        }
        del_hi = hi - hi_old;
        if (hi < NXS_HMIN) {
            Qio -= (-qs * hs + (E1 + E2) * hi / 2.) / dt;
            if (del_hi < 0.) {
                mlt_hi_top *= -hi_old / del_hi;
                mlt_hi_bot *= -hi_old / del_hi;
            }
            del_hi_s2i = 0.;
            del_hi = -hi_old;
            hi = 0.;
            hs = 0.;
            Tsurf = Tfr_ice;
            T1 = Tfr_ice;
            T2 = Tfr_ice;
        }
    }
    Qio_ = Qio; hi_ = hi; hs_ = hs; hi_old_ = hi_old; del_hi_ = del_hi; del_hs_mlt_ = del_hs_mlt; mlt_hi_top_ = mlt_hi_top; mlt_hi_bot_ = mlt_hi_bot; del_hi_s2i_ = del_hi_s2i;
    Tsurf_ = Tsurf; T1_ = T1; T2_ = T2;
}

__global__ void __launch_bounds__(BLOCK) k_column(ColArrays a, ColDev c) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    const size_t n = (size_t)a.Ne;
    const double ddt = c.dt;
    // the snowfall in kg/m^2/s, FE.cpp:5321-5332
    double tmp_snowfall = 0.;
    if (c.snowfall_source == NXS_COL_SNOWFALL_PRECIP_SNOWFR) tmp_snowfall = a.precip[e] * a.snow[e];
    else if (c.snowfall_source == NXS_COL_SNOWFALL_SNOWFALL) tmp_snowfall = a.snow[e];
    else if (a.tair[e] < 0) tmp_snowfall = a.precip[e];
    tmp_snowfall = STD_MAX(0., tmp_snowfall);
    double mld = c.constant_mld;
    if (c.mld_source == NXS_COL_MLD_ROW) mld = a.mld[e];
    double sst = a.sst[e], sss = a.sss[e];
    // the flux due to nudging, FE.cpp:5343-5366
    double Qdw, Fdw;
    if (c.ocean_type == NXS_COL_OCEAN_CONSTANT) {
        Qdw = c.Qdw_const;
        Fdw = c.Fdw_const;
    } else if (c.ocean_type == NXS_COL_OCEAN_COUPLED) {   // FE.cpp:5348-5358: no nudging, M_sst and M_sss are reset to the values received (an attached coupled ocean)
        Qdw = 0;
        Fdw = 0;
        sst = a.ocean_temp[e];
        sss = a.ocean_salt[e];
        a.sst_reset[e] = sst;
        a.sss_reset[e] = sss;
    } else {
        Qdw = -(sst - a.ocean_temp[e]) * mld * NXS_RHOW * NXS_CPW / c.timeT;
        const double delS = sss - a.ocean_salt[e];
        Fdw = delS * mld * NXS_RHOW / (c.timeS * sss - ddt * delS);
    }
    // iceOceanHeatflux, FE.cpp:6396-6428
    const double tfrw = col_freezing_point(c, sss);
    double Qio;
    if (c.qio_type == NXS_COL_QIO_BASIC) Qio = (sst - tfrw) * NXS_RHOW * NXS_CPW * mld / c.dt;
    else {
        const int nd[3] = {a.t0[e], a.t1[e], a.t2[e]};
        double welt_oce_ice = 0.;
#pragma unroll
        for (int i = 0; i < 3; ++i) welt_oce_ice += hypot(a.VT[nd[i]] - a.ocean[nd[i]], a.VT[nd[i] + a.Nn] - a.ocean[nd[i] + a.Nn]);
        const double norm_Voce_ice = welt_oce_ice / 3.;
        Qio = (sst - tfrw) * norm_Voce_ice * c.Csens_io * NXS_RHOW * NXS_CPW;
    }
    double Qio_young = 0.;
    if (c.young_cat) Qio_young = Qio;
    a.out[COL_SNOWFALL * n + e] = tmp_snowfall; a.out[COL_QDW * n + e] = Qdw; a.out[COL_FDW * n + e] = Fdw; a.out[COL_TFRW * n + e] = tfrw;
    {   // the old ice, FE.cpp:5381-5398
        double hi = 0., hs = 0., hi_old = 0., del_hi = 0., del_hs_mlt = 0, mlt_hi_top = 0, mlt_hi_bot = 0, del_hi_s2i = 0;
        const double conc = a.conc[e], voli = a.thick[e], vols = a.snow_thick[e];
        const double Qia = a.flux[FLUX_QIA * n + e], dQiadT = a.flux[FLUX_DQIADT * n + e], I = a.flux[FLUX_I * n + e], subl = a.flux[FLUX_SUBL * n + e];
        double Tsurf = a.tice0[e];
        if (c.thermo_type == NXS_COL_THERMO_WINTON) {
            double T1 = a.tice1[e], T2 = a.tice2[e];
            col_winton(c, ddt, conc, voli, vols, tmp_snowfall, Qia, dQiadT, I, subl, tfrw, Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf, T1, T2);
            a.tice1[e] = T1; a.tice2[e] = T2;
        } else
            col_ice0(c, ddt, conc, voli, vols, tmp_snowfall, Qia, dQiadT, I, subl, tfrw, Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf);
        a.tice0[e] = Tsurf;
        double *o = a.out + COL_QIO * n + e;
        o[0] = Qio; o[n] = hi; o[2 * n] = hs; o[3 * n] = hi_old; o[4 * n] = del_hi; o[5 * n] = del_hs_mlt; o[6 * n] = mlt_hi_top; o[7 * n] = mlt_hi_bot; o[8 * n] = del_hi_s2i;
    }
    {   // the young ice, FE.cpp:5400-5411
        double hi_young = 0., hs_young = 0., hi_young_old = 0., del_hi_young = 0., del_hs_young_mlt = 0, mlt_hi_top_young = 0, mlt_hi_bot_young = 0, del_hi_s2i_young = 0;
        if (c.young_cat) {
            const double old_conc_young = a.cyoung[e];
            const double Qia = a.flux[(FLUX_YOUNG + 0) * n + e], dQiadT = a.flux[(FLUX_YOUNG + 7) * n + e], I = a.flux[(FLUX_YOUNG + 5) * n + e], subl = a.flux[(FLUX_YOUNG + 6) * n + e];
            double Tsurf = a.tsurf_young[e];
            col_ice0(c, ddt, old_conc_young, a.hyoung[e], a.hsyoung[e], tmp_snowfall, Qia, dQiadT, I, subl, tfrw, Qio_young, hi_young, hs_young, hi_young_old, del_hi_young,
                     del_hs_young_mlt, mlt_hi_top_young, mlt_hi_bot_young, del_hi_s2i_young, Tsurf);
            a.tsurf_young[e] = Tsurf;
            a.hyoung[e] = hi_young * old_conc_young;
            a.hsyoung[e] = hs_young * old_conc_young;
        }
        double *o = a.out + COL_YOUNG * n + e;
        o[0] = Qio_young; o[n] = hi_young; o[2 * n] = hs_young; o[3 * n] = hi_young_old; o[4 * n] = del_hi_young; o[5 * n] = del_hs_young_mlt; o[6 * n] = mlt_hi_top_young;
        o[7 * n] = mlt_hi_bot_young; o[8 * n] = del_hi_s2i_young;
    }
}
