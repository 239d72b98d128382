// nxs_flux_kernels.inl -- the atmospheric bulk fluxes of thermo() on the device: its "fluxes" timer, FE.cpp:5214-5277 (textually included by nxs_dyn.hip behind
// nxs_dyn_kernels.inl; include/nxs_dyn.h, nxs_dyn_flux_* / nxs_dyn_fluxes).  FE.cpp = model/finiteelement.cpp.
//   k_fluxes   OWBulkFluxes (FE.cpp:5096-5132, 5138-5158), IABulkFluxes for the old ice and, in the young-ice category, for the young ice (FE.cpp:6204-6352), with
//              specificHumidity (FE.cpp:4966-5019), albedo (FE.cpp:6454-6535), windSpeedElement (FE.cpp:6359-6370), incomingLongwave (FE.cpp:6376-6389)
// One thread = one element, ghost elements included, one launch per call.  What the three bulk computations share -- the humidity of the atmosphere, the density of
// the air, the wind speed on the element, the incoming long wave -- is formed once (the reference forms the same expressions three times: the same bits).  Every row
// is [Ne] and a thread touches entry e of it: whole lines per wave; only the three nodes' wind is gathered.  No LDS, no atomics.  Operand order is the reference's;
// the build is uncontracted (-ffp-contract=off).  Everything that does not depend on the element -- the constants block of FE.cpp:6170-6202 -- is computed by the
// host's libm and arrives in FluxDev by value.
// NOT here: the AEROBULK branch of OWBulkFluxes (a Fortran library), the OceanType::COUPLED term M_qsrml (FE.cpp:5153-5154), thermo() from FE.cpp:5279 on.

// physical::, model/constants.hpp
#define NXS_TFRWK 273.15
#define NXS_RA_DRY 287.058
#define NXS_RA_VAP 461.5
#define NXS_CPA 1000.5
#define NXS_CPV 1860.
#define NXS_LV0 2500000.
#define NXS_EPS 0.996
#define NXS_SIGMA_SB 5.67e-8
#define NXS_VONKARMAN 0.4
#define NXS_GAMMA_D 0.0098
#define NXS_PHYS_G 9.8   // physical::g (NOT physical::gravity)

#include "nxs_wind_speed.inl"   // wind_speed_element: shared with k_slab and the Moorings means

enum { FLUX_QOW = 0, FLUX_QLW_OW, FLUX_QSW_OW, FLUX_QLH_OW, FLUX_QSH_OW, FLUX_EVAP, FLUX_TAU_OW,
       FLUX_QIA, FLUX_QLWI, FLUX_QSWI, FLUX_QLHI, FLUX_QSHI, FLUX_I, FLUX_SUBL, FLUX_DQIADT, FLUX_ALBEDO, FLUX_YOUNG = 16 /* the nine rows again */, FLUX_ROWS = 25 };
enum { FLUX_ATM_ROWS = 5 /* nxs_dyn_flux_atmosphere */, FLUX_ST_ROWS = 8 /* nxs_dyn_flux_state */ };
static_assert(FLUX_ROWS == NXS_FLUX_ROWS && FLUX_TAU_OW == NXS_FLUX_TAU_OW && FLUX_YOUNG == NXS_FLUX_QIA_YOUNG && FLUX_ALBEDO == NXS_FLUX_ALBEDO, "the rows of nxs_dyn_fluxes_get");

struct FluxDev {
    int alb_scheme, hum_source, lw_source, fix_drag;
    double alb_ice, alb_sn, alb_pnd, I_0, ocean_albedo, drag_ocean_t, drag_ocean_q, zref_wind, zref_temp;
    double Linvrange, Bm, Bm2, C1, C2, C3, C4, C5, C6, C7, D1, D2, D3, D4, D5, lambda_u, lambda_h;   // FE.cpp:6170-6202
};

// the constants block of IABulkFluxes (FE.cpp:6170-6202) on the HOST, by its's libm like the reference's
static inline FluxDev flux_derive(const nxs_dyn_flux_config &c, double quad_drag_coef_air) {
    FluxDev d{};
    d.alb_scheme = c.alb_scheme; d.hum_source = c.humidity_source; d.lw_source = c.longwave_source; d.fix_drag = c.force_neutral_atmosphere != 0;
    d.alb_ice = c.alb_ice; d.alb_sn = c.alb_sn; d.alb_pnd = c.alb_ponds; d.I_0 = c.I_0; d.ocean_albedo = c.ocean_albedo;
    d.drag_ocean_t = c.drag_ocean_t; d.drag_ocean_q = c.drag_ocean_q; d.zref_wind = c.zref_wind; d.zref_temp = c.zref_temp;
    const double zref_wind = c.zref_wind;
    const double z0 = zref_wind * std::exp(-NXS_VONKARMAN / std::sqrt(quad_drag_coef_air));
    d.Linvrange = 1. / c.limiting_lengthscale;
    const double am = 5.;
    const double bm = am / 6.5;
    const double Bm = std::cbrt((1 - bm) / bm);
    const double ah = 5.;
    const double bh = 5.;
    const double ch = 3.;
    const double Bh = std::sqrt(5);
    d.Bm = Bm;
    d.C1 = -3. * am / bm;
    d.C2 = 0.5 * am * Bm / bm;
    d.C3 = 1. / (1. + Bm);
    d.Bm2 = Bm * Bm;
    d.C4 = 1. / (1. - Bm + d.Bm2);
    const double sqrt3 = std::sqrt(3.);
    d.C5 = 2. * sqrt3;
    d.C6 = 1. / (sqrt3 * Bm);
    d.C7 = std::atan((2. - Bm) * d.C6);
    d.D1 = -0.5 * bh;
    d.D2 = -ah / Bh + 0.5 * bh * ch / Bh;
    d.D3 = ch - Bh;
    d.D4 = ch + Bh;
    d.D5 = std::log(d.D3 / d.D4);
    d.lambda_u = std::log(zref_wind / z0);
    d.lambda_h = std::log(zref_wind / z0);
    return d;
}

struct FluxArrays {
    int Ne, Nn, young_cat;
    const int *t0, *t1, *t2;
    const double *wind;                                     // [2Nn] M_wind as the step's prep kernels read it
    const double *tair, *mslp, *Qsw_in, *hum, *lw;          // the atmosphere (hum: dew point, specific humidity or mixing ratio; lw: Qlw_in or tcc)
    const double *conc, *snow, *cyoung, *hsyoung;           // the state's rows
    const double *tice0, *tsurf_young, *sst, *pond, *lid;
    double *drag_ui, *drag_ti, *drag_ui_young, *drag_ti_young;   // updated in place
    double *out;                                            // [FLUX_ROWS][Ne], row FLUX_TAU_OW unused:
    double *tau_ow;                                         // D_tau_ow is the row the Moorings means read
    const double *qsrml;                                    // [Ne] M_qsrml of an attached coupled ocean (nxs_dyn_ocean_coupled_*), NULL without one
};

struct FluxAtm { double mslp, tair, sphuma, rhoair, wspeed, Qsw_in, Qlw_in; };

// FE.cpp:5004-5006 for ATMOSPHERE (ice == false) and ICE (ice == true); salinity is 0 in both: est * (1 - 5.37e-4 * 0)
template <bool ICE>
__device__ __forceinline__ double flux_sphum(double temp, double mslp, double *dsphumdT) {
    const double A = ICE ? 2.2e-4 : 7.2e-4, B = ICE ? 3.83e-6 : 3.20e-6, C = ICE ? 6.4e-10 : 5.9e-10;
    const double a = ICE ? 6.1115e2 : 6.1121e2, b = ICE ? 23.036 : 18.729, c = ICE ? 279.82 : 257.87, d = ICE ? 333.7 : 227.3;
    const double alpha = 0.62197, beta = 0.37803, salinity = 0;
    const double f = 1. + A + mslp * 1e-2 * (B + C * temp * temp);
    const double est = a * exp((b - temp / d) * temp / (temp + c)) * (1 - 5.37e-4 * salinity);
    const double sphum = alpha * f * est / (mslp - beta * f * est);
    if (ICE) {   // FE.cpp:5011-5013
        const double dfdT = 2. * C * B * temp;
        const double destdT = (b * c * d - temp * (2. * c + temp)) / (d * pow(c + temp, 2.)) * est;
        *dsphumdT = alpha * mslp * (f * destdT + est * dfdT) / pow(mslp - beta * est * f, 2.);
    }
    return sphum;
}

// albedo(), FE.cpp:6454-6535 (the scheme is 1..4: nxs_dyn_flux_configure refuses every other)
__device__ __forceinline__ void flux_albedo(const FluxDev &c, double Tsurf, double hs, double frac_pnd, double *alb, double *pen) {
    double albedo, pen_sw;
    if (c.alb_scheme <= 2) {
        if (hs > 0.) {
            if (c.alb_scheme == 2) albedo = STD_MIN(c.alb_sn, c.alb_ice + (c.alb_sn - c.alb_ice) * hs / 0.2);
            else albedo = c.alb_sn;
            pen_sw = 0.;
        } else {
            albedo = c.alb_ice;
            pen_sw = c.I_0;
        }
    } else if (c.alb_scheme == 3) {
        double albi, albs;
        if (Tsurf > -1.) {
            albi = c.alb_ice - 0.075 * (Tsurf + 1.);
            albs = c.alb_sn - 0.124 * (Tsurf + 1.);
        } else {
            albi = c.alb_ice;
            albs = c.alb_sn;
        }
        const double frac_sn = hs / (hs + 0.02);
        albedo = frac_sn * albs + frac_pnd * c.alb_pnd + (1. - frac_sn - frac_pnd) * albi;
        pen_sw = (1. - frac_sn - frac_pnd) * c.I_0;
    } else {
        const double frac_sn = hs / (hs + 0.02);
        double albs;
        if (Tsurf > -1.) albs = c.alb_sn - 0.124 * (Tsurf + 1.);
        else albs = c.alb_sn;
        albedo = frac_sn * albs + frac_pnd * c.alb_pnd + (1. - frac_sn - frac_pnd) * c.alb_ice;
        pen_sw = (1. - frac_sn - frac_pnd) * c.I_0;
    }
    *alb = albedo; *pen = pen_sw;
}

// one element of IABulkFluxes' loop, FE.cpp:6204-6352; rows: the nine outputs from FLUX_QIA (or FLUX_YOUNG) on
__device__ __forceinline__ void flux_ice(const FluxDev &c, const FluxAtm &at, int e, int Ne, double Tsurf, double snow_thick, double conc, double pond_frac_in, double lid,
                                         bool bulk_for_young, double *drag_ui_p, double *drag_ti_p, double *rows) {
    const double Qlw_out = NXS_EPS * NXS_SIGMA_SB * pow(Tsurf + NXS_TFRWK, 4.);
    const double dQlwdT = 4. * NXS_EPS * NXS_SIGMA_SB * pow(Tsurf + NXS_TFRWK, 3.);
    double dsphumidT;
    const double sphumi = flux_sphum<true>(Tsurf, at.mslp, &dsphumidT);
    const double sphuma = at.sphuma;
    const double tairK = at.tair + NXS_TFRWK;
    const double tsurfK = Tsurf + NXS_TFRWK;
    const double rhoair = at.rhoair;
    const double wspeed = at.wspeed;
    const double Tpot = tairK + NXS_GAMMA_D * c.zref_temp;
    double drag_ti = drag_ti_p[e];
    if (!c.fix_drag) {
        const double retv = 0.6078;
        double drag_ui = drag_ui_p[e];
        const double ustar = sqrt(drag_ui) * wspeed;
        const double Tvirt = Tpot * (1. + retv * sphuma);
        const double mixrat = sphuma / (1. - sphuma);
        const double wTpot = drag_ti * wspeed * (tsurfK - Tpot);
        const double wr = drag_ti * wspeed * (sphumi - sphuma) / ((1. - sphumi) * (1. - sphuma));
        const double wTvirt = wTpot * (1. + retv * mixrat) + retv * Tpot * wr;
        // (calm wind: ustar == 0 and the quotient is 0 / 0; std::min(Linvrange, NaN) is Linvrange)
        const double q = -NXS_VONKARMAN * NXS_PHYS_G * wTvirt / (ustar * ustar * ustar * Tvirt);
        const double lo = -c.Linvrange, inner = STD_MIN(c.Linvrange, q);
        const double Linv = STD_MAX(lo, inner);
        const double zetam = c.zref_wind * Linv;
        const double zetah = c.zref_temp * Linv;
        double psim, psih;
        if (Linv >= 0) {
            const double x = cbrt(1. + zetam);
            psim = c.C1 * (x - 1.) + c.C2 * (2. * log((x + c.Bm) * c.C3) - log((x * x - x * c.Bm + c.Bm2) * c.C4) + c.C5 * (atan((2. * x - c.Bm) * c.C6) - c.C7));
            psih = c.D1 * log(1. + 3. * zetah + zetah * zetah) + c.D2 * (log((2. * zetah + c.D3) / (2. * zetah + c.D4)) - c.D5);   // ch = 3.
        } else {
            double x = sqrt(sqrt(1. - 16. * zetam));
            psim = 2. * log(0.5 * (1. + x)) + log(0.5 * (1. + x * x)) - 2. * atan(x) + 0.5 * NXS_PI;
            x = sqrt(sqrt(1. - 16. * zetah));
            psih = 2. * log(0.5 * (1. + x * x));
        }
        drag_ui = NXS_VONKARMAN / (c.lambda_u - psim);
        drag_ui *= drag_ui;
        drag_ti = NXS_VONKARMAN / (c.lambda_h - psih);
        drag_ti *= drag_ti;
        drag_ui_p[e] = drag_ui;
        drag_ti_p[e] = drag_ti;
    }
    const double Qsh = drag_ti * rhoair * NXS_CPA * wspeed * (tsurfK - Tpot);
    const double dQshdT = drag_ti * rhoair * NXS_CPA * wspeed;
    const double Lsub = NXS_LF + NXS_LV0 - 240. - 290. * Tsurf - 4. * Tsurf * Tsurf;
    const double Qlh = drag_ti * rhoair * Lsub * wspeed * (sphumi - sphuma);
    const double dQlhdT = drag_ti * Lsub * rhoair * wspeed * dsphumidT;
    const double dQiadT = dQlwdT + dQshdT + dQlhdT;
    const double ql = Qlh / Lsub;
    const double subl = STD_MAX(0., ql);
    double hs;
    if (conc > 0) hs = snow_thick / conc;
    else hs = 0;
    double pond_fraction;
    if (pond_frac_in > 0. && lid / pond_frac_in <= 0.05) pond_fraction = pond_frac_in;
    else pond_fraction = 0.;
    if (bulk_for_young) pond_fraction = 0.;
    double alb_tot, pen_sw;
    flux_albedo(c, Tsurf, hs, pond_fraction, &alb_tot, &pen_sw);
    const double Qsw = -at.Qsw_in * (1. - alb_tot) * (1. - pen_sw);
    const double I = at.Qsw_in * (1. - alb_tot) * pen_sw;
    const double Qlw = Qlw_out - at.Qlw_in;
    const double Qia = Qsw + Qlw + Qsh + Qlh;
    const size_t n = (size_t)Ne;
    rows[0 * n + e] = Qia; rows[1 * n + e] = Qlw; rows[2 * n + e] = Qsw; rows[3 * n + e] = Qlh; rows[4 * n + e] = Qsh;
    rows[5 * n + e] = I; rows[6 * n + e] = subl; rows[7 * n + e] = dQiadT; rows[8 * n + e] = alb_tot;
}

__global__ void __launch_bounds__(BLOCK) k_fluxes(FluxArrays a, FluxDev c) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    const size_t n = (size_t)a.Ne;
    FluxAtm at;
    at.mslp = a.mslp[e]; at.tair = a.tair[e]; at.Qsw_in = a.Qsw_in[e];
    // specificHumidity(ATMOSPHERE), FE.cpp:4979-4987: M_sphuma, M_mixrat or the dew point, in that precedence
    const double hum = a.hum[e];
    if (c.hum_source == NXS_FLUX_HUM_SPHUMA) at.sphuma = STD_MAX(0., hum);
    else if (c.hum_source == NXS_FLUX_HUM_MIXRAT) at.sphuma = hum / (1. + hum);
    else at.sphuma = flux_sphum<false>(hum, at.mslp, nullptr);
    // incomingLongwave, FE.cpp:6376-6389
    if (c.lw_source == NXS_FLUX_LW_QLW_IN) at.Qlw_in = a.lw[e];
    else {
        const double taa = at.tair + NXS_TFRWK;
        at.Qlw_in = NXS_SIGMA_SB * pow(taa, 4.) * (1. - 0.261 * exp(-7.77e-4 * pow(taa - NXS_TFRWK, 2.))) * (1. + 0.275 * a.lw[e]);
    }
    at.wspeed = wind_speed_element(a.wind, a.Nn, a.t0[e], a.t1[e], a.t2[e]);   // windSpeedElement, FE.cpp:6359-6370
    at.rhoair = at.mslp / (NXS_RA_DRY * (at.tair + NXS_TFRWK)) * (1. - at.sphuma * (1. - NXS_RA_VAP / NXS_RA_DRY));   // FE.cpp:5110, 6227
    {   // OWBulkFluxes, FE.cpp:5096-5132 and 5138-5158
        const double sst = a.sst[e];
        const double sphumw = 640380. / NXS_RHOA * exp(-5107.4 / (sst + NXS_TFRWK));   // specificHumidity(WATER), FE.cpp:4992-4993
        const double Qsh = c.drag_ocean_t * at.rhoair * (NXS_CPA + at.sphuma * NXS_CPV) * at.wspeed * (sst - at.tair);
        const double Lv = NXS_LV0 - 2.36418e3 * sst + 1.58927 * sst * sst - 6.14342e-2 * pow(sst, 3.);
        const double ql = c.drag_ocean_q * NXS_RHOA * Lv * at.wspeed * (sphumw - at.sphuma);
        const double Qlh = STD_MAX(ql, 0.);
        const double evap = Qlh / Lv;
        const double inner = STD_MIN(2., 0.61 + 0.063 * at.wspeed);
        const double drag_ocean_m = 1e-3 * STD_MAX(1., inner);
        const double Qsw = -at.Qsw_in * (1. - c.ocean_albedo);
        const double Qlw_out = NXS_EPS * NXS_SIGMA_SB * pow(sst + NXS_TFRWK, 4.);
        const double Qlw = Qlw_out - at.Qlw_in;
        double Qow = Qlw + Qsh + Qlh;
        if (a.qsrml) Qow += Qsw * a.qsrml[e];   // OceanType::COUPLED, FE.cpp:5150-5157: the short wave the ocean's first layer absorbs
        else Qow += Qsw;
        a.out[FLUX_QOW * n + e] = Qow; a.out[FLUX_QLW_OW * n + e] = Qlw; a.out[FLUX_QSW_OW * n + e] = Qsw; a.out[FLUX_QLH_OW * n + e] = Qlh;
        a.out[FLUX_QSH_OW * n + e] = Qsh; a.out[FLUX_EVAP * n + e] = evap;
        a.tau_ow[e] = at.rhoair * drag_ocean_m;
    }
    // thermo(), FE.cpp:5245-5273
    flux_ice(c, at, e, a.Ne, a.tice0[e], a.snow[e], a.conc[e], a.pond[e], a.lid[e], false, a.drag_ui, a.drag_ti, a.out + FLUX_QIA * n);
    if (a.young_cat) flux_ice(c, at, e, a.Ne, a.tsurf_young[e], a.hsyoung[e], a.cyoung[e], a.pond[e], a.lid[e], true, a.drag_ui_young, a.drag_ti_young, a.out + FLUX_YOUNG * n);
    else {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.out[(FLUX_YOUNG + k) * n + e] = 0.;
    }
}
