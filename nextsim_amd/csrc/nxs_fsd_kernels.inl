// nxs_fsd_kernels.inl -- the floe-size distribution of the wave-coupled build (#ifdef OASIS, M_num_fsd_bins > 0) on the device (textually included by
// nxs_dyn.hip behind nxs_dyn_kernels.inl; include/nxs_dyn.h, nxs_dyn_fsd_*).  FE.cpp = model/finiteelement.cpp.
//   k_fsd_init      FE.cpp:7562-7576   the distribution at the end of initFsd()
//   k_fsd_update    FE.cpp:4674-4732   updateFSD()
//   k_fsd_breakup   FE.cpp:4268-4483   redistributeFSD()
//   k_fsd_weld      FE.cpp:4737-4870, 5888-5896   weldingRoach() + the mechanical healing of thermo()
// One thread = one element, its bins in registers: the kernels are builds for NB = 2, 6, 12, 16 bins at most (the runtime number n <= NB guards every unrolled
// loop), so that the register arrays are indexed by compile-time constants and nothing goes to scratch memory (checked on the built library, see k_fsd_breakup).  The rows are bin-major ([k][Ne]): lane e of a wave
// reads fsd[k * Ne + e], a whole line per bin.  Operand order is the reference's; the build is uncontracted (-ffp-contract=off).
static_assert(NXS_FSD_MAX_BINS == 16, "the builds of the FSD kernels end at 16 bins");
#define NXS_FSD_G 9.8   // physical::g, model/constants.hpp:35 (NOT physical::gravity)

// what nxs_dyn_fsd_configure uploads: the options and tables the loops read, and everything that does not depend on the element (host libm)
struct FsdDev {
    int n, breakup_type, damage_type, welding_type, distinguish, debug, cell_avg, pad0;
    double coef1, coef2, coef3, prob_cutoff;
    double pfac[2];          // P_inf * (1. - exp(-P_inf * cpl_time_step / tau_w)) for P_inf = 0 and 1 (FE.cpp:4335)
    double pi4_young;        // pow(PI, 4) * M_floes_flex_young (FE.cpp:4312)
    double dflex_den;        // 48 * rhow * g * (1 - pow(poisson, 2)) (FE.cpp:4313)
    double thick_min, damage_max, kappa, log_ksi;
    double centres[NXS_FSD_MAX_BINS], low[NXS_FSD_MAX_BINS], up[NXS_FSD_MAX_BINS];
    double asu[NXS_FSD_MAX_BINS], asc[NXS_FSD_MAX_BINS], asb[NXS_FSD_MAX_BINS];   // M_fsd_area_scaled_up, _centered, _binwidth
    double beta[NXS_FSD_MAX_BINS][NXS_FSD_MAX_BINS];   // [j][k], k <= j: the redistributor of ZHANG / UNIFORM_SIZE (FE.cpp:4361, 4380-4381)
    int alpha[NXS_FSD_MAX_BINS][NXS_FSD_MAX_BINS];     // M_alpha_fsd_merge[kx][ky]
    double widths[NXS_FSD_MAX_BINS];                   // M_fsd_bin_widths (redistributeThermoFSD, melt_type 3: nxs_slab_fsd_kernels.inl); last, the other offsets stay
};

// the arrays of one launch
struct FsdArrays {
    int Ne, young_cat;
    double *fsd, *mech;                  // [n][Ne]; mech NULL = not attached
    double *cum, *cumw;                  // [Ne] M_cum_damage, M_cum_wave_damage; NULL = not attached
    const double *conc, *cyoung, *thick, *hyoung, *theal;
    double *damage; int dstride;         // M_damage[e] = damage[e * dstride]: the array, or the fourth word of the sub-step loop's records (k_pack_state)
    int *flags;                          // [0] M_breakup_in_dt, [1] crash of redistributeFSD, [2] crash of weldingRoach
};
enum { FSD_FLAG_BREAKUP = 0, FSD_FLAG_CRASH = 1, FSD_FLAG_WELD_CRASH = 2, FSD_FLAGS = 4 };

// one store per wave that saw the condition (every lane would store the same value)
__device__ __forceinline__ void fsd_raise(int *flag, bool mine) {
    const unsigned long long b = __ballot(mine);
    if (mine && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) *flag = 1;
}

// FE.cpp:7562-7576
__global__ void __launch_bounds__(BLOCK) k_fsd_init(FsdArrays a, const FsdDev *__restrict__ c) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    const int n = c->n;
    double top = a.conc[e];
    if (a.young_cat) top += a.cyoung[e];
    for (int k = 0; k < n; ++k) {
        const double v = (k == n - 1) ? top : 0.;
        a.fsd[(size_t)k * a.Ne + e] = v;
        if (c->distinguish) a.mech[(size_t)k * a.Ne + e] = v;
    }
}

// the body of updateFSD for one set of bins (FE.cpp:4687-4706 and 4710-4728); true when a bin was written
template <int NB>
__device__ __forceinline__ bool fsd_rescale(double (&b)[NB], int n, double ctot) {
    double ctot2 = b[0];
#pragma unroll
    for (int j = 1; j < NB; ++j) if (j < n) ctot2 += b[j];
    if (ctot >= 1.) {   // "Before ridge creation": ctot / ctot2 also where ctot2 == 0, as written
#pragma unroll
        for (int k = 0; k < NB; ++k) if (k < n) b[k] *= ctot / ctot2;
        return true;
    }
    if (fabs(ctot - ctot2) > 1e-11) {
        if ((ctot2 == 0.) && (ctot > 0.)) {
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k == n - 1) b[k] = ctot;
        } else {
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k < n) b[k] *= ctot / ctot2;
        }
        return true;
    }
    return false;
}

template <int NB>
__global__ void __launch_bounds__(BLOCK) k_fsd_update(FsdArrays a, const FsdDev *__restrict__ c) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    const int n = c->n;
    double ctot = a.conc[e];
    if (a.young_cat) ctot += a.cyoung[e];
    for (int pass = 0; pass < (c->distinguish ? 2 : 1); ++pass) {
        double *rows = pass ? a.mech : a.fsd;
        double b[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) b[k] = (k < n) ? rows[(size_t)k * a.Ne + e] : 0.;
        if (fsd_rescale<NB>(b, n, ctot)) {
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k < n) rows[(size_t)k * a.Ne + e] = b[k];
        }
    }
}

// The builds for 12 and 16 bins: the optimizer reports that it did NOT unroll the loop over the bins j as asked (its body holds three pow, two tanh and a log), and
// the report is silenced below.  So that b[] and P[] stay in registers there rests on what the backend does with the rolled loop today, not on the source: it emits
// ScratchSize 0 and 167 / 180 VGPRs (ROCm 7.2).  tests/test_fsd_abi.py::test_no_fsd_kernel_uses_scratch_memory reads the private segment size and the VGPR spill count
// of every k_fsd_* build from the library and fails if that changes; `make resource-usage` prints the same figures.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <int NB>
__global__ void __launch_bounds__(BLOCK) k_fsd_breakup(FsdArrays a, const FsdDev *__restrict__ c, const double *__restrict__ wlbk) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = e < a.Ne;
    const int n = c->n;
    bool broke = false, crash = false;
    if (in) {
        double ctot = a.conc[e];
        if (a.young_cat) ctot += a.cyoung[e];
        if (ctot > 0.) {
            double P_inf = 0.;   // "don't try to break if there are no waves"
            const double lambda = wlbk[e];
            if (lambda < 500. - 1.) P_inf = 1.;
            if (!(P_inf <= c->prob_cutoff)) {
                broke = true;
                // "As break-up indeed occurs reset real FSD to mechanical FSD"
                const double *src = c->distinguish ? a.mech : a.fsd;
                double b[NB], P[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) b[k] = (k < n) ? src[(size_t)k * a.Ne + e] : 0.;
                const double thick = a.thick[e];
                double sea_ice_thickness = 0;
                if (c->cell_avg) sea_ice_thickness = thick;
                else if (a.young_cat) sea_ice_thickness = (thick + a.hyoung[e]) / ctot;
                sea_ice_thickness = STD_MAX(c->thick_min, sea_ice_thickness);
                const double d_flex = 0.5 * pow(c->pi4_young * pow(sea_ice_thickness, 3.) / c->dflex_den, 0.25);
                const double Pj = c->pfac[P_inf == 1. ? 1 : 0];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    P[j] = 0.;
                    if (j < n) {
                        P[j] = Pj;
                        double broken_area = 0.;
                        const double lim_lambda = STD_MAX(0., tanh((c->centres[j] - c->coef1 * lambda) / (c->coef2 * lambda)));
                        const double lim_dflex = STD_MAX(0., tanh((c->centres[j] - d_flex) / (c->coef3 * d_flex)));
                        if (c->breakup_type == NXS_BREAKUP_ZHANG || c->breakup_type == NXS_BREAKUP_UNIFORM_SIZE) {
                            P[j] = P[j] * lim_dflex * lim_lambda;
                            if (P[j] > 0.) {
                                broken_area = b[j] * P[j];
                                b[j] -= broken_area;
#pragma unroll
                                for (int k = 0; k < NB; ++k) if (k <= j) b[k] += broken_area * c->beta[j][k];   // "redistribution also occurs within the broken category"
                            }
                        } else if (c->breakup_type == NXS_BREAKUP_DUMONT) {
                            const double fragility = lim_dflex * lim_lambda;
                            if (fragility > 0) {
                                broken_area = b[j] * P[j] * fragility;
                                b[j] -= broken_area;
                                const double exponent = STD_MAX(2. - (2. + log(fragility) / c->log_ksi), 1e-6);
                                const double den = pow(c->up[j], exponent) - pow(c->low[0], exponent);
#pragma unroll
                                for (int k = 0; k < NB; ++k)
                                    if (k <= j) {
                                        const double beta = (pow(c->up[k], exponent) - pow(c->low[k], exponent)) / den;
                                        b[k] += broken_area * beta;
                                    }
                            }
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    if (k < n) {
                        a.fsd[(size_t)k * a.Ne + e] = b[k];
                        if (c->distinguish) a.mech[(size_t)k * a.Ne + e] = b[k];   // "Ensure that mech FSD and real FSD are the same after break-up"
                    }
                // Mini Checkfields
                double ctot2 = b[0];
#pragma unroll
                for (int j = 1; j < NB; ++j) if (j < n) ctot2 += b[j];
                if ((fabs(ctot - ctot2) > 2e-7) && c->debug) crash = true;
                if (thick > 0.) {   // "only thick ice can be damaged"
                    const double dmg = a.damage[(size_t)e * a.dstride];
                    double tmp = dmg;
                    if (c->damage_type != 0) {   // M_conc_mech_fsd: the bins just written where the two are kept the same, else the attached rows
                        double m[NB];
#pragma unroll
                        for (int k = 0; k < NB; ++k) m[k] = (k < n) ? (c->distinguish ? b[k] : a.mech[(size_t)k * a.Ne + e]) : 0.;
                        if (c->damage_type == 1) {   // no break in the reference (FE.cpp:4454): the value is overwritten by case 2 below
#pragma unroll
                            for (int k = 0; k < NB; ++k) if (k == n - 1) tmp = STD_MAX(dmg, 1. - m[k] / ctot);
                        }
                        double tot_broken_area = m[0] * P[0];
#pragma unroll
                        for (int j = 1; j < NB; ++j) if (j < n) tot_broken_area += m[j] * P[j];
                        tmp = dmg * (1. - tot_broken_area / ctot) + tot_broken_area / ctot * c->damage_max;
                    }
                    const double inc = STD_MAX(tmp - dmg, 0.);
                    if (a.cumw) a.cumw[e] += inc;
                    if (a.cum) a.cum[e] += inc;
                    a.damage[(size_t)e * a.dstride] = STD_MAX(dmg, STD_MIN(tmp, c->damage_max));
                }
            }
        } else {
            for (int k = 0; k < n; ++k) {
                a.fsd[(size_t)k * a.Ne + e] = 0.;
                if (a.mech) a.mech[(size_t)k * a.Ne + e] = 0.;
            }
        }
    }
    fsd_raise(a.flags + FSD_FLAG_BREAKUP, broke);
    fsd_raise(a.flags + FSD_FLAG_CRASH, crash);
}

#pragma clang diagnostic pop

template <int NB>
__global__ void __launch_bounds__(BLOCK) k_fsd_weld(FsdArrays a, const FsdDev *__restrict__ c, double ddt, const unsigned char *__restrict__ freezing) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const int n = c->n;
    bool crash = false;
    if (e < a.Ne && freezing[e]) {
        double tmp[NB];   // M_conc_fsd[..][cpt], then tmp_conc_fsd, then M_conc_fsd again
#pragma unroll
        for (int k = 0; k < NB; ++k) tmp[k] = (k < n) ? a.fsd[(size_t)k * a.Ne + e] : 0.;
        if (c->welding_type == NXS_WELDING_ROACH) {
#define FSD_WELD_MERGED() ((void)0)
#include "nxs_fsd_weld_body.inl"
#undef FSD_WELD_MERGED
        }
        if (c->distinguish) {   // FE.cpp:5888-5896
            const double w = STD_MIN(1., ddt / a.theal[e]);
#pragma unroll
            for (int m = 0; m < NB; ++m)
                if (m < n) {
                    double *q = a.mech + (size_t)m * a.Ne + e;
                    *q = *q * (1. - w) + w * tmp[m];
                }
        }
    }
    fsd_raise(a.flags + FSD_FLAG_WELD_CRASH, crash);
}
