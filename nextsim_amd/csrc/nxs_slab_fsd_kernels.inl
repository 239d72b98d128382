// nxs_slab_fsd_kernels.inl -- thermo()'s slab loop with floe-size bins attached, FE.cpp:5413-6133 as an OASIS build compiles it (textually included by nxs_dyn.hip
// behind nxs_slab_kernels.inl; include/nxs_dyn.h, nxs_dyn_slab_coupled).  FE.cpp = model/finiteelement.cpp.  Two launches on the handle's stream:
//   k_coupled_thermo   slab_element<true> (nxs_slab_kernels.inl): k_slab's loop plus melt_type 3 (FE.cpp:5592-5640).  The bins are not held: the unbroken test needs
//                      M_conc_fsd[nb-1], the melt rate M_conc_fsd[0] and one running sum over j < nb - 1 in the reference's order, so they are read as a stream.  It
//                      leaves old_conc, old_conc_young, lat_melt_rate and young_ice_growth as four rows and NXS_SLAB_BR_LIMIT in the branch word
//   k_coupled_bins     the FSD branches of the limit block (FE.cpp:5729-5764), else under melt_type 3 redistributeThermoFSD (5768-5776, 4487-4670); the in-loop
//                      weldingRoach where del_hi > 0 (5779-5797: nxs_fsd_weld_body.inl, k_fsd_weld's own statements); 9.b, the mechanical healing
//                      (5883-5898).  M_conc_young is not written after FE.cpp:5637, M_conc not after 5719 and M_time_relaxation_damage not after 5879: all three
//                      are final when the first launch has ended, and the column's del_hi row is read-only.
// k_coupled_bins is one thread = one element with its bins in registers, builds for NB = 2, 6, 12, 16 like k_fsd_* (compile-time indices, selects for bin n - 1:
// nothing goes to scratch memory; tests/test_slab_fsd_abi.py reads that from the library).  The mechanical bins are worked on in a pass of their own at the end,
// when only the final bins are still live.  Bin-major rows: whole lines per wave, no LDS, no atomics.  Operand order, divisions and the argument order of std::max /
// std::min are the reference's; the build is uncontracted.
// Not here, they need the coupled ocean's received fields: the OceanType::COUPLED guards (FE.cpp:5826-5841), their counterpart in the column (5348-5358), M_qsrml
// (5150-5156).

__global__ void __launch_bounds__(BLOCK) k_coupled_thermo(SlabArrays a, SlabDev c, SlabCoupled x) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.Ne) return;
    slab_element<true>(a, c, x, e);
}

struct CoupledBins {
    double ddt;
    int melt_type;
    const double *scr;        // [SLAB_SCR_ROWS][Ne] of the first launch
    const double *del_hi;     // [Ne] the column's row
    const unsigned *br;       // [Ne] NXS_SLAB_BR_* of the first launch
    unsigned *br2;            // [Ne] NXS_SLAB_FSD_BR_*: the first launch's bits, completed here
    int *crash;               // thermo_fsd_crash
};

template <int NB>
__global__ void __launch_bounds__(BLOCK) k_coupled_bins(FsdArrays a, const FsdDev *__restrict__ c, CoupledBins x) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const int n = c->n;
    bool crash = false, weld_crash = false;
    if (e < a.Ne) {
        const size_t N = (size_t)a.Ne;
        const bool young = a.young_cat != 0, dist = c->distinguish != 0;
        const double ddt = x.ddt;
        unsigned br2 = x.br2[e];
        const bool limit = (x.br[e] & NXS_SLAB_BR_LIMIT) != 0;
        const bool redist = !limit && x.melt_type == 3;
        const double conc = a.conc[e];
        double cy = 0.;
        if (young) cy = a.cyoung[e];
        const double old_conc = x.scr[SLAB_SCR_OLD_CONC * N + e];
        double del_c_fsd = 0.;   // redistributeThermoFSD's, kept for the mechanical bins
        bool store = false;
        double b[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) b[k] = (k < n) ? a.fsd[(size_t)k * N + e] : 0.;
        if (limit) {   // FE.cpp:5732-5763
            double ctot = 0;
#pragma unroll
            for (int m = 0; m < NB; ++m) if (m < n) ctot += b[m];
            if ((ctot > old_conc) && young && (cy > 0.)) {
                br2 |= NXS_SLAB_FSD_BR_LIMIT_RESCALED;
#pragma unroll
                for (int m = 0; m < NB; ++m) if (m < n) b[m] += (-old_conc) * b[m] / ctot;
                store = true;
            }
            if (!dist) {   // the else of FE.cpp:5754 belongs to if (M_distinguish_mech_fsd)
                br2 |= NXS_SLAB_FSD_BR_LIMIT_ZEROED;
#pragma unroll
                for (int k = 0; k < NB; ++k) b[k] = 0.;
                store = true;
            }
        } else if (redist) {   // redistributeThermoFSD, FE.cpp:4487-4670
            const double old_conc_young = x.scr[SLAB_SCR_OLD_CONC_YOUNG * N + e], lat_melt_rate = x.scr[SLAB_SCR_LAT_MELT_RATE * N + e],
                         young_ice_growth = x.scr[SLAB_SCR_YOUNG_ICE_GROWTH * N + e];
            double del_c_young = 0.;
            del_c_fsd = conc - old_conc;
            double cat0_del_c = 0.;
            double ctot_init = 0.;
#pragma unroll
            for (int m = 0; m < NB; ++m) if (m < n) ctot_init += b[m];
            if (young) del_c_young = cy - old_conc_young;
            del_c_fsd += del_c_young;
            if ((fabs(lat_melt_rate) > 0.) && (ctot_init > 1e-12)) {
                br2 |= NXS_SLAB_FSD_BR_LATERAL;
                double fsd_init[NB];
#pragma unroll
                for (int m = 0; m < NB; ++m) fsd_init[m] = b[m];
                // fsd_dr[m] = M_conc_fsd[m] / M_fsd_bin_widths[m] for 1 <= m < n - 1 and 0. elsewhere ([n + 1] entries); dfsd_dr[m] = fsd_dr[m + 1] - fsd_dr[m].
                // The loop of FE.cpp:4545 changes M_conc_fsd[m] only behind the last reading of fsd_dr[m], so the quotients are taken of fsd_init, when they are needed
                if (c->debug) {
                    double sum = 0.;
#pragma unroll
                    for (int m = 0; m < NB; ++m)
                        if (m < n) {
                            const double lo = (m >= 1 && m < n - 1) ? fsd_init[m] / c->widths[m] : 0.;
                            const double up = (m + 1 < NB && m + 1 < n - 1) ? fsd_init[m + 1 < NB ? m + 1 : m] / c->widths[m + 1 < NB ? m + 1 : m] : 0.;
                            sum += up - lo;
                        }
                    if (fabs(sum) > 1e-11) crash = true;
                }
#pragma unroll
                for (int m = 0; m < NB; ++m)
                    if (m < n - 1) {
                        const double lo = (m >= 1) ? fsd_init[m] / c->widths[m] : 0.;
                        const double up = (m + 1 < NB && m + 1 < n - 1) ? fsd_init[m + 1 < NB ? m + 1 : m] / c->widths[m + 1 < NB ? m + 1 : m] : 0.;
                        const double dfsd_dr = up - lo;
                        const double del_c_bin_melt = ddt * lat_melt_rate * (-dfsd_dr + fsd_init[m] * 2. / c->centres[m]);
                        b[m] = b[m] + del_c_bin_melt;
                    }
                if (lat_melt_rate < 0.) {
                    br2 |= NXS_SLAB_FSD_BR_LAT_MELTING;
                    cat0_del_c = lat_melt_rate * fsd_init[0] / c->widths[0] * ddt;
                    b[0] += cat0_del_c;
                } else {
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m == n - 1) b[m] += fsd_init[m] / c->widths[m] * ddt * lat_melt_rate;
                }
                double ctot = 0.;
#pragma unroll
                for (int m = 0; m < NB; ++m) if (m < n) ctot += b[m];
                if (young_ice_growth < 0) {
                    br2 |= NXS_SLAB_FSD_BR_YOUNG_SHRINKS;
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m < n) b[m] += (young_ice_growth) * b[m] / ctot;
                }
                if (c->debug) {
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m == n - 1 && b[m] < -1e-11) crash = true;
                }
            } else {   // refreezing
                if (young) {
                    if (conc + cy == 1.) {
                        br2 |= NXS_SLAB_FSD_BR_FILLS_LEAD;
#pragma unroll
                        for (int m = 0; m < NB; ++m) b[m] = (m == n - 1) ? 1. : 0.;
                    } else if (del_c_fsd >= 0) {
                        br2 |= NXS_SLAB_FSD_BR_DEL_C_FSD_GE0;
#pragma unroll
                        for (int m = 0; m < NB; ++m) if (m == n - 1) b[m] += del_c_fsd;
                    } else {
#pragma unroll
                        for (int m = 0; m < NB; ++m) if (m < n) b[m] += del_c_fsd * b[m] / ctot_init;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m == n - 1) b[m] += del_c_fsd;
                }
            }
            store = true;
            if (c->debug) {   // FE.cpp:4617-4640 (the mechanical bins' sum, 4641: below)
#pragma unroll
                for (int m = 0; m < NB; ++m) if (m == n - 1 && b[m] < -1e-11) crash = true;
                double ctot = conc;
                if (young) ctot += cy;
                double ctot2 = b[0];
#pragma unroll
                for (int j = 1; j < NB; ++j) if (j < n) ctot2 += b[j];
                if (fabs(ctot - ctot2) > 1e-7) crash = true;
            }
        }
        if (store) {
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k < n) a.fsd[(size_t)k * N + e] = b[k];
        }
        // 6.b) FE.cpp:5783-5796
        const bool freezing = x.del_hi[e] > 0.;
        if (freezing && c->welding_type == NXS_WELDING_ROACH) {
            // the names nxs_fsd_weld_body.inl works on (its header lists them): tmp IS b, and `crash` SHADOWS this kernel's own flag on purpose, so that the
            // welding's conditions raise weld_crash (FSD_FLAG_WELD_CRASH) and not thermo_fsd_crash; c, n, ddt, a and e are the kernel's
            double (&tmp)[NB] = b;
            bool &crash = weld_crash;
#define FSD_WELD_MERGED() br2 |= NXS_SLAB_FSD_BR_WELDED
#include "nxs_fsd_weld_body.inl"
#undef FSD_WELD_MERGED
        }
        // the mechanical bins: FE.cpp:5744-5753, 4601-4613, 4631-4646, 5888-5896, in that order
        if (dist && (limit || redist || freezing)) {   // (the sum of FE.cpp:4631 is checked where the mechanical bins are kept apart: elsewhere the reference has none to read)
            double q[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) q[k] = (k < n) ? a.mech[(size_t)k * N + e] : 0.;
            if (limit) {
                double ctot_mech = 0;
#pragma unroll
                for (int m = 0; m < NB; ++m) if (m < n) ctot_mech += q[m];
                if ((ctot_mech > old_conc) && young && (cy > 0.)) {
                    br2 |= NXS_SLAB_FSD_BR_LIMIT_MECH_RESCALED;
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m < n) q[m] += (-old_conc) * q[m] / ctot_mech;
                }
            }
            if (redist) {
                double ctot_mech = q[0];
#pragma unroll
                for (int j = 1; j < NB; ++j) if (j < n) ctot_mech += q[j];
                if (del_c_fsd >= 0) {
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m == n - 1) q[m] += del_c_fsd;
                } else {
#pragma unroll
                    for (int m = 0; m < NB; ++m) if (m < n) q[m] += del_c_fsd * q[m] / ctot_mech;
                }
            }
            if (redist && c->debug) {
                double ctot = conc;
                if (young) ctot += cy;
                double ctot3 = q[0];
#pragma unroll
                for (int j = 1; j < NB; ++j) if (j < n) ctot3 += q[j];
                if (fabs(ctot - ctot3) > 1e-7) crash = true;
            }
            if (freezing) {   // 9.b: M_time_relaxation_damage is section 9's, just written
                br2 |= NXS_SLAB_FSD_BR_HEALED;
                const double fsd_mech_healing_weight = STD_MIN(1., ddt / a.theal[e]);
#pragma unroll
                for (int m = 0; m < NB; ++m) q[m] = q[m] * (1. - fsd_mech_healing_weight) + fsd_mech_healing_weight * b[m];
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k < n) a.mech[(size_t)k * N + e] = q[k];
        }
        x.br2[e] = br2;
    }
    fsd_raise(a.flags + FSD_FLAG_WELD_CRASH, weld_crash);
    fsd_raise(x.crash, crash);
}
