// The two kernels of nxs_dyn_slab_coupled (nextsim_amd/csrc/nxs_slab_fsd_kernels.inl; slab_element<true> of nxs_slab_kernels.inl, the welding of
// nxs_fsd_weld_body.inl) compiled for the HOST: the kernels' own source with the HIP qualifiers defined away, one call per element, the host's libm.
// tests/test_slab_fsd_ref.py builds it (g++ -O2 -fno-builtin -ffp-contract=off) and requires the bits of tests/slab_fsd_ref.py.
//   usage: slab_fsd_host_kernel IN FSD OUT
//   IN : exactly the input of tests/slab_host_kernel.cpp (its melt_type is the slab's own)
//   FSD: int32[8] melt_type of the coupled call, nb, distinguish_mech_fsd, welding_type, debug_fsd, mech attached, 0, 0; double[1] welding_kappa; double[5][nb]
//        bin_widths, bin_centres, area_scaled_up, area_scaled_centered, area_scaled_binwidth; int32[nb][nb] alpha_merge; double[nb][Ne] conc_fsd; then, if attached,
//        double[nb][Ne] conc_mech_fsd
//   OUT: the output of slab_host_kernel, then double[nb][Ne] conc_fsd, double[nb][Ne] conc_mech_fsd (if attached), the NXS_SLAB_FSD_BR_* words as double[Ne],
//        double[2] thermo_fsd_crash, weld_crash
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
#define NXS_RHOI 917.       // nxs_dyn_kernels.inl
#define NXS_RHOW 1025.
#define NXS_RHOS 330.
#define NXS_SI 5.
#define NXS_LF 333.55e3
#define NXS_HEAT_C 2100.
#define NXS_DAYS_IN_SEC 86400.
#define STD_MAX(a, b) (((a) < (b)) ? (b) : (a))
#define STD_MIN(a, b) (((b) < (a)) ? (b) : (a))
static constexpr int BLOCK = 256;
static struct { int x; } blockIdx, threadIdx;
#define __ballot(m) ((m) ? 1ull << (threadIdx.x & 63) : 0ull)   // a wave of one lane
#define __ffsll(b) __builtin_ffsll(b)
enum { FLUX_QOW = 0, FLUX_QLW_OW, FLUX_QSW_OW, FLUX_QLH_OW, FLUX_QSH_OW, FLUX_EVAP, FLUX_TAU_OW, FLUX_QIA, FLUX_QLWI, FLUX_QSWI, FLUX_QLHI, FLUX_QSHI, FLUX_I, FLUX_SUBL,
       FLUX_DQIADT, FLUX_ALBEDO, FLUX_YOUNG = 16, FLUX_ROWS = 25 };   // nxs_flux_kernels.inl
#include "nxs_dyn.h"
static_assert((int)FLUX_QOW == (int)NXS_FLUX_QOW && (int)FLUX_EVAP == (int)NXS_FLUX_EVAP && (int)FLUX_QIA == (int)NXS_FLUX_QIA && (int)FLUX_QSHI == (int)NXS_FLUX_QSHI &&
              (int)FLUX_ALBEDO == (int)NXS_FLUX_ALBEDO && (int)FLUX_YOUNG == (int)NXS_FLUX_QIA_YOUNG && FLUX_ROWS == NXS_FLUX_ROWS, "the rows of nxs_dyn_fluxes_get");
#include "nxs_fsd_kernels.inl"
#include "nxs_column_kernels.inl"
#include "nxs_slab_kernels.inl"
#include "nxs_slab_fsd_kernels.inl"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[20];
    double cfg[15];
    if (fread(hdr, 4, 20, f) != 20 || fread(cfg, 8, 15, f) != 15) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    if (fread(t.data(), 4, t.size(), f) != t.size()) return 4;
    std::vector<double> wind(2 * (size_t)Nn), flux((size_t)FLUX_ROWS * Ne), col((size_t)COL_ROWS * Ne);
    if (fread(wind.data(), 8, wind.size(), f) != wind.size() || fread(flux.data(), 8, flux.size(), f) != flux.size() || fread(col.data(), 8, col.size(), f) != col.size()) return 4;
    std::vector<std::vector<double>> r(29, std::vector<double>(Ne));
    for (auto &v : r) if (fread(v.data(), 8, v.size(), f) != v.size()) return 4;
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) return 3;
    int fh[8];
    double kappa;
    if (fread(fh, 4, 8, f) != 8 || fread(&kappa, 8, 1, f) != 1) return 6;
    const int nb = fh[1];
    if (nb < 1 || nb > NXS_FSD_MAX_BINS) return 6;
    static FsdDev d{};
    d.n = nb; d.distinguish = fh[2]; d.welding_type = fh[3]; d.debug = fh[4]; d.kappa = kappa;
    if (fread(d.widths, 8, nb, f) != (size_t)nb || fread(d.centres, 8, nb, f) != (size_t)nb || fread(d.asu, 8, nb, f) != (size_t)nb || fread(d.asc, 8, nb, f) != (size_t)nb ||
        fread(d.asb, 8, nb, f) != (size_t)nb) return 6;
    for (int j = 0; j < nb; ++j) if (fread(d.alpha[j], 4, nb, f) != (size_t)nb) return 6;
    std::vector<double> fsd((size_t)nb * Ne), mech(fh[5] ? (size_t)nb * Ne : 0);
    if (fread(fsd.data(), 8, fsd.size(), f) != fsd.size() || fread(mech.data(), 8, mech.size(), f) != mech.size()) return 6;
    fclose(f);
    SlabDev c{};
    c.dt = double(hdr[6]); c.newice_type = hdr[7]; c.melt_type = fh[0]; c.freezingpoint_type = hdr[4];
    c.flags = (hdr[2] ? SF_YOUNG_CAT : 0) | (hdr[3] ? SF_WINTON : 0) | (hdr[5] == NXS_COL_MLD_ROW ? SF_MLD_ROW : 0) | (hdr[9] ? SF_ASSIM : 0) | (hdr[10] ? SF_HEALING : 0) |
              (hdr[11] ? SF_PONDS : 0) | (hdr[12] ? SF_RESET_BY_DATE : 0) | (hdr[13] && hdr[12] ? SF_YOUNG_IN_MYI_RESET : 0) | (hdr[14] ? SF_EQUAL_MELTING : 0) |
              (hdr[15] ? SF_FIRST_STEP : 0) | (hdr[16] ? SF_LAST_STEP : 0) | (hdr[17] ? SF_FYI_RESET : 0) | (hdr[18] ? SF_MYI_RESET : 0) | (hdr[19] ? SF_ONSET_RESET : 0);
    c.rh0 = 1. / cfg[0]; c.rPhiF = 1. / cfg[1]; c.PhiF = cfg[1]; c.PhiM = cfg[2]; c.h_young_min = cfg[3]; c.h_young_max_sharp = .5 * (cfg[3] + cfg[4]);
    c.assim_flux_exponent = cfg[5]; c.freeze_days_threshold = cfg[6]; c.meltponds_roff = cfg[7]; c.meltponds_dep2frac = cfg[8]; c.time_relaxation_damage = cfg[9];
    c.deltaT_relaxation_damage = cfg[10]; c.mu = cfg[11]; c.ks = cfg[12]; c.constant_mld = cfg[13]; c.ocean_albedo = cfg[14];
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> out((size_t)SLAB_ROWS * Ne), scr((size_t)SLAB_SCR_ROWS * Ne);
    std::vector<unsigned> br(Ne), br2(Ne);
    auto R = [&](int k) { return r[k].data(); };
    std::vector<double> st((size_t)SLAB_ST_ROWS * Ne);
    for (int e = 0; e < Ne; ++e) {
        st[e] = r[2][e];
        for (int k = 1; k < SLAB_ST_ROWS; ++k) st[(size_t)k * Ne + e] = r[19 + k][e];
    }
    const SlabArrays a{Ne, Nn, t0.data(), t1.data(), t2.data(), wind.data(), flux.data(), col.data(), R(0), R(1),
                       R(3), R(4), R(5), R(6), R(7), R(8), R(9), R(10), R(11), R(12), R(13), R(14), R(15), R(16), R(17), R(18), R(19), st.data(), out.data(), br.data()};
    const SlabCoupled x{fsd.data(), d.widths, d.centres, nb, scr.data(), br2.data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_coupled_thermo(a, c, x); }
    int flags[FSD_FLAGS] = {0, 0, 0, 0}, crash = 0;
    // rows of nxs_dyn_state as the first launch left them: conc R(3), thick R(4), conc_young R(7), h_young R(8), time_relaxation_damage R(12)
    const FsdArrays fa{Ne, hdr[2], fsd.data(), fh[5] ? mech.data() : nullptr, nullptr, nullptr, R(3), R(7), R(4), R(8), R(12), nullptr, 1, flags};
    const CoupledBins b{c.dt, c.melt_type, scr.data(), col.data() + (size_t)COL_DEL_HI * Ne, br.data(), br2.data(), &crash};
    for (int e = 0; e < Ne; ++e) {
        blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK;
        if (nb <= 2) k_coupled_bins<2>(fa, &d, b);          // FSD_LAUNCH of nxs_fsd.inl
        else if (nb <= 6) k_coupled_bins<6>(fa, &d, b);
        else if (nb <= 12) k_coupled_bins<12>(fa, &d, b);
        else k_coupled_bins<16>(fa, &d, b);
    }
    for (int e = 0; e < Ne; ++e)
        for (int k = 1; k < SLAB_ST_ROWS; ++k) r[19 + k][e] = st[(size_t)k * Ne + e];
    FILE *g = fopen(argv[3], "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    for (int k = 3; k < 29; ++k) fwrite(r[k].data(), 8, Ne, g);
    std::vector<double> w(br.begin(), br.end());
    fwrite(w.data(), 8, w.size(), g);
    fwrite(fsd.data(), 8, fsd.size(), g);
    fwrite(mech.data(), 8, mech.size(), g);
    std::vector<double> w2(br2.begin(), br2.end());
    fwrite(w2.data(), 8, w2.size(), g);
    const double fl[2] = {double(crash), double(flags[FSD_FLAG_WELD_CRASH])};
    fwrite(fl, 8, 2, g);
    fclose(g);
    return 0;
}
