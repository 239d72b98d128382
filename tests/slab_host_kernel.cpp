// The body of k_slab (nextsim_amd/csrc/nxs_slab_kernels.inl) compiled for the HOST: the kernel's own source with the HIP qualifiers defined away, one call per
// element, the host's libm.  tests/test_slab_host_kernel.py builds it (g++ -O2 -fno-builtin -ffp-contract=off) and requires the bits of tests/slab_ref.py: the
// transcription of FE.cpp:5413-6133 is then checked without a device.
//   usage: slab_host_kernel IN OUT
//   IN : int32[20] Ne, Nn, young, winton, freezingpoint_type, mld_source, dt, newice_type, melt_type, use_assim_flux, temp_dep_healing, use_meltponds,
//        reset_by_date, include_young_ice, equal_melting, then the five flags of nxs_dyn_slab_clock; double[15] hnull, PhiF, PhiM, h_young_min, h_young_max,
//        assim_flux_exponent, reset_freeze_days, meltpond_runoff_fraction, meltpond_depth_to_fraction, time_relaxation_damage, deltaT_relaxation_damage,
//        freezingpoint_mu, snow_cond, constant_mld, ocean_albedo; int32[3 Ne] 0-based triangles; double[2 Nn] wind; double[25][Ne] the flux rows; double[22][Ne]
//        the column rows; then 29 rows double[Ne]: precip mld conc_upd  conc thick snow_thick ridge_ratio conc_young h_young hs_young conc_myi thick_myi
//        time_relaxation_damage  sst sss pond_fraction lid_volume  tice0 tice1 tice2  pond_volume del_vi_tend freeze_days freeze_onset conc_summer thick_summer
//        fyi_fraction age_det age
//   OUT: double[29][Ne] the rows in NXS_SLAB_* order, then the 26 rows from conc on (everything written in place), then the branch words as double[Ne]
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
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
enum { FLUX_QOW = 0, FLUX_QLW_OW, FLUX_QSW_OW, FLUX_QLH_OW, FLUX_QSH_OW, FLUX_EVAP, FLUX_TAU_OW, FLUX_QIA, FLUX_QLWI, FLUX_QSWI, FLUX_QLHI, FLUX_QSHI, FLUX_I, FLUX_SUBL,
       FLUX_DQIADT, FLUX_ALBEDO, FLUX_YOUNG = 16, FLUX_ROWS = 25 };   // nxs_flux_kernels.inl
#include "nxs_dyn.h"
static_assert((int)FLUX_QOW == (int)NXS_FLUX_QOW && (int)FLUX_EVAP == (int)NXS_FLUX_EVAP && (int)FLUX_QIA == (int)NXS_FLUX_QIA && (int)FLUX_QSHI == (int)NXS_FLUX_QSHI &&
              (int)FLUX_ALBEDO == (int)NXS_FLUX_ALBEDO && (int)FLUX_YOUNG == (int)NXS_FLUX_QIA_YOUNG && FLUX_ROWS == NXS_FLUX_ROWS, "the rows of nxs_dyn_fluxes_get");
#include "nxs_column_kernels.inl"
#include "nxs_slab_kernels.inl"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
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
    SlabDev c{};
    c.dt = double(hdr[6]); c.newice_type = hdr[7]; c.melt_type = hdr[8]; c.freezingpoint_type = hdr[4];
    c.flags = (hdr[2] ? SF_YOUNG_CAT : 0) | (hdr[3] ? SF_WINTON : 0) | (hdr[5] == NXS_COL_MLD_ROW ? SF_MLD_ROW : 0) | (hdr[9] ? SF_ASSIM : 0) | (hdr[10] ? SF_HEALING : 0) |
              (hdr[11] ? SF_PONDS : 0) | (hdr[12] ? SF_RESET_BY_DATE : 0) | (hdr[13] && hdr[12] ? SF_YOUNG_IN_MYI_RESET : 0) | (hdr[14] ? SF_EQUAL_MELTING : 0) |
              (hdr[15] ? SF_FIRST_STEP : 0) | (hdr[16] ? SF_LAST_STEP : 0) | (hdr[17] ? SF_FYI_RESET : 0) | (hdr[18] ? SF_MYI_RESET : 0) | (hdr[19] ? SF_ONSET_RESET : 0);
    c.rh0 = 1. / cfg[0]; c.rPhiF = 1. / cfg[1]; c.PhiF = cfg[1]; c.PhiM = cfg[2]; c.h_young_min = cfg[3]; c.h_young_max_sharp = .5 * (cfg[3] + cfg[4]);
    c.assim_flux_exponent = cfg[5]; c.freeze_days_threshold = cfg[6]; c.meltponds_roff = cfg[7]; c.meltponds_dep2frac = cfg[8]; c.time_relaxation_damage = cfg[9];
    c.deltaT_relaxation_damage = cfg[10]; c.mu = cfg[11]; c.ks = cfg[12]; c.constant_mld = cfg[13]; c.ocean_albedo = cfg[14];
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> out((size_t)SLAB_ROWS * Ne);
    std::vector<unsigned> br(Ne);
    auto R = [&](int k) { return r[k].data(); };
    // nxs_dyn_slab_state is one block [10][Ne] in the library: conc_upd (row 2 of the input), then the nine rows from pond_volume on (rows 20 .. 28)
    std::vector<double> st((size_t)SLAB_ST_ROWS * Ne);
    for (int e = 0; e < Ne; ++e) {
        st[e] = r[2][e];
        for (int k = 1; k < SLAB_ST_ROWS; ++k) st[(size_t)k * Ne + e] = r[19 + k][e];
    }
    const SlabArrays a{Ne, Nn, t0.data(), t1.data(), t2.data(), wind.data(), flux.data(), col.data(), R(0), R(1),
                       R(3), R(4), R(5), R(6), R(7), R(8), R(9), R(10), R(11), R(12), R(13), R(14), R(15), R(16), R(17), R(18), R(19), st.data(), out.data(), br.data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_slab(a, c); }
    for (int e = 0; e < Ne; ++e)
        for (int k = 1; k < SLAB_ST_ROWS; ++k) r[19 + k][e] = st[(size_t)k * Ne + e];
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    for (int k = 3; k < 29; ++k) fwrite(r[k].data(), 8, Ne, g);
    std::vector<double> w(br.begin(), br.end());
    fwrite(w.data(), 8, w.size(), g);
    fclose(g);
    return 0;
}
