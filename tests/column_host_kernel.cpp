// The body of k_column (nextsim_amd/csrc/nxs_column_kernels.inl) compiled for the HOST: the kernel's own source with the HIP qualifiers defined away, one call per
// element, the host's libm.  tests/test_column_host_kernel.py builds it (g++ -O2 -fno-builtin -ffp-contract=off) and requires the bits of tests/column_ref.py: the
// transcription of the two column models is then checked without a device.
//   usage: column_host_kernel IN OUT
//   IN : int32[12] Ne, Nn, young, thermo_type, qio_type, freezingpoint_type, ocean_type, snowfall_source, mld_source, flooding, dt, 0; double[8] freezingpoint_mu,
//        snow_cond, Csens_io, constant_mld, nudge_timeT, nudge_timeS, Qdw_const, Fdw_const; int32[3 Ne] 0-based triangles; double[2 Nn] VT; double[2 Nn] ocean;
//        26 rows double[Ne]: tair precip snow ocean_temp ocean_salt mld  Qia dQiadT I subl  Qia_young dQiadT_young I_young subl_young  conc thick snow_thick conc_young
//        h_young hs_young tice0 tice1 tice2 tsurf_young sst sss
//   OUT: double[22][Ne] the rows in NXS_COL_* order, then tice0 tice1 tice2 tsurf_young h_young hs_young
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
#define STD_MAX(a, b) (((a) < (b)) ? (b) : (a))
#define STD_MIN(a, b) (((b) < (a)) ? (b) : (a))
static constexpr int BLOCK = 256;
static struct { int x; } blockIdx, threadIdx;
enum { FLUX_QIA = 7, FLUX_I = 12, FLUX_SUBL = 13, FLUX_DQIADT = 14, FLUX_YOUNG = 16, FLUX_ROWS = 25 };   // nxs_flux_kernels.inl
#include "nxs_dyn.h"
static_assert((int)FLUX_QIA == (int)NXS_FLUX_QIA && (int)FLUX_I == (int)NXS_FLUX_I && (int)FLUX_SUBL == (int)NXS_FLUX_SUBL && (int)FLUX_DQIADT == (int)NXS_FLUX_DQIADT &&
              (int)FLUX_YOUNG == (int)NXS_FLUX_QIA_YOUNG && FLUX_ROWS == NXS_FLUX_ROWS, "the rows of nxs_dyn_fluxes_get");
#include "nxs_column_kernels.inl"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[12];
    double cfg[8];
    if (fread(hdr, 4, 12, f) != 12 || fread(cfg, 8, 8, f) != 8) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    if (fread(t.data(), 4, t.size(), f) != t.size()) return 4;
    std::vector<double> VT(2 * (size_t)Nn), ocean(2 * (size_t)Nn);
    if (fread(VT.data(), 8, VT.size(), f) != VT.size() || fread(ocean.data(), 8, ocean.size(), f) != ocean.size()) return 4;
    std::vector<std::vector<double>> r(26, std::vector<double>(Ne));
    for (auto &v : r) if (fread(v.data(), 8, v.size(), f) != v.size()) return 4;
    fclose(f);
    ColDev c{};
    c.young_cat = hdr[2]; c.thermo_type = hdr[3]; c.qio_type = hdr[4]; c.freezingpoint_type = hdr[5]; c.ocean_type = hdr[6]; c.snowfall_source = hdr[7]; c.mld_source = hdr[8];
    c.flooding = hdr[9]; c.dt = double(hdr[10]);
    c.mu = cfg[0]; c.ks = cfg[1]; c.Csens_io = cfg[2]; c.constant_mld = cfg[3]; c.timeT = cfg[4]; c.timeS = cfg[5]; c.Qdw_const = cfg[6]; c.Fdw_const = cfg[7];
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> flux((size_t)FLUX_ROWS * Ne, 0.), out((size_t)COL_ROWS * Ne);
    const int where[8] = {FLUX_QIA, FLUX_DQIADT, FLUX_I, FLUX_SUBL, FLUX_YOUNG + 0, FLUX_YOUNG + 7, FLUX_YOUNG + 5, FLUX_YOUNG + 6};
    for (int k = 0; k < 8; ++k) for (int e = 0; e < Ne; ++e) flux[(size_t)where[k] * Ne + e] = r[6 + k][e];
    const ColArrays a{Ne, Nn, t0.data(), t1.data(), t2.data(), VT.data(), ocean.data(), r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(),
                      flux.data(), r[14].data(), r[15].data(), r[16].data(), r[17].data(), r[18].data(), r[19].data(), r[20].data(), r[21].data(), r[22].data(),
                      r[23].data(), r[24].data(), r[25].data(), out.data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_column(a, c); }
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    for (int k : {20, 21, 22, 23, 18, 19}) fwrite(r[k].data(), 8, Ne, g);
    fclose(g);
    return 0;
}
