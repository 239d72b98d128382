// The body of k_fluxes (nextsim_amd/csrc/nxs_flux_kernels.inl) compiled for the HOST: the kernel's own source with the HIP qualifiers defined away, one call per
// element, the host's libm.  tests/test_fluxes_host_kernel.py builds it (g++ -O2 -fno-builtin -ffp-contract=off: no libm call folded at compile time, no
// contraction) and requires the bits of tests/fluxes_ref.py: the transcription of the formulas is then checked without a device, and what is left for the device
// comparison (tests/test_gpu_fluxes.py) is the device's libm.
//   usage: fluxes_host_kernel IN OUT
//   IN : int32[8] Ne, Nn, young, alb_scheme, humidity_source, longwave_source, force_neutral_atmosphere, 0; double[11] alb_ice, alb_sn, alb_ponds, I_0, ocean_albedo,
//        drag_ocean_t, drag_ocean_q, zref_wind, zref_temp, limiting_lengthscale, quad_drag_coef_air; int32[3 Ne] 0-based triangles; double[2 Nn] wind; 18 rows
//        double[Ne]: tair mslp Qsw_in humidity longwave conc snow_thick conc_young hs_young tice0 tsurf_young sst pond_fraction lid_volume drag_ui drag_ti
//        drag_ui_young drag_ti_young
//   OUT: double[25][Ne] the rows in NXS_FLUX_* order, then the four updated drags
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define NXS_RHOA 1.22       // nxs_dyn_kernels.inl
#define NXS_LF 333.55e3
#define NXS_PI 3.141592653589793238462643383279502884197169399375105820974944592308
#define STD_MAX(a, b) (((a) < (b)) ? (b) : (a))
#define STD_MIN(a, b) (((b) < (a)) ? (b) : (a))
static constexpr int BLOCK = 256;
static struct { int x; } blockIdx, threadIdx;
#include "nxs_dyn.h"
#include "nxs_flux_kernels.inl"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[8];
    double cfg[11];
    if (fread(hdr, 4, 8, f) != 8 || fread(cfg, 8, 11, f) != 11) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    if (fread(t.data(), 4, t.size(), f) != t.size()) return 4;
    std::vector<double> wind(2 * (size_t)Nn);
    if (fread(wind.data(), 8, wind.size(), f) != wind.size()) return 4;
    std::vector<std::vector<double>> r(18, std::vector<double>(Ne));
    for (auto &v : r) if (fread(v.data(), 8, v.size(), f) != v.size()) return 4;
    fclose(f);
    nxs_dyn_flux_config c{};
    c.alb_scheme = hdr[3]; c.humidity_source = hdr[4]; c.longwave_source = hdr[5]; c.force_neutral_atmosphere = hdr[6];
    c.alb_ice = cfg[0]; c.alb_sn = cfg[1]; c.alb_ponds = cfg[2]; c.I_0 = cfg[3]; c.ocean_albedo = cfg[4]; c.drag_ocean_t = cfg[5]; c.drag_ocean_q = cfg[6];
    c.zref_wind = cfg[7]; c.zref_temp = cfg[8]; c.limiting_lengthscale = cfg[9];
    const FluxDev d = flux_derive(c, cfg[10]);
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> out((size_t)FLUX_ROWS * Ne), tau(Ne);
    const FluxArrays a{Ne, Nn, hdr[2], t0.data(), t1.data(), t2.data(), wind.data(), r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(),
                       r[5].data(), r[6].data(), r[7].data(), r[8].data(), r[9].data(), r[10].data(), r[11].data(), r[12].data(), r[13].data(),
                       r[14].data(), r[15].data(), r[16].data(), r[17].data(), out.data(), tau.data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_fluxes(a, d); }
    for (int e = 0; e < Ne; ++e) out[(size_t)FLUX_TAU_OW * Ne + e] = tau[e];
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    for (int k = 14; k < 18; ++k) fwrite(r[k].data(), 8, Ne, g);
    fclose(g);
    return 0;
}
