// The device code of a coupled ocean compiled for the HOST: the body of the receive kernel (nxs_remap::receive_values, nextsim_amd/csrc/nxs_remap_core.inl) and
// the three kernels that hold an OceanType::COUPLED statement -- k_fluxes, k_column, k_slab -- from their own sources with the HIP qualifiers defined away, one
// call per element, the host's libm.  tests/test_ocean_coupled_host_kernel.py builds it (g++ -O2 -fno-builtin -ffp-contract=off) and requires the bits of
// tests/ocean_coupled_ref.py; the same program is run once under -fsanitize=address,undefined.
//   usage: ocean_coupled_host_kernel MODE IN OUT
//   receive  IN : int32[4] nels, G, n, n_var; int32[nels + 1] t_off; int32[n] t_pos; int32[n] cell; double[n] w (cell and w in the forward lists' order);
//                 double[n_var][4] a, b, factor, bias; double[n_var][G] the fields
//            OUT: double[n_var][nels] through t_pos, then double[n_var][nels] through copies of cell and w in transposed order
//   fluxes   IN : the input of tests/fluxes_host_kernel.cpp, then double[Ne] qsrml            OUT: as tests/fluxes_host_kernel.cpp
//   column   IN : the input of tests/column_host_kernel.cpp (its ocean_type is not consulted)  OUT: as tests/column_host_kernel.cpp, then sst, sss
//   slab     IN : the input of tests/slab_host_kernel.cpp                                      OUT: as tests/slab_host_kernel.cpp
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#define NXS_HD
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define NXS_RHOA 1.22       // nxs_dyn_kernels.inl
#define NXS_PI 3.141592653589793238462643383279502884197169399375105820974944592308
#define NXS_RHOI 917.
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
#include "nxs_dyn.h"
#include "nxs_remap_core.inl"
#include "nxs_flux_kernels.inl"
#include "nxs_column_kernels.inl"
#include "nxs_slab_kernels.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return fread(p, size, n, f) == n; }

template <int NV>
static void receive_all(int nels, const int *t_off, const int *t_pos, const int *cell, const double *w, const double *const *field, const nxs_remap::ReceiveCoef *co,
                        double *out) {
    for (int t = 0; t < nels; ++t) {
        double v[NV];
        nxs_remap::receive_values<NV>(field, co, t_pos, t_off[t], t_off[t + 1] - t_off[t], cell, w, v);
        for (int i = 0; i < NV; ++i) out[(size_t)i * nels + t] = v[i];
    }
}

static int receive(FILE *f, FILE *g) {
    int hdr[4];
    if (!rd(f, hdr, 4, 4)) return 4;
    const int nels = hdr[0], G = hdr[1], n = hdr[2], nv = hdr[3];
    if (nv < 1 || nv > 5) return 6;
    std::vector<int> t_off((size_t)nels + 1), t_pos(n), cell(n);
    std::vector<double> w(n), co4(4 * (size_t)nv), fld((size_t)nv * G);
    if (!rd(f, t_off.data(), 4, t_off.size()) || !rd(f, t_pos.data(), 4, n) || !rd(f, cell.data(), 4, n) || !rd(f, w.data(), 8, n) || !rd(f, co4.data(), 8, co4.size()) ||
        !rd(f, fld.data(), 8, fld.size()))
        return 4;
    nxs_remap::ReceiveCoef co[5];
    const double *field[5] = {};
    for (int v = 0; v < nv; ++v) { co[v] = nxs_remap::ReceiveCoef{co4[4 * v], co4[4 * v + 1], co4[4 * v + 2], co4[4 * v + 3]}; field[v] = fld.data() + (size_t)v * G; }
    std::vector<int> cell_t(n);
    std::vector<double> w_t(n);
    for (int k = 0; k < n; ++k) { cell_t[k] = cell[t_pos[k]]; w_t[k] = w[t_pos[k]]; }   // k_gridmap_permute
    std::vector<double> out((size_t)nv * nels);
    for (int pass = 0; pass < 2; ++pass) {
        const int *pos = pass ? nullptr : t_pos.data(), *c = pass ? cell_t.data() : cell.data();
        const double *ww = pass ? w_t.data() : w.data();
        switch (nv) {
            case 1: receive_all<1>(nels, t_off.data(), pos, c, ww, field, co, out.data()); break;
            case 2: receive_all<2>(nels, t_off.data(), pos, c, ww, field, co, out.data()); break;
            case 3: receive_all<3>(nels, t_off.data(), pos, c, ww, field, co, out.data()); break;
            case 4: receive_all<4>(nels, t_off.data(), pos, c, ww, field, co, out.data()); break;
            default: receive_all<5>(nels, t_off.data(), pos, c, ww, field, co, out.data()); break;
        }
        fwrite(out.data(), 8, out.size(), g);
    }
    return 0;
}

static int fluxes(FILE *f, FILE *g) {
    int hdr[8];
    double cfg[11];
    if (!rd(f, hdr, 4, 8) || !rd(f, cfg, 8, 11)) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    std::vector<double> wind(2 * (size_t)Nn);
    if (!rd(f, t.data(), 4, t.size()) || !rd(f, wind.data(), 8, wind.size())) return 4;
    std::vector<std::vector<double>> r(19, std::vector<double>(Ne));   // the 18 rows of fluxes_host_kernel.cpp, then qsrml
    for (auto &v : r) if (!rd(f, v.data(), 8, v.size())) return 4;
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
                       r[14].data(), r[15].data(), r[16].data(), r[17].data(), out.data(), tau.data(), r[18].data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_fluxes(a, d); }
    for (int e = 0; e < Ne; ++e) out[(size_t)FLUX_TAU_OW * Ne + e] = tau[e];
    fwrite(out.data(), 8, out.size(), g);
    for (int k = 14; k < 18; ++k) fwrite(r[k].data(), 8, Ne, g);
    return 0;
}

static int column(FILE *f, FILE *g) {
    int hdr[12];
    double cfg[8];
    if (!rd(f, hdr, 4, 12) || !rd(f, cfg, 8, 8)) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    std::vector<double> VT(2 * (size_t)Nn), ocean(2 * (size_t)Nn);
    if (!rd(f, t.data(), 4, t.size()) || !rd(f, VT.data(), 8, VT.size()) || !rd(f, ocean.data(), 8, ocean.size())) return 4;
    std::vector<std::vector<double>> r(26, std::vector<double>(Ne));
    for (auto &v : r) if (!rd(f, v.data(), 8, v.size())) return 4;
    ColDev c{};
    c.young_cat = hdr[2]; c.thermo_type = hdr[3]; c.qio_type = hdr[4]; c.freezingpoint_type = hdr[5]; c.ocean_type = NXS_COL_OCEAN_COUPLED; c.snowfall_source = hdr[7];
    c.mld_source = hdr[8]; c.flooding = hdr[9]; c.dt = double(hdr[10]);
    c.mu = cfg[0]; c.ks = cfg[1]; c.Csens_io = cfg[2]; c.constant_mld = cfg[3]; c.timeT = cfg[4]; c.timeS = cfg[5]; c.Qdw_const = cfg[6]; c.Fdw_const = cfg[7];
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> flux((size_t)FLUX_ROWS * Ne, 0.), out((size_t)COL_ROWS * Ne);
    const int where[8] = {FLUX_QIA, FLUX_DQIADT, FLUX_I, FLUX_SUBL, FLUX_YOUNG + 0, FLUX_YOUNG + 7, FLUX_YOUNG + 5, FLUX_YOUNG + 6};
    for (int k = 0; k < 8; ++k) for (int e = 0; e < Ne; ++e) flux[(size_t)where[k] * Ne + e] = r[6 + k][e];
    const ColArrays a{Ne, Nn, t0.data(), t1.data(), t2.data(), VT.data(), ocean.data(), r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(),
                      flux.data(), r[14].data(), r[15].data(), r[16].data(), r[17].data(), r[18].data(), r[19].data(), r[20].data(), r[21].data(), r[22].data(),
                      r[23].data(), r[24].data(), r[25].data(), out.data(), r[24].data(), r[25].data()};
    for (int e = 0; e < Ne; ++e) { blockIdx.x = e / BLOCK; threadIdx.x = e % BLOCK; k_column(a, c); }
    fwrite(out.data(), 8, out.size(), g);
    for (int k : {20, 21, 22, 23, 18, 19, 24, 25}) fwrite(r[k].data(), 8, Ne, g);
    return 0;
}

static int slab(FILE *f, FILE *g) {
    int hdr[20];
    double cfg[15];
    if (!rd(f, hdr, 4, 20) || !rd(f, cfg, 8, 15)) return 4;
    const int Ne = hdr[0], Nn = hdr[1];
    std::vector<int> t(3 * (size_t)Ne);
    std::vector<double> wind(2 * (size_t)Nn), flux((size_t)FLUX_ROWS * Ne), col((size_t)COL_ROWS * Ne);
    if (!rd(f, t.data(), 4, t.size()) || !rd(f, wind.data(), 8, wind.size()) || !rd(f, flux.data(), 8, flux.size()) || !rd(f, col.data(), 8, col.size())) return 4;
    std::vector<std::vector<double>> r(29, std::vector<double>(Ne));
    for (auto &v : r) if (!rd(f, v.data(), 8, v.size())) return 4;
    SlabDev c{};
    c.dt = double(hdr[6]); c.newice_type = hdr[7]; c.melt_type = hdr[8]; c.freezingpoint_type = hdr[4];
    c.flags = (hdr[2] ? SF_YOUNG_CAT : 0) | (hdr[3] ? SF_WINTON : 0) | (hdr[5] == NXS_COL_MLD_ROW ? SF_MLD_ROW : 0) | (hdr[9] ? SF_ASSIM : 0) | (hdr[10] ? SF_HEALING : 0) |
              (hdr[11] ? SF_PONDS : 0) | (hdr[12] ? SF_RESET_BY_DATE : 0) | (hdr[13] && hdr[12] ? SF_YOUNG_IN_MYI_RESET : 0) | (hdr[14] ? SF_EQUAL_MELTING : 0) |
              (hdr[15] ? SF_FIRST_STEP : 0) | (hdr[16] ? SF_LAST_STEP : 0) | (hdr[17] ? SF_FYI_RESET : 0) | (hdr[18] ? SF_MYI_RESET : 0) | (hdr[19] ? SF_ONSET_RESET : 0) |
              SF_OCEAN_COUPLED;
    c.rh0 = 1. / cfg[0]; c.rPhiF = 1. / cfg[1]; c.PhiF = cfg[1]; c.PhiM = cfg[2]; c.h_young_min = cfg[3]; c.h_young_max_sharp = .5 * (cfg[3] + cfg[4]);
    c.assim_flux_exponent = cfg[5]; c.freeze_days_threshold = cfg[6]; c.meltponds_roff = cfg[7]; c.meltponds_dep2frac = cfg[8]; c.time_relaxation_damage = cfg[9];
    c.deltaT_relaxation_damage = cfg[10]; c.mu = cfg[11]; c.ks = cfg[12]; c.constant_mld = cfg[13]; c.ocean_albedo = cfg[14];
    std::vector<int> t0(Ne), t1(Ne), t2(Ne);
    for (int e = 0; e < Ne; ++e) { t0[e] = t[3 * e]; t1[e] = t[3 * e + 1]; t2[e] = t[3 * e + 2]; }
    std::vector<double> out((size_t)SLAB_ROWS * Ne);
    std::vector<unsigned> br(Ne);
    auto R = [&](int k) { return r[k].data(); };
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
    fwrite(out.data(), 8, out.size(), g);
    for (int k = 3; k < 29; ++k) fwrite(r[k].data(), 8, Ne, g);
    std::vector<double> w(br.begin(), br.end());
    fwrite(w.data(), 8, w.size(), g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 3;
    FILE *g = fopen(argv[3], "wb");
    if (!g) { fclose(f); return 5; }
    int rc = 2;
    if (!strcmp(argv[1], "receive")) rc = receive(f, g);
    else if (!strcmp(argv[1], "fluxes")) rc = fluxes(f, g);
    else if (!strcmp(argv[1], "column")) rc = column(f, g);
    else if (!strcmp(argv[1], "slab")) rc = slab(f, g);
    fclose(f);
    fclose(g);
    return rc;
}
