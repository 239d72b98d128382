// The bodies of k_nesting_ice, k_nesting_dynamics, k_diffuse_pack and k_diffuse (nextsim_amd/csrc/nxs_nesting_kernels.inl) compiled for the HOST: the kernels' own
// source with the HIP qualifiers defined away, one call per thread of the launch grid.  tests/test_nesting_host_kernel.py builds it (g++ -O2 -ffp-contract=off) and
// requires the bits of tests/nesting_ref.py: the transcription is then checked without a device.  Every row is an allocation of its own, as on the device.
//   usage: nesting_host_kernel IN OUT
//   IN (nudge)  : int32[8] 0, Ne, Nn, nudge_function, young, rec, dmg_rec, which (0: k_nesting_ice, 1: k_nesting_dynamics); double[3] nudge_scale, q, qvt;
//                 5 x { int32[2] mode, 0; double[4] fcoeff0, fcoeff1, factor, bias }; double[12][Ne] + double[3][Nn] snapshot 0; the same of snapshot 1;
//                 double[11][Ne] conc, thick, snow_thick, conc_young, h_young, hs_young, sigma0, sigma1, sigma2, damage, ridge_ratio; double[2 Nn] VT
//   OUT         : double[11][Ne], double[2 Nn] the same after the launch; double[Ne] the records' fourth slot (rec; -777 went in where it is not the damage)
//   IN (diffuse): int32[8] 1, Ne, on_sst, on_sss, 0, 0, 0, 0; double[2] factor_sst, factor_sss; int32[3 Ne] the table; double[Ne] sst; double[Ne] sss
//   OUT         : double[Ne] sst, double[Ne] sss
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
static constexpr int BLOCK = 256;
static struct { int x, y; } blockIdx, threadIdx;
#include "nxs_dyn.h"
#include "nxs_nesting_kernels.inl"

typedef std::vector<double> Row;
static bool rd(FILE *f, void *p, size_t size, size_t n) { return fread(p, size, n, f) == n; }
static bool rd(FILE *f, Row &r, size_t n) { r.resize(n); return rd(f, r.data(), 8, n); }
static int nblocks(int n) { return n > 0 ? (n + BLOCK - 1) / BLOCK : 1; }
template <class K, class... A> static void launch(int blocks, K kernel, A... args) {
    for (int bx = 0; bx < blocks; ++bx)
        for (int tx = 0; tx < BLOCK; ++tx) { blockIdx.x = bx; blockIdx.y = 0; threadIdx.x = tx; kernel(args...); }
}

static int nudge(FILE *f, const int *hdr, const char *out_path) {
    const int Ne = hdr[1], Nn = hdr[2], fn = hdr[3], young = hdr[4], rec = hdr[5], dmg_rec = hdr[6], which = hdr[7];
    double par[3];
    if (!rd(f, par, 8, 3)) return 4;
    NestTime t[NEST_DATASETS];
    for (int k = 0; k < NEST_DATASETS; ++k) {
        int m[2];
        double c[4];
        if (!rd(f, m, 4, 2) || !rd(f, c, 8, 4)) return 4;
        t[k] = NestTime{c[0], c[1], c[2], c[3], m[0]};
    }
    Row el[2][NEST_EL_ROWS], nd[2][NEST_ND_ROWS], st[11], VT;
    for (int s = 0; s < 2; ++s) {
        for (auto &r : el[s]) if (!rd(f, r, Ne)) return 4;
        for (auto &r : nd[s]) if (!rd(f, r, Nn)) return 4;
    }
    for (auto &r : st) if (!rd(f, r, Ne)) return 4;
    if (!rd(f, VT, 2 * (size_t)Nn)) return 4;
    auto row = [&](int ds, bool nodal, int k) { return NestRow{(nodal ? nd[0][k] : el[0][k]).data(), t[ds].mode == NXS_TF_LINEAR ? (nodal ? nd[1][k] : el[1][k]).data() : nullptr}; };
    Row S4(4 * (size_t)Ne), slot3(Ne, 0.);
    if (which == 0) {
        NestIce a{};
        a.Ne = Ne; a.nfields = young ? 6 : 3; a.fn = fn; a.scale = par[0]; a.q = par[1];
        a.t_dist = t[NXS_NEST_DS_DISTANCE_ELEMENTS]; a.t_ice = t[NXS_NEST_DS_ICE_ELEMENTS];
        a.dist = row(NXS_NEST_DS_DISTANCE_ELEMENTS, false, NXS_NEST_DIST);
        const int src[6] = {NXS_NEST_CONC, NXS_NEST_THICK, NXS_NEST_SNOW_THICK, NXS_NEST_CONC_YOUNG, NXS_NEST_H_YOUNG, NXS_NEST_HS_YOUNG};
        for (int k = 0; k < a.nfields; ++k) { a.snap[k] = row(NXS_NEST_DS_ICE_ELEMENTS, false, src[k]); a.x[k] = st[k].data(); }
        launch(nblocks((Ne + 1) / 2), k_nesting_ice, a);
    } else {
        NestDyn a{};
        a.Ne = Ne; a.Nn = Nn; a.fn = fn; a.rec = rec; a.dmg_rec = dmg_rec; a.scale = par[0]; a.q = par[1]; a.qvt = par[2];
        a.t_dist = t[NXS_NEST_DS_DISTANCE_ELEMENTS]; a.t_dyn = t[NXS_NEST_DS_DYNAMICS_ELEMENTS]; a.t_dist_n = t[NXS_NEST_DS_DISTANCE_NODES]; a.t_nodes = t[NXS_NEST_DS_NODES];
        a.dist = row(NXS_NEST_DS_DISTANCE_ELEMENTS, false, NXS_NEST_DIST);
        for (int k = 0; k < 3; ++k) a.sig[k] = row(NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_SIGMA1 + k);
        a.dmg = row(NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_DAMAGE);
        a.ridge = row(NXS_NEST_DS_DYNAMICS_ELEMENTS, false, NXS_NEST_RIDGE_RATIO);
        a.dist_n = row(NXS_NEST_DS_DISTANCE_NODES, true, NXS_NEST_DIST_NODES);
        for (int k = 0; k < 2; ++k) a.vt[k] = row(NXS_NEST_DS_NODES, true, NXS_NEST_VT1 + k);
        Row stale(Ne, -999.);   // records home: the arrays of sigma (and of the damage, BBM) are NOT current and must not be touched
        if (rec) {
            for (int e = 0; e < Ne; ++e) { for (int k = 0; k < 3; ++k) S4[4 * (size_t)e + k] = st[6 + k][e]; S4[4 * (size_t)e + 3] = dmg_rec ? st[9][e] : -777.; }
            a.S4 = S4.data();
            for (int k = 0; k < 3; ++k) a.s[k] = stale.data();
            a.damage = dmg_rec ? stale.data() : st[9].data();
        } else {
            for (int k = 0; k < 3; ++k) a.s[k] = st[6 + k].data();
            a.damage = st[9].data();
        }
        a.ridge_x = st[10].data(); a.VT = VT.data();
        launch(nblocks(((Ne > Nn ? Ne : Nn) + 1) / 2), k_nesting_dynamics, a);
        if (rec) {
            for (int e = 0; e < Ne; ++e) {
                for (int k = 0; k < 3; ++k) st[6 + k][e] = S4[4 * (size_t)e + k];
                if (dmg_rec) st[9][e] = S4[4 * (size_t)e + 3];
                slot3[e] = S4[4 * (size_t)e + 3];
                if (stale[e] != -999.) return 8;
            }
        }
    }
    FILE *g = fopen(out_path, "wb");
    if (!g) return 5;
    for (auto &r : st) fwrite(r.data(), 8, r.size(), g);
    fwrite(VT.data(), 8, VT.size(), g);
    fwrite(slot3.data(), 8, slot3.size(), g);
    fclose(g);
    return 0;
}

static int diffuse(FILE *f, const int *hdr, const char *out_path) {
    const int Ne = hdr[1], on_sst = hdr[2], on_sss = hdr[3];
    double factor[2];
    std::vector<int32_t> ec(3 * (size_t)Ne);
    Row sst, sss;
    if (!rd(f, factor, 8, 2) || !rd(f, ec.data(), 4, ec.size()) || !rd(f, sst, Ne) || !rd(f, sss, Ne)) return 4;
    for (int v : ec) if (v < -1 || v >= Ne) return 6;
    std::vector<NestPair> old(Ne);
    static_assert(sizeof(DiffTri) == 12, "three ints");
    launch(nblocks(Ne), k_diffuse_pack, Ne, (const double *)sst.data(), (const double *)sss.data(), old.data());
    launch(nblocks(Ne), k_diffuse, Ne, reinterpret_cast<const DiffTri *>(ec.data()), (const NestPair *)old.data(), factor[0], factor[1], on_sst, on_sss, sst.data(), sss.data());
    FILE *g = fopen(out_path, "wb");
    if (!g) return 5;
    fwrite(sst.data(), 8, Ne, g);
    fwrite(sss.data(), 8, Ne, g);
    fclose(g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[8] = {0};
    if (!rd(f, hdr, 4, 8)) return 4;
    const int rc = hdr[0] == 0 ? nudge(f, hdr, argv[2]) : diffuse(f, hdr, argv[2]);
    fclose(f);
    return rc;
}
