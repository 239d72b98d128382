// Both bodies of nxs_dyn_means_regular_update (nextsim_amd/csrc/nxs_means_regular_body.inl) compiled for the HOST: the kernels' own text with the HIP qualifiers
// defined away.  The search runs as k_means_regular_hits does, one call per element -- sequentially, with max for the atomic maximum --, the gather as
// k_means_regular_gather does, one call per grid point with interp_out staged at [nv][256].  tests/test_means_regular_host_kernel.py builds it
// (g++ -O2 -ffp-contract=off) and requires the bits of the fixture the real contrib/bamg wrote (tests/golden/means_regular.npz) and of tests/means_regular_ref.py.
//   usage: means_regular_host_kernel IN OUT
//   IN : int32[12] ncols, nrows, n_el, n_nod, n_pairs, ice_col, Neo, rotate, Ne, Nn, displaced, order (0: elements ascending, 1: descending -- the maximum
//        must not care); uint32[2] mask_el, mask_nod; int32[12] first; int32[12] second; double[4] miss_val, xmin, ymax, spacing; int32[3 Ne] triangles (0-based,
//        [Ne][3]); double[Nn] x0; double[Nn] y0; displaced: double[2 Nn] UM; rotate: double[G] cos, double[G] sin (entry k from gridLON[k]);
//        double[Ne*n_el] el; double[Nn*n_nod] nod; double[n_el*G] grid_el before; double[n_nod*G] grid_nod before
//   OUT: double[n_el*G] grid_el; double[n_nod*G] grid_nod after; int32[G] the winners
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define __device__
#define __host__
#include "nxs_means_regular_body.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[12], first[12], second[12];
    unsigned mask[2];
    double par[4];
    nxs_mr::Args a{};
    if (!rd(f, hdr, 4, 12) || !rd(f, mask, 4, 2) || !rd(f, first, 4, 12) || !rd(f, second, 4, 12) || !rd(f, par, 8, 4)) return 4;
    const int ncols = hdr[0], nrows = hdr[1], n_el = hdr[2], n_nod = hdr[3], rotate = hdr[7], Ne = hdr[8], Nn = hdr[9], displaced = hdr[10], order = hdr[11];
    if (ncols < 1 || nrows < 1 || n_el < 0 || n_el > nxs_mp::MAX_VARS || n_nod < 0 || n_nod > nxs_mp::MAX_VARS || hdr[4] < 0 || hdr[4] > nxs_mp::MAX_PAIRS || Ne < 0 || Nn < 0) return 6;
    const int G = ncols * nrows;
    a.m.G = G; a.m.n_el = n_el; a.m.n_nod = n_nod; a.m.n_pairs = hdr[4]; a.m.ice_col = hdr[5]; a.m.Neo = hdr[6];
    a.m.mask_el = mask[0]; a.m.mask_nod = mask[1];
    for (int k = 0; k < a.m.n_pairs; ++k) {
        if (first[k] < 0 || first[k] >= n_nod || second[k] < 0 || second[k] >= n_nod) return 6;
        a.m.first[k] = (unsigned char)first[k]; a.m.second[k] = (unsigned char)second[k];
    }
    a.m.miss_val = par[0];
    a.ncols = ncols; a.nrows = nrows; a.Ne = Ne; a.Nn = Nn; a.spacing = par[3];
    std::vector<int> t3(3 * (size_t)Ne), t0(Ne), t1(Ne), t2(Ne), hit(G, -1);
    std::vector<double> x0(Nn), y0(Nn), UM(displaced ? 2 * (size_t)Nn : 0), cs(rotate ? G : 0), sn(rotate ? G : 0), el((size_t)Ne * n_el), nod((size_t)Nn * n_nod),
        grid((size_t)(n_el + n_nod) * G);
    if (!rd(f, t3.data(), 4, t3.size()) || !rd(f, x0.data(), 8, Nn) || !rd(f, y0.data(), 8, Nn) || !rd(f, UM.data(), 8, UM.size()) || !rd(f, cs.data(), 8, cs.size()) ||
        !rd(f, sn.data(), 8, sn.size()) || !rd(f, el.data(), 8, el.size()) || !rd(f, nod.data(), 8, nod.size()) || !rd(f, grid.data(), 8, grid.size()))
        return 4;
    fclose(f);
    for (int e = 0; e < Ne; ++e) {
        t0[e] = t3[3 * e]; t1[e] = t3[3 * e + 1]; t2[e] = t3[3 * e + 2];
        if (t0[e] < 0 || t0[e] >= Nn || t1[e] < 0 || t1[e] >= Nn || t2[e] < 0 || t2[e] >= Nn) return 6;
    }
    // x_grid, y_grid as nxs_dyn_means_regular_set builds them (InterpFromMeshToGridx.cpp:78, 88)
    std::vector<double> xg(ncols), yg(nrows);
    for (int i = 0; i < ncols; ++i) xg[i] = par[1] + par[3] * i;
    for (int i = 0; i < nrows; ++i) yg[nrows - 1 - i] = par[2] - par[3] * i;
    a.xg = xg.data(); a.yg = yg.data();
    a.t0 = t0.data(); a.t1 = t1.data(); a.t2 = t2.data(); a.x0 = x0.data(); a.y0 = y0.data(); a.UM = displaced ? UM.data() : nullptr;
    a.hit = hit.data();
    a.m.cosang = rotate ? cs.data() : nullptr; a.m.sinang = rotate ? sn.data() : nullptr;
    a.m.el = el.data(); a.m.nod = nod.data();
    a.m.grid_el = grid.data(); a.m.grid_nod = grid.data() + (size_t)n_el * G;
    int *h = hit.data();
    for (int k = 0; k < Ne; ++k) {
        const int n = order ? Ne - 1 - k : k;
        nxs_mr::element_hits(a, n, [h, n, G](int g) { if (g >= 0 && g < G && n > h[g]) h[g] = n; });
    }
    std::vector<double> interp_out((size_t)nxs_mp::MAX_VARS * 256, -777.);   // a block's LDS
    for (int g = 0; g < G; ++g) nxs_mr::point(a, g, interp_out.data() + g % 256, 256);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 5;
    fwrite(grid.data(), 8, grid.size(), o);
    fwrite(hit.data(), 4, hit.size(), o);
    fclose(o);
    return 0;
}
