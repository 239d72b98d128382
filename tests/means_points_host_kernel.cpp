// The per-point body of nxs_dyn_means_points_update (nextsim_amd/csrc/nxs_means_points_body.inl) compiled for the HOST: the kernel's own text with the HIP
// qualifiers defined away, one call per grid point as k_means_points makes it (interp_out staged at [nv][256], one column per thread of a block), fed the located
// triangle and its integer area coordinates.  tests/test_means_points_host_kernel.py builds it (g++ -O2 -ffp-contract=off) and requires the bits of the fixture the
// real contrib/bamg wrote (tests/golden/means_points.npz) and of tests/means_points_ref.py.
//   usage: means_points_host_kernel IN OUT
//   IN : int32[10] G, n_el, n_nod, n_pairs, ice_col, Neo, rotate, Ne, Nn, 0; uint32[2] mask_el, mask_nod; int32[12] first; int32[12] second; double miss_val;
//        int32[G] it; int32[3G] the triangle's vertices; int64[3G] dd; rotate: double[G] cos, double[G] sin; double[Ne*n_el] el; double[Nn*n_nod] nod;
//        double[n_el*G] grid_el before; double[n_nod*G] grid_nod before
//   OUT: double[n_el*G] grid_el; double[n_nod*G] grid_nod after
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define __device__
#define __host__
#include "nxs_means_points_body.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[10], first[12], second[12];
    unsigned mask[2];
    nxs_mp::Args a{};
    if (!rd(f, hdr, 4, 10) || !rd(f, mask, 4, 2) || !rd(f, first, 4, 12) || !rd(f, second, 4, 12) || !rd(f, &a.miss_val, 8, 1)) return 4;
    const int G = hdr[0], n_el = hdr[1], n_nod = hdr[2], rotate = hdr[6], Ne = hdr[7], Nn = hdr[8];
    if (G < 0 || n_el < 0 || n_el > nxs_mp::MAX_VARS || n_nod < 0 || n_nod > nxs_mp::MAX_VARS || hdr[3] < 0 || hdr[3] > nxs_mp::MAX_PAIRS) return 6;
    a.G = G; a.n_el = n_el; a.n_nod = n_nod; a.n_pairs = hdr[3]; a.ice_col = hdr[4]; a.Neo = hdr[5];
    a.mask_el = mask[0]; a.mask_nod = mask[1];
    for (int k = 0; k < a.n_pairs; ++k) {
        if (first[k] < 0 || first[k] >= n_nod || second[k] < 0 || second[k] >= n_nod) return 6;
        a.first[k] = (unsigned char)first[k]; a.second[k] = (unsigned char)second[k];
    }
    std::vector<int> it(G), v3(3 * (size_t)G);
    std::vector<long long> dd(3 * (size_t)G);
    std::vector<double> cs(rotate ? G : 0), sn(rotate ? G : 0), el((size_t)Ne * n_el), nod((size_t)Nn * n_nod), grid((size_t)(n_el + n_nod) * G);
    if (!rd(f, it.data(), 4, G) || !rd(f, v3.data(), 4, v3.size()) || !rd(f, dd.data(), 8, dd.size()) || !rd(f, cs.data(), 8, cs.size()) || !rd(f, sn.data(), 8, sn.size()) ||
        !rd(f, el.data(), 8, el.size()) || !rd(f, nod.data(), 8, nod.size()) || !rd(f, grid.data(), 8, grid.size()))
        return 4;
    fclose(f);
    for (int j = 0; j < G; ++j)
        if (it[j] >= Ne || (it[j] >= 0 && (v3[3 * j] < 0 || v3[3 * j] >= Nn || v3[3 * j + 1] < 0 || v3[3 * j + 1] >= Nn || v3[3 * j + 2] < 0 || v3[3 * j + 2] >= Nn))) return 6;
    a.cosang = rotate ? cs.data() : nullptr; a.sinang = rotate ? sn.data() : nullptr;
    a.el = el.data(); a.nod = nod.data();
    a.grid_el = grid.data(); a.grid_nod = grid.data() + (size_t)n_el * G;
    std::vector<double> interp_out((size_t)nxs_mp::MAX_VARS * 256, -777.);   // a block's LDS
    for (int j = 0; j < G; ++j) nxs_mp::point(a, j, it[j], v3[3 * j], v3[3 * j + 1], v3[3 * j + 2], &dd[3 * (size_t)j], interp_out.data() + j % 256, 256);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 5;
    fwrite(grid.data(), 8, grid.size(), g);
    fclose(g);
    return 0;
}
